"""tests/label_caps.py without a device: the caps are the sources', the tool list is the library's, the tool x family grid is
complete, every scene sits where it says it does, and the tables gathered from prototypes equal the direct restatement."""
import numpy as np
import pytest

import label_caps as LC
from cellscreen import intensity as IN
from cellscreen import quality as Q
from cellscreen import spots as SP

FAMILIES = tuple(LC.FAMILIES)
RUNNING = {"neighbors": (2, 3), "spots": (1, 2)}         # the tables that have no image axis: label_caps.gather


def test_caps_are_read_from_the_sources_and_pinned():
    c = LC.read_caps()
    assert c == LC.CAPS
    assert (c["kMaxSide"], c["kMaxBatch"], c["kMaxLabel"]) == (4096, 65535, 1 << 20)
    for name in ("kLiMaxCells", "kLqMaxCells", "kShMaxRows", "kNbMaxRows", "kLcMaxCells", "kLrMaxCells", "kGrMaxCells", "kLmMaxRows"):
        assert c[name] == 1 << 22, name
    assert c["kTxMaxCells"] == 1 << 24
    for name in ("kLrMaxRing", "kGrMaxBytes", "kLcMaxScratch", "kPgMaxBytes"):
        assert c[name] == 1 << 30, name
    assert c["LC_LEVELS"] == 65536
    assert (c["kSdMaxRows"], c["kSdMaxSpots"], c["kSdMaxScratch"]) == (1 << 22, 1 << 22, 1 << 30)
    assert (c["kIqMaxTiles"], c["kLfMaxCells"], c["kIqMaxChannels"]) == (1 << 20, 1 << 22, 4)
    assert set(LC.CAP_SOURCES) == set(c)


def test_python_limits_equal_the_devices():
    assert LC.read_python_limits() == dict(MAX_SIDE=LC.CAPS["kMaxSide"], MAX_BATCH=LC.CAPS["kMaxBatch"], MAX_LABEL=LC.CAPS["kMaxLabel"])
    c = LC.CAPS
    text = {("spots", "MAX_ROWS"): c["kSdMaxRows"], ("spots", "MAX_SPOTS"): c["kSdMaxSpots"], ("spots", "MAX_SCRATCH"): c["kSdMaxScratch"],
            ("quality", "MAX_TILES"): c["kIqMaxTiles"], ("quality", "MAX_CHANNELS"): c["kIqMaxChannels"]}
    assert LC.read_tool_limits() == text
    for (mod, name), v in text.items():                  # and as the modules hold them once imported
        assert getattr({"spots": SP, "quality": Q}[mod], name) == v, (mod, name)
    assert IN.MAX_CELLS == c["kLfMaxCells"]              # the focus records borrow the intensity measurer's size check


def test_tools_name_every_entry_point_with_a_batch():
    assert sorted(t["entry"] for t in LC.TOOLS.values()) == LC.declared_entry_points()
    assert len({t["entry"] for t in LC.TOOLS.values()}) == len(LC.TOOLS) == 14
    body = LC.defined_entry_points()                     # the rule that finds them reads the definitions, not the names
    with_state = {n for n, text in body.items() if "state_begin(" in text}
    assert {"cs_spot_detect", "cs_image_quality", "cs_object_focus"} <= with_state and "cs_label_match" not in with_state
    assert not any(n.startswith("cs_segment_") for n in LC.declared_entry_points()) and "cs_spot_fill" not in with_state
    for name, t in LC.TOOLS.items():
        assert set(t["caps"]) <= set(LC.CAPS), name
        assert (name in LC.ROW_CAP) == (t["factor"] > 0) and (name not in LC.ROW_CAP or LC.ROW_CAP[name] in t["caps"]), name
    used = {c for t in LC.TOOLS.values() for c in t["caps"]} | {"kMaxSide", "kMaxBatch", "LC_LEVELS"}
    assert used == set(LC.CAPS)                          # no cap without a tool that is run against it


def test_the_grid_is_a_scene_or_a_written_reason():
    reasons = {}
    for tool in LC.TOOLS:
        for family in FAMILIES:
            s = LC.scenes(tool, family)
            if isinstance(s, str):
                assert s in LC.REASONS
                reasons[tool, family] = s
            else:
                assert isinstance(s, list) and s and all(x["tool"] == tool for x in s)
    assert reasons == {("expand", "labels"): LC.NO_TABLE, ("propagate", "labels"): LC.NO_TABLE, ("expand", "rows"): LC.NO_CAP,
                       ("quality", "labels"): LC.NO_LABELS}
    sat_on = {x["cap"] for t in LC.TOOLS for f in FAMILIES if (t, f) not in reasons for x in LC.scenes(t, f)}
    assert sat_on == set(LC.CAPS) - {"LC_LEVELS"}                                        # every cap has a scene that sits on it
    assert len(LC.nodes()) == sum(len(LC.scenes(t, f)) for t in LC.TOOLS for f in FAMILIES if (t, f) not in reasons)


def _labels_of(x):
    """The planes a scene is made on: the labels, the propagator's seeds, or the image of a tool that takes no labels."""
    return LC.planes_of(x)


@pytest.mark.parametrize("tool", list(LC.TOOLS))
def test_every_scene_sits_on_its_cap(tool):
    t, C = LC.TOOLS[tool], LC.CAPS
    batch = LC.scenes(tool, "batch")
    assert [x["cap"] for x in batch] == (["kMaxBatch", "kIqMaxChannels"] if tool == "quality" else ["kMaxBatch"])
    for x in batch:
        lab = _labels_of(x)
        key = "image" if tool in LC.LABEL_FREE else "seeds" if tool == "propagate" else "labels"
        assert lab.shape[:3] == (C["kMaxBatch"], 8, 8) and lab[-1].any() and len(x["protos"][key]) <= 24
        assert lab.max() <= 8 if tool not in LC.LABEL_FREE else lab.shape[3:] == ((4,) if x["cap"] == "kIqMaxChannels" else ())
        idx = x["index"]
        assert not any(np.array_equal(idx[:-p], idx[p:]) for p in range(1, 2000))        # no small period
    if not isinstance(LC.scenes(tool, "labels"), str):
        (x,) = LC.scenes(tool, "labels")
        top = C["kMaxLabel"]
        assert x["labels"].shape == (2, 40, 300) and x["max_label"] == top
        assert sorted(np.unique(x["labels"][0]).tolist()) == [0, 1, 2, 1000, top - 1, top]
        assert sorted(np.unique(x["labels"][1]).tolist()) == [0, 2, top] and (x["labels"][1, :, 0] == top).all()
        a = x["labels"][0]
        for lo, hi in ((1, 2), (top - 1, top)):          # adjacent along a row
            assert ((a[:, :-1] == lo) & (a[:, 1:] == hi)).any()
        if tool == "match":
            assert x["max_truth"] == top
        if tool == "neighbors":
            assert len(LC.expected(x)[3]) > 0
    rows = LC.scenes(tool, "rows")
    if not isinstance(rows, str):
        for x in rows:
            lab = _labels_of(x)
            if tool == "propagate":
                assert lab.size * 8 == C["kPgMaxBytes"] and x["cap"] == "kPgMaxBytes" and lab.max() == C["kMaxLabel"]
                continue
            big, total = LC.table_bytes(x)
            assert big < 2 << 30 and total < 4 << 30, (tool, x["name"], big, total)
            if tool == "quality":                        # 32768 images x 4 channels x a mesh of 2 x 4, off the pixel grid
                B, H, W, ch = lab.shape
                m_r, m_c = LC.QY.mesh_dims(H, W, x["params"]["tile"])
                assert x["cap"] == "kIqMaxTiles" and B * ch * m_r * m_c == C["kIqMaxTiles"] and ch == C["kIqMaxChannels"]
                assert (m_r, m_c) == (2, 4) and H % m_r and W % m_c and lab.dtype == np.uint8 and (B + 1) * ch * m_r * m_c > C["kIqMaxTiles"]
                continue
            B, M = lab.shape[0], x["max_label"]
            if x["cap"] in ("kSdMaxSpots", "kSdMaxScratch"):                  # test_spot_scenes_meet_their_conditions
                assert lab.shape[1:] == (64, 64) and B * M <= C["kSdMaxRows"]
                continue
            if x["name"] == "rows-channels":             # the cells are rows x channels
                ch = LC.full(x)["image"].shape[3]
                assert x["cap"] == LC.ROW_CAP[tool] and B * M * ch == C[x["cap"]] and ch == C["kIqMaxChannels"] and B == 4096
                assert 1 in lab and M in lab and lab[-1].max() == M and lab.shape[1:] == (16, 16)
                crowded = [b for b in range(40) if len(np.unique(lab[b])) == M]           # as many objects as the table has slots
                assert M == 256 and crowded and len(crowded) < 40
                continue
            if x["cap"] == "kLcMaxScratch":
                per = B * t["channels"] * LC.LC_SCRATCH_PER
                assert x["params"]["rwc"] and per <= C["kLcMaxScratch"] < per + t["channels"] * LC.LC_SCRATCH_PER
                continue
            if x["name"] == "rows-bytes":
                widest = {"radial": x["params"].get("bins", 0) * 8 * 2 * 8, "granularity": (x["params"].get("steps", 0) + 1) * 8}[tool]
                assert B * M * widest == C[x["cap"]] == LC.table_bytes(x)[0] and x["cap"] in t["caps"] and x["cap"] != LC.ROW_CAP[tool]
            else:
                assert x["cap"] == LC.ROW_CAP[tool], (tool, x["name"])
            assert B * M * t["factor"] == C[LC.ROW_CAP[tool]], (tool, x["name"])
            assert B in (4096, 4) and lab.shape[1:] == (16, 16) and M < C["kMaxLabel"] or B == 4 and M == C["kMaxLabel"]
            present = np.unique(lab)
            assert 1 in present and M in present and len(present) <= 8 and lab[-1].max() == M
            big, total = LC.table_bytes(x)
            assert big < 2 << 30 and total < 4 << 30, (tool, big, total)
        assert any(x["name"] == "rows4" and x["labels"].shape[0] == 4 for x in rows) == (t["factor"] == 1)
    sides = LC.scenes(tool, "sides")
    per = 2 if tool == "quality" else 1                  # without a mesh and with one
    assert [_labels_of(x).shape for x in sides] == [(2,) + s for s in LC.SIDES for _ in range(per)] and all(_labels_of(x).any() for x in sides)
    if tool == "quality":
        assert [x["params"]["tile"] for x in sides] == [0, 16] * 4 and all(np.array_equal(a["image"], b["image"]) for a, b in zip(sides[::2], sides[1::2]))
    if tool == "spots":                                  # both tables at the largest radius, the window at its widest
        for x in sides:
            w_a, w_b, m, T = LC.spot_tables(x["params"])
            assert (len(w_a) - 1, len(w_b) - 1, m, T) == (64, 64, 8, 256) and LC.expected(x)[0][:, 0].min() > 0
    if tool == "propagate":
        x = sides[2]
        assert not x["mask"][:, 1, 1024:3072].any() and x["mask"][:, 1, :1024].all() and x["mask"][:, 0].all()
        lab = LC.expected(x)[0]
        assert (lab[:, 0] > 0).all() and (lab[0, :, 0] == 2).all() and (lab[0, :, -1] == 1).all()       # both seeds grow past the wall


@pytest.mark.parametrize("tool", list(LC.TOOLS))
def test_gathered_tables_equal_the_direct_restatement_at_both_ends(tool):
    """The first 300 and the last 300 images of the batch scene, and of the gathered rows scenes 40 each (their tables are wide)."""
    cases = [(x, 300) for x in LC.scenes(tool, "batch")]
    rows = LC.scenes(tool, "rows")
    if not isinstance(rows, str):
        cases += [(x, 40) for x in rows if "index" in x]
    for x, n in cases:
        B = len(x["index"])
        for lo, hi in ((0, n), (B - n, B)):
            got, want = LC.expected(x, lo, hi), LC.restate(LC.full(x, lo, hi))
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (tool, x["name"], lo)
        whole = LC.expected(x)
        for i, (g, part) in enumerate(zip(whole, LC.expected(x, B - n, B))):
            if i in RUNNING.get(tool, ()):               # the offsets and the pair or spot list run through the batch
                continue
            assert np.array_equal(g[B - n:], part)
        if tool == "spots":                              # and the tail of what runs through equals the part's, moved to 0
            lo = whole[1][B - n]
            part = LC.expected(x, B - n, B)
            assert np.array_equal(whole[1][B - n:] - lo, part[1]) and np.array_equal(whole[2][lo:], part[2]) and whole[1][-1] == len(whole[2])
            assert np.array_equal(np.diff(whole[1]), whole[0][:, 0])


def test_neighbor_gather_keeps_the_csr_whole():
    (x,) = LC.scenes("neighbors", "batch")
    geom, objects, offsets, pairs = LC.expected(x)
    B, M = geom.shape[:2]
    assert offsets.shape == (B * M + 1,) and offsets[0] == 0 and offsets[-1] == len(pairs) > 0 and (np.diff(offsets) >= 0).all()
    assert np.array_equal(np.diff(offsets), objects[..., 2].reshape(-1))                 # a row's length is its degree
    lo = (B - 300) * M
    want = LC.restate(LC.full(x, B - 300, B))
    assert np.array_equal(pairs[offsets[lo]:], want[3]) and np.array_equal(offsets[lo:] - offsets[lo], want[2])


def test_absent_rows_and_what_a_wrong_stride_would_leave():
    """What each family's expected tables hold that one wrong line would miss: a non-zero row beyond the first 2^20
    cells; a last image whose rows differ from every image's a 16-bit or short batch index would read; the largest label's row
    non-zero; the last column tile of a 4096 row non-empty."""
    x = LC.scenes("intensity", "rows")[0]
    geom = LC.expected(x)[0].reshape(-1, 3)
    assert geom.shape[0] == 1 << 22 and geom[1 << 20:].any() and geom[-1].any() and geom[3 << 20:].any()
    absent = LC.absent_rows(x)
    assert absent.shape == (4096, 1024) and not LC.expected(x)[0][absent].any() and LC.expected(x)[0][~absent].all(axis=-1).sum() > 0
    lo = LC.expected(x)[1].reshape(-1, 6)[1 << 20:, 4]                                   # the minimum, which li_close decodes
    assert ((lo > 0) & (lo != 65536 - lo)).any()
    xn = LC.scenes("neighbors", "rows")[0]
    objects, offsets = LC.expected(xn)[1:3]
    assert objects[-1, :, 2].sum() > 0 and objects[-1, -1, 2] > 0 and offsets[-1] > offsets[-2]       # pairs in the last CSR row
    x4 = LC.scenes("intensity", "rows")[1]
    assert LC.expected(x4)[0][3, -1].any()                                               # row 2^22 - 1 itself
    xb = LC.scenes("intensity", "batch")[0]
    g = LC.expected(xb)[0]
    assert g[-1].any() and not np.array_equal(g[-1], g[65534 - 32768]) and not np.array_equal(g[-1], g[-2])
    xl = LC.scenes("quantiles", "labels")[0]
    count = LC.expected(xl)[0]
    assert count[0, 0] > 0 and count[0, -1] > 0 and count[0, -2] > 0 and count[1, -1] == 40 and count[:, 2:999].sum() == 0
    for xs in LC.scenes("shape", "sides"):
        H, W = xs["labels"].shape[1:]
        assert xs["labels"][:, :, W - min(W, 64):].any() and xs["labels"][:, H - min(H, 16):, :].any()


def test_texture_restated_on_renumbered_ids_is_the_direct_form():
    top = LC.SPARSE_ABOVE + 904
    x = LC._scene("texture", "labels", LC.labels_planes(top), top, 31, None)
    ids = np.unique(x["labels"])
    assert len(ids) == 6 and ids.max() == top
    img = x["image"]
    direct = LC.TR.measure(img, x["labels"], 1, LC.TEXTURE_LEVELS, LC.TR.full_range(img.dtype.type, 1), None, top, False)[:4]
    for g, w in zip(LC.restate(x), direct):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert direct[0][0, -1] > 0 and direct[1][0, -1].any() and direct[3][0, -1].any()


def test_the_small_call_is_input_one_of_the_shared_handle():
    for tool in LC.TOOLS:
        x = LC.small_scene(tool)
        assert _labels_of(x).shape == (1, 33, 67) and x["tool"] == tool and "index" not in x
        assert any(a.any() for a in LC.expected(x))


# ---- the spots, the focus records and the image quality records -------------------------------------------------------------------
LDS_SLOTS, PLACE_ROWS, TILE_ROWS, TILE_COLS = 512, 256, 64, 256          # spots.hip: 1 << SD_SLOTS_LOG2, SD_CHUNK; label_tile.hpp


def test_spot_tables_are_those_of_spot_params():
    for p in (LC.SPOTS, LC.SPOTS_WIDE):
        w_a, w_b, m, T = LC.spot_tables(p)
        prm = SP.spot_params(p["sigma"], sigma_coarse=p["sigma_coarse"], min_distance=m)
        assert SP.tables_of(prm) == ([65536] if w_a is None else w_a, w_b) and prm.min_distance == m and prm.channel == 0
        assert T == int(round(256 * p["threshold"])) == 256
    assert LC.spot_tables(LC.SPOTS)[0] is None and len(LC.spot_tables(LC.SPOTS)[1]) - 1 == 4
    rows, ra, rb, e = 64, 64, 64, 4                      # sd_cols_lds at H >= 64 under SPOTS_WIDE: its largest request
    assert (2 * rows + 2 * ra + 2 * rb + 2 * e) * 64 * 4 == 100352 > 64 << 10


def test_spot_scenes_meet_their_conditions():
    C = LC.CAPS
    (xb,) = LC.scenes("spots", "batch")
    counts, offsets, lst = LC.expected(xb)[:3]
    assert offsets[-1] == len(lst) > C["kMaxBatch"] and counts[-1, 0] > counts[-1, 1]      # the last image: a spot inside an object
    (xl,) = LC.scenes("spots", "labels")
    records = LC.expected(xl)[4]
    top = C["kMaxLabel"]
    assert records[0, 0, 0] >= 1 and records[0, top - 2, 0] >= 1 and records[0, top - 1, 0] >= 1 and records[1, top - 1, 0] >= 1
    rows = {x["name"]: x for x in LC.scenes("spots", "rows")}
    assert list(rows) == ["rows", "rows4", "spots-list", "scratch"]
    for name in ("rows", "rows4"):
        lab = LC.full(rows[name])["labels"]
        assert lab.shape[0] * rows[name]["max_label"] == C["kSdMaxRows"] and LC.expected(rows[name])[4][..., 0].sum() > 0

    x = rows["spots-list"]                               # 2^22 spots, 2^22 table rows, and a capacity bound of 2^22, all at once
    lab, m = LC.full(x)["labels"], x["params"]["min_distance"]
    B, H, W = lab.shape
    counts, offsets, lst, geom, records, _ = LC.expected(x)
    assert offsets[-1] == len(lst) == C["kSdMaxSpots"]
    assert B * x["max_label"] == C["kSdMaxRows"] == C["kSdMaxSpots"]
    assert B * -(-H // (m + 1)) * -(-W // (m + 1)) == C["kSdMaxSpots"]                     # capacity, as cs_spot_detect bounds it
    assert B * H * W * 12 < C["kSdMaxScratch"]
    assert (counts == [1024, 0]).all() and (records[..., 0] == 1).all() and (geom[..., 0] == 4).all()       # one spot in every object
    assert PLACE_ROWS // H * x["max_label"] == 4096 > LDS_SLOTS                          # the table rows an sd_place workgroup meets
    assert H <= TILE_ROWS and W <= TILE_COLS and len(np.unique(lab[0])) == 1024 > LDS_SLOTS                  # the labels of an sd_geom tile
    protos = x["protos"]
    assert protos["image"].dtype == np.uint8 and protos["image"][:, 1::2].max() < 40 and protos["image"][:, ::2, ::2].min() >= 200
    assert len({a.tobytes() for a in protos["image"]}) == len(protos["image"]) == 6
    flat = np.zeros((1, H, W), np.uint16)                # the count does not hang on the noise: a flat lattice gives it too
    flat[:, ::2, ::2] = 200
    assert LC.restate(dict(tool="spots", image=flat, params=x["params"]))[0].tolist() == [[1024, 1024]]

    over = LC.spots_over_the_list()                      # one spot more, without labels
    assert over["image"].shape == (B + 1, H, W) and np.array_equal(over["image"][:B], LC.full(x)["image"]) and "labels" not in over
    last = LC.restate(dict(over, image=over["image"][B:]))
    assert last[0].tolist() == [[1, 1]] and last[2][0, :2].tolist() == [33, 21]
    assert (B + 1) * H * W * 12 < C["kSdMaxScratch"]     # refused for the list's length alone

    x = rows["scratch"]
    lab = LC.full(x)["labels"]
    B, H, W = lab.shape
    assert B == LC.scratch_batch() == 21845 and B * H * W * 12 == 1073725440 < C["kSdMaxScratch"] <= (B + 1) * H * W * 12
    counts, offsets = LC.expected(x)[:2]
    assert 0 < offsets[-1] < C["kSdMaxSpots"] and counts[-1, 0] > 0 and (counts[:, 0] == 0).any()
    assert sorted(set(counts[:, 0].tolist())) == [0, 1, 2, 5, 16]              # of two equal neighbours only the first is a spot


def test_focus_and_quality_scenes_meet_their_conditions():
    C = LC.CAPS
    rows = {x["name"]: x for x in LC.scenes("focus", "rows")}
    assert list(rows) == ["rows", "rows4", "rows-channels"]
    x = rows["rows-channels"]
    geom, focus = LC.expected(x)
    assert focus.shape == (4096, 256, 4, 5) and focus.size // 5 == C["kLfMaxCells"] and focus[-1, -1].all() and geom[-1, -1, 0] > 0
    assert not any(np.array_equal(focus[:, :, 0], focus[:, :, c]) for c in (1, 2, 3))      # four different channels
    (xt,) = LC.scenes("quality", "rows")
    records, mesh = LC.expected(xt)
    assert mesh.shape == (32768, 4, 2, 4, 8) and mesh.size // 8 == C["kIqMaxTiles"] and mesh[-1, -1, -1, -1].any()
    assert np.array_equal(mesh.sum(axis=(2, 3)), records[:, :, [0, 1, 2, 8, 9, 10, 11, 12]])
    assert len(np.unique(mesh[0, 0, :, :, 0])) > 1       # off the pixel grid: the tiles differ in size
    one, many = LC.scenes("quality", "batch")
    assert LC.expected(one)[0].shape == (65535, 1, 13) and LC.expected(many)[0].shape == (65535, 4, 13)
    r = LC.expected(many)[0]
    assert not np.array_equal(r[-1], r[-2]) and not np.array_equal(r[-1], r[65534 - 32768]) and r[-1, 3].any()


# ---- the segmenter --------------------------------------------------------------------------------------------------------------
def test_segmenter_scene_and_its_gather():
    protos = LC.segment_protos()
    images, index = LC.segment_scene()
    assert protos.shape == (24, 8, 8) and images.shape == (LC.MAX_BATCH, 8, 8) and images.dtype == np.uint16
    assert not any(np.array_equal(index[:-p], index[p:]) for p in range(1, 2000))
    assert set(LC.SEGMENT_CASES) == {"default", "split", "split_intensity", "local", "noise"}
    for case in LC.SEGMENT_CASES:
        tabs = LC._segment_proto_tables(case)
        assert tabs[1].max() >= 2 and tabs[1][index[-1]] >= 1, case                      # objects, and some in the last image
        for lo, hi in ((0, 300), (LC.MAX_BATCH - 300, LC.MAX_BATCH)):
            got, want = LC.segment_expected(case, lo, hi), LC.segment_restate(images[lo:hi], case)
            assert len(got) == len(want) == (4 if LC.SEGMENT_CASES[case].get("split_touching") else 3)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), case
