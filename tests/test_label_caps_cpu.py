"""tests/label_caps.py without a device: the caps are the sources', the tool list is the library's, the tool x family grid is
complete, every scene sits where it says it does, and the tables gathered from prototypes equal the direct restatement."""
import numpy as np
import pytest

import label_caps as LC

FAMILIES = tuple(LC.FAMILIES)


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
    assert set(LC.CAP_SOURCES) == set(c)


def test_python_limits_equal_the_devices():
    assert LC.read_python_limits() == dict(MAX_SIDE=LC.CAPS["kMaxSide"], MAX_BATCH=LC.CAPS["kMaxBatch"], MAX_LABEL=LC.CAPS["kMaxLabel"])


def test_tools_name_every_entry_point_with_a_batch():
    assert sorted(t["entry"] for t in LC.TOOLS.values()) == LC.declared_entry_points()
    assert len({t["entry"] for t in LC.TOOLS.values()}) == len(LC.TOOLS) == 11
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
    assert reasons == {("expand", "labels"): LC.NO_TABLE, ("propagate", "labels"): LC.NO_TABLE, ("expand", "rows"): LC.NO_CAP}
    sat_on = {x["cap"] for t in LC.TOOLS for f in FAMILIES if (t, f) not in reasons for x in LC.scenes(t, f)}
    assert sat_on == set(LC.CAPS) - {"LC_LEVELS"}                                        # every cap has a scene that sits on it
    assert len(LC.nodes()) == sum(len(LC.scenes(t, f)) for t in LC.TOOLS for f in FAMILIES if (t, f) not in reasons)


def _labels_of(x):
    return LC.full(x)["seeds" if x["tool"] == "propagate" else "labels"]


@pytest.mark.parametrize("tool", list(LC.TOOLS))
def test_every_scene_sits_on_its_cap(tool):
    t, C = LC.TOOLS[tool], LC.CAPS
    (x,) = LC.scenes(tool, "batch")
    lab = _labels_of(x)
    assert lab.shape == (C["kMaxBatch"], 8, 8) and lab.max() <= 8 and lab[-1].any() and len(x["protos"][("seeds" if tool == "propagate" else "labels")]) <= 24
    idx = x["index"]
    assert not any(np.array_equal(idx[:-p], idx[p:]) for p in range(1, 2000))            # no small period
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
            B, M = lab.shape[0], x["max_label"]
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
    assert [_labels_of(x).shape for x in sides] == [(2,) + s for s in LC.SIDES] and all(_labels_of(x).any() for x in sides)
    if tool == "propagate":
        x = sides[2]
        assert not x["mask"][:, 1, 1024:3072].any() and x["mask"][:, 1, :1024].all() and x["mask"][:, 0].all()
        lab = LC.expected(x)[0]
        assert (lab[:, 0] > 0).all() and (lab[0, :, 0] == 2).all() and (lab[0, :, -1] == 1).all()       # both seeds grow past the wall


@pytest.mark.parametrize("tool", list(LC.TOOLS))
def test_gathered_tables_equal_the_direct_restatement_at_both_ends(tool):
    """The first 300 and the last 300 images of the batch scene, and of the gathered rows scenes 40 each (their tables are wide)."""
    cases = [(LC.scenes(tool, "batch")[0], 300)]
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
        for g, part in zip(whole, LC.expected(x, B - n, B)):
            if tool == "neighbors" and g.ndim < 3:       # the CSR offsets and the pair list run through the batch
                continue
            assert np.array_equal(g[B - n:], part)


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
