"""The ten label tools, the matcher, the spot detector, the focus and image quality records and the segmenter run at the caps their
argument checks accept (tests/label_caps.py): 65535 images in one call, a label equal to kMaxLabel, each tool's own row, cell, list,
mesh or byte cap met exactly (and, where the library counts before it refuses, missed by one), and the four thin planes with a
side of 4096.  Every node is one (tool, scene); every integer table is compared with np.array_equal, dtype and shape against the
tool's own CPU restatement, texture's clogc within the CLOGC_REL of tests/test_gpu_texture.py.  Behind each cap run the same handle
takes one small ordinary call (input 1 of tests/handle_schedule.py): a buffer grown to the cap and reused small.

Memory kinds: the `labels` scenes and the `rows` scenes of the tools that also have a `rows4` scene go in as CUDA tensors, and their
tables are written on the device and copied to the host here; everything else goes in as numpy arrays and comes back through the
library's own staging, so each tool's tables at its cap take both ways at least once.  measure_dense and match_batch always hand
the library host tables, so DeviceTables stands between such a wrapper and the library for that one call.  The image quality records
take no labels: their scenes with a mesh go in as tensors.  The spot detector writes its tables on the device whenever its images
are tensors, so it needs no proxy.

Sizes: the largest table of a node is texture's marginals at its cell cap, 1 GiB (2^21 rows x 4 directions x 32 int32); the largest
sum of a node's tables is the propagator's, 2.8 GiB on the device at kPgMaxBytes (keys 1 GiB, costs 1 GiB, labels 512 MiB, two
masks of 128 MiB), which is why that scene has no guide and goes in as numpy; label_caps.table_bytes and the CPU test hold every
rows scene under 2 GiB for one table and 4 GiB for all."""
import ctypes as C
import time

import numpy as np
import pytest

import label_caps as LC
from cellscreen import _lib as L
from cellscreen import colocalize as CO
from cellscreen import expand as EX
from cellscreen import granularity as GR
from cellscreen import intensity as IN
from cellscreen import neighbors as NB
from cellscreen import propagate as PG
from cellscreen.preprocess import PIX_U8, PIX_U16
from cellscreen import quality as Q
from cellscreen import quantile as QU
from cellscreen import radial as RA
from cellscreen import score as SC
from cellscreen import segment as S
from cellscreen import shape as SH
from cellscreen import spots as SP
from cellscreen import texture as TX

pytestmark = pytest.mark.gpu

CLOGC_REL = 2.0 ** -40                                   # tests/test_gpu_texture.py
MAKE = {"expand": EX.LabelExpander, "intensity": IN.IntensityMeasurer, "quantiles": QU.QuantileMeasurer, "texture": TX.TextureMeasurer,
        "shape": SH.ShapeMeasurer, "neighbors": NB.NeighborMeasurer, "colocalize": CO.ColocalizationMeasurer, "radial": RA.RadialMeasurer,
        "granularity": GR.GranularityMeasurer, "propagate": PG.LabelPropagator, "match": SC.LabelMatcher, "spots": SP.SpotDetector,
        "focus": Q.ImageQualityMeasurer, "quality": Q.ImageQualityMeasurer}
HAS_ROWS4 = tuple(t for t, d in LC.TOOLS.items() if d["factor"] == 1)


def as_tensor(a):
    import torch
    if a is None:
        return None
    return torch.from_numpy(a.view(np.int16).copy() if a.dtype == np.uint16 else a.copy()).to(torch.device("cuda", 0))


# per entry point: how many table pointers stand in front of out_kind, and how many arguments behind it (include/cellscreen.h)
OUT_ARGS = {"cs_label_intensity": (2, 0), "cs_label_quantiles": (3, 0), "cs_label_texture": (5, 0), "cs_label_shape": (5, 0),
            "cs_label_neighbors": (3, 1), "cs_label_colocalize": (4, 0), "cs_label_radial": (5, 0), "cs_label_granularity": (4, 0),
            "cs_label_match": (2, 1), "cs_image_quality": (2, 0), "cs_object_focus": (2, 0)}


class DeviceTables:
    """The library as a wrapper sees it, but for one entry point: its call gets device tables (CUDA tensors of the shapes and
    types of `want`, filled with -1 so that an entry the call leaves out shows) and out_kind CS_MEM_DEVICE in place of the
    wrapper's host arrays, which are then filled from the tensors.  A null table (no mad, no glcm, no hull) stays null."""

    def __init__(self, lib, entry, want):
        self._lib, self._entry, self._want = lib, entry, want
        self.calls = 0

    def __getattr__(self, name):
        return self._call if name == self._entry else getattr(self._lib, name)

    def _call(self, *args):
        import torch
        n_out, tail = OUT_ARGS[self._entry]
        args = list(args)
        k = len(args) - 1 - tail
        assert args[k] == L.CS_MEM_HOST
        want, filled = iter(self._want), []
        for i in range(k - n_out, k):
            if args[i] is None:
                continue
            w = next(want)
            t = torch.full(w.shape, -1, dtype=getattr(torch, w.dtype.name), device=torch.device("cuda", 0))
            filled.append((args[i], t, w.nbytes))
            args[i] = t.data_ptr()
        args[k] = L.CS_MEM_DEVICE
        torch.cuda.synchronize()                         # the fills are done before the handle's own stream writes
        rc = getattr(self._lib, self._entry)(*args)
        torch.cuda.synchronize()
        self.calls += 1
        if rc == 0:
            for ptr, t, nbytes in filled:
                host = t.cpu().numpy()
                assert host.nbytes == nbytes
                C.memmove(ptr, host.ctypes.data, nbytes)
        return rc


def call(t, x, on_device):
    """One call of a tool on a scene, its tables in the order of the scene's restatement."""
    tool, p = x["tool"], x["params"]
    put = as_tensor if on_device else (lambda a: a)
    if tool == "propagate":
        out = t.propagate_batch(put(x["seeds"]), mask=put(x["mask"]), guide=put(x["guide"]), return_cost=True, **p)
        return tuple(o if isinstance(o, np.ndarray) else o.cpu().numpy() for o in out)
    if tool == "quality":
        return tuple(o for o in t.measure_batch_dense(put(x["image"]), p["tile"], p["sat_level"]) if o is not None)
    lab, image, M = put(x.get("labels")), put(x["image"]), x.get("max_label")
    if tool == "spots":                                  # the response is always asked for; without labels no geom and no records
        prm = SP.spot_params(p["sigma"], sigma_coarse=p["sigma_coarse"], min_distance=p["min_distance"])
        out = t.detect_dense(image, p["threshold"], lab, None, M, prm, True)
        return tuple(o if isinstance(o, np.ndarray) else o.cpu().numpy() for o in out if o is not None)
    if tool == "focus":
        return t.measure_objects_dense(image, lab, max_label=M)
    if tool == "expand":
        out = t.expand_batch(lab, p["distance"], return_d2=True)
        out = tuple(o if isinstance(o, np.ndarray) else o.cpu().numpy() for o in out)
        return out[0], out[1].view(np.uint16) if out[1].dtype == np.int16 else out[1]
    if tool == "intensity":
        return t.measure_dense(image, lab, max_label=M)
    if tool == "quantiles":
        return t.measure_dense(image, lab, p["quantiles"], p["mad"], max_label=M)[:2]
    if tool == "texture":
        return t.measure_dense(image, lab, p["distance"], p["levels"], max_label=M, glcm=p["glcm"])[:4]
    if tool == "shape":
        return t.measure_dense(lab, max_label=M, hull=p["hull"])[:4]
    if tool == "neighbors":
        return t.measure_dense(lab, p["distance"], max_label=M)
    if tool == "colocalize":
        return t.measure_dense(image, lab, max_label=M, threshold=p["threshold"], rwc=p["rwc"])
    if tool == "radial":
        return t.measure_dense(image, lab, max_label=M, bins=p["bins"])[:4]
    if tool == "granularity":
        return t.measure_dense(image, lab, steps=p["steps"], subsample=p["subsample"], max_label=M)[:3]
    if tool == "match":
        m = t.match_batch(lab, put(x["truth"]), max_pred=M, max_truth=x["max_truth"])
        return m.pred, m.truth, m.n_pairs
    raise KeyError(tool)


def same(tool, got, want, what):
    assert len(got) == len(want), what
    floats = LC.TOOLS[tool].get("float_outputs", ())
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        if i in floats:
            err = np.abs(g - w)
            print(f"{what}: table {i}, largest |dev - ref| / ref = {float(np.max(err[w > 0] / w[w > 0], initial=0.0)):.3e}")
            assert (err <= CLOGC_REL * w).all(), (what, i)
        else:
            assert np.array_equal(g, w), (what, i, int((g != w).sum()))


def absent_rows_are_empty(x, got):
    """The rows of the labels an image does not hold, over the whole table: all zero, and for the neighbours an empty CSR row."""
    tool = x["tool"]
    absent = LC.absent_rows(x)
    assert absent.any() and not absent.all()
    for i, g in enumerate(got):
        if tool == "match" and i == 1:
            a = LC.absent_rows(dict(labels=x["truth"], max_label=x["max_truth"]))
        elif g.ndim >= 2 and g.shape[:2] == absent.shape:
            a = absent
        elif tool == "neighbors" and i == 2:
            assert not np.diff(g).reshape(absent.shape)[absent].any(), (tool, x["name"], i)
            continue
        else:
            continue                                    # a table per image, or the pair list
        assert not g[a].any(), (tool, x["name"], i, int(g[a].reshape(a.sum(), -1).any(axis=1).sum()))


def run_node(tool, family, n):
    x = LC.full(LC.scenes(tool, family)[n])
    want = LC.expected(LC.scenes(tool, family)[n])                                # outside the times below
    small = LC.small_scene(tool)
    small_want = LC.expected(small)
    on_device = family == "labels" or x["name"] == "rows-scratch" or (x["name"] == "rows" and tool in HAS_ROWS4) or \
        (tool == "quality" and x["params"]["tile"] > 0)
    what = f"{tool} {x['name']} on {x['cap']}, tensors={on_device}"
    t = MAKE[tool](0)
    try:
        entry, lib = LC.TOOLS[tool]["entry"], t._lib
        if on_device and entry in OUT_ARGS:
            t._lib = DeviceTables(lib, entry, want)
        t0 = time.perf_counter()
        got = call(t, x, on_device)
        t1 = time.perf_counter()
        timing = t.last_timing()                         # the cap call's own, before the small call replaces it
        assert not isinstance(t._lib, DeviceTables) or t._lib.calls == 1
        t._lib = lib
        same(tool, got, want, what)
        # the spots-list scene has every row present (tests/test_label_caps_cpu.py), the image quality records have no label rows
        if family in ("labels", "rows") and tool != "propagate" and tool not in LC.LABEL_FREE and x["name"] != "spots-list":
            absent_rows_are_empty(x, got)
        del got, want
        t2 = time.perf_counter()
        same(tool, call(t, small, not on_device), small_want, f"{tool}, small, behind {x['name']}")
        print(f"\n{what}: {t1 - t0:.2f} s the call, {time.perf_counter() - t2:.2f} s the small call behind it; device {timing}")
    finally:
        t.close()


def ids_of(family):
    return [pytest.param(t, f, n, id=f"{t}-{LC.scenes(t, f)[n]['name'].replace(' ', '-')}") for t, f, n in LC.nodes() if f == family]


@pytest.mark.parametrize("tool,family,n", ids_of("batch"))
def test_batch_of_65535_images(tool, family, n):
    run_node(tool, family, n)


@pytest.mark.parametrize("tool,family,n", ids_of("labels"))
def test_label_equal_to_the_largest(tool, family, n):
    run_node(tool, family, n)


@pytest.mark.parametrize("tool,family,n", ids_of("rows"))
def test_row_cell_or_byte_cap_met_exactly(tool, family, n):
    run_node(tool, family, n)


@pytest.mark.parametrize("tool,family,n", ids_of("sides"))
def test_thin_planes_with_a_side_of_4096(tool, family, n):
    run_node(tool, family, n)


CS_ERR_INVALID, CS_ERR_UNSUPPORTED = -1, -6              # include/cellscreen.h


def small_call_is_right(t, tool, behind):
    small = LC.small_scene(tool)
    same(tool, call(t, small, True), LC.expected(small), f"{tool}, small, behind {behind}")


def test_one_spot_more_than_the_list_holds_is_refused():
    """The spots-list scene's images and one more with one bright pixel, without labels: cs_spot_detect finds 2^22 + 1 spots, writes
    the first 2^22 (no position at or beyond the capacity is stored), and refuses the call once it has read the count; no list is
    left for cs_spot_fill, and the handle takes the small call."""
    x = LC.spots_over_the_list()
    t = SP.SpotDetector(0)
    try:
        t0 = time.perf_counter()
        with pytest.raises(L.CellScreenError) as ei:
            call(t, x, False)
        dt, timing = time.perf_counter() - t0, t.last_timing()
        assert ei.value.status == CS_ERR_UNSUPPORTED and "capped at" in str(ei.value) and f"{LC.CAPS['kSdMaxSpots'] + 1} spots" in str(ei.value)
        offsets = np.zeros(len(x["image"]) + 1, np.int64)
        assert t._lib.cs_spot_fill(t._handle, None, 0, L._ptr(offsets), L.CS_MEM_HOST) == CS_ERR_INVALID
        assert "no spot list" in t._lib.cs_last_error().decode() and not offsets.any()
        small_call_is_right(t, "spots", "a refused list")
        print(f"\nspots, one above kSdMaxSpots: {dt:.2f} s the refused call; device {timing}")
    finally:
        t.close()


def test_one_image_more_than_the_spot_scratch_holds_is_refused():
    """21846 images of 64 x 64 need 2^30 bytes of scratch or more: refused by the wrapper, and by the entry point itself before it
    touches the device, so a one-image buffer stands in for the stack."""
    B, s = LC.scratch_batch() + 1, LC.SCRATCH_SIDE
    t = SP.SpotDetector(0)
    try:
        with pytest.raises(ValueError, match="scratch"):
            t.detect_dense(np.zeros((B, s, s), np.uint16), 1.0)
        img, thr, counts, n = np.zeros((1, s, s), np.uint16), np.full(B, 256, np.int32), np.full((1, 2), -1, np.int64), C.c_int64(-1)
        prm = SP.spot_params(LC.SPOTS["sigma"], sigma_coarse=LC.SPOTS["sigma_coarse"], min_distance=LC.SPOTS["min_distance"])
        for batch, status in ((B, CS_ERR_UNSUPPORTED), (1, 0)):                  # and the same arguments with one image are taken
            rc = t._lib.cs_spot_detect(t._handle, L._ptr(img), PIX_U16, 1, None, None, batch, s, s, L.CS_MEM_HOST, 0, C.byref(prm), L._ptr(thr),
                                       L._ptr(counts), None, None, None, L.CS_MEM_HOST, C.byref(n))
            assert rc == status, (batch, rc, t._lib.cs_last_error().decode())
            if status:
                assert "scratch" in t._lib.cs_last_error().decode() and n.value == -1 and (counts == -1).all()
        assert n.value == 0 and not counts.any()
        small_call_is_right(t, "spots", "a refused stack")
    finally:
        t.close()


def test_one_image_more_than_the_mesh_holds_is_refused():
    """32769 images x 4 channels x a mesh of 2 x 4 are 2^20 + 32 tiles: refused by the wrapper and by the entry point."""
    (x,) = LC.scenes("quality", "rows")
    B, (H, W), tile, nc = x["batch"] + 1, LC.TILES_SHAPE, LC.TILES_TILE, LC.CAPS["kIqMaxChannels"]
    t = Q.ImageQualityMeasurer(0)
    try:
        with pytest.raises(ValueError, match="tiles"):
            t.measure_batch_dense(np.zeros((B, H, W, nc), np.uint8), tile=tile)
        img, records, mesh = np.zeros((1, H, W, nc), np.uint8), np.full((1, nc, 13), -1, np.int64), np.full((1, nc, 2, 4, 8), -1, np.int64)
        for batch, status in ((B, CS_ERR_UNSUPPORTED), (1, 0)):
            rc = t._lib.cs_image_quality(t._handle, L._ptr(img), PIX_U8, nc, batch, H, W, L.CS_MEM_HOST, tile, None, L._ptr(records), L._ptr(mesh),
                                         L.CS_MEM_HOST)
            assert rc == status, (batch, rc, t._lib.cs_last_error().decode())
            if status:
                assert "capped at" in t._lib.cs_last_error().decode() and (records == -1).all() and (mesh == -1).all()
        assert records[0, :, 0].tolist() == [H * W] * nc and mesh[..., 0].sum() == nc * H * W
        small_call_is_right(t, "quality", "a refused stack")
    finally:
        t.close()


@pytest.mark.parametrize("case", list(LC.SEGMENT_CASES))
def test_segmenter_on_65535_images(case):
    images, _ = LC.segment_scene()
    opts = LC.SEGMENT_CASES[case]
    want = LC.segment_expected(case)
    seg = S.ThresholdSegmenter(0, **opts)
    try:
        t0 = time.perf_counter()
        got = seg.segment_batch(images, return_distance=bool(opts.get("split_touching")))
        dt = time.perf_counter() - t0
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            g = np.asarray(g)
            assert g.dtype == w.dtype and g.shape == w.shape, (case, i, g.dtype, w.dtype, g.shape, w.shape)
            assert np.array_equal(g, w), (case, i, int((g != w).sum()), np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:5])
        print(f"\nsegmenter {case} on {images.shape}: {dt:.2f} s")
    finally:
        seg.close()
