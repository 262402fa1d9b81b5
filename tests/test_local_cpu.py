"""CPU tests of the segmenter's local mean threshold (cs_segment_local, ThresholdSegmenter(threshold="local", ...)): the
restatement of tests/local_reference.py against windows summed one by one and against scikit-image's threshold_local
(tests/golden/golden_local.npz), the tie rule, the field of bright and dim cells that the option exists for, and the wrapper's
and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import local_reference as LR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import segment as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_local.npz")


def inputs(shape, dtype, seed=0):
    """(name, image): noise over the full range, constant, a ramp, one bright pixel, saturated."""
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(seed + 1000 * shape[0] + shape[1])
    H, W = shape
    bright = np.full(shape, top // 5, dtype)
    bright[H // 2, W // 3] = top
    ramp = ((np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5) % (top + 1)).astype(dtype)
    return [("noise", rng.integers(0, top + 1, shape).astype(dtype)), ("constant", np.full(shape, top // 3, dtype)), ("ramp", ramp),
            ("bright", bright), ("saturated", np.full(shape, top, dtype))]


def dim_cell_scene(seed, side=512, n_cells=40, sigma=25.0):
    """A field of bright and dim cells: uint16, background 300 with Gaussian noise of `sigma` counts, n_cells separated
    flat-topped blobs of radius 9..15, alternately of peak 6000 and 900.  Returns (image, [(y, x, radius, peak)])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    cells = []
    while len(cells) < n_cells:
        y, x = (int(v) for v in rng.integers(25, side - 25, 2))
        rad = int(rng.integers(9, 16))
        if all((y - cy) ** 2 + (x - cx) ** 2 > (rad + cr + 6) ** 2 for cy, cx, cr, _ in cells):
            cells.append((y, x, rad, (6000, 900)[len(cells) % 2]))
    img = 300.0 + rng.normal(0.0, sigma, (side, side))
    for y, x, rad, peak in cells:
        img += peak * np.exp(-((((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (rad / 1.6) ** 2)) ** 2))
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16), cells


SCENE_R, SCENE_DELTA = 25, 60           # a 51 x 51 window, wider than the widest cell (31 px); 60 counts: 2.4 noise sigmas


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_restatement_equals_windows_summed_one_by_one(dtype):
    for shape in ((1, 1), (1, 7), (7, 1), (5, 7), (9, 4), (12, 13)):
        for name, x in inputs(shape, dtype):
            for r in (1, 2, 3, 7, 13, 30):                           # 7, 13 and 30 reach or exceed the sides: the fold wraps
                want = LR.window_sum_direct(x, r)
                assert np.array_equal(LR.window_sum(x, r), want), (shape, name, r)
                n = (2 * r + 1) ** 2
                for delta in (-3, 0, 5):
                    for floor in (-1, int(np.iinfo(dtype).max) // 2):
                        m = (n * x.astype(np.int64) - want - n * delta > 0) & (x.astype(np.int64) > floor)
                        assert np.array_equal(LR.local_mask(x, r, delta, floor), m.astype(np.uint8)), (shape, name, r, delta, floor)


def test_fold_is_numpy_s_symmetric_padding():
    for n in (1, 2, 3, 8):
        line = np.arange(n)
        for r in (1, 5, 17):
            assert np.array_equal(LR.fold(np.arange(-r, n + r), n), np.pad(line, r, mode="symmetric"))


def test_median_stands_on_both_sides():
    import background_reference as BR
    x = inputs((37, 53), np.uint16)[0][1]
    med = BR.median3(x)
    assert np.array_equal(LR.local_mask(x, 4, 5, 100, median=True), LR.local_mask(med, 4, 5, 100))
    assert not np.array_equal(LR.local_mask(x, 4, 5, 100, median=True), LR.local_mask(x, 4, 5, 100))


def test_golden_equals_scikit_image_on_every_pixel():
    g = np.load(GOLDEN)
    assert "scikit-image 0.18.3" in list(g["versions"])
    radii, deltas = [int(v) for v in g["radii"]], [int(v) for v in g["deltas"]]
    assert radii == [1, 2, 7, 31, 64, 127, 255] and all(d & 1 for d in deltas)
    shapes = set()
    for i in range(int(g["n"])):
        x = g[f"x_{i}"]
        assert (x & 1).all()                                          # odd pixels, odd delta, odd n: no tie can exist
        shapes.add((x.dtype.name,) + x.shape)
        for r in radii:
            sums = LR.window_sum(x, r)
            for d in deltas:
                assert (LR.margin(x, r, d, sums) != 0).all()
                want = np.unpackbits(g[f"m_{r}_{'m' + str(-d) if d < 0 else d}_{i}"])[:x.size].reshape(x.shape)
                assert np.array_equal(LR.local_mask(x, r, d, sums=sums), want), (i, r, d)
    assert {(t,) + s for t in ("uint8", "uint16") for s in ((37, 53), (17, 65), (130, 200), (3, 40))} <= shapes


def test_tie_rule():
    for dtype in (np.uint8, np.uint16):
        for shape in ((1, 1), (9, 14), (40, 3)):
            x = np.full(shape, 77, dtype)
            for r in (1, 6, 255):
                assert not LR.local_mask(x, r, 0).any()               # n * x = S everywhere: a tie is background
                assert LR.local_mask(x, r, -1).all()                  # one count below the mean is enough
                assert not LR.local_mask(x, r, -1, floor=77).any()    # the floor at the image's value empties it again
                assert LR.local_mask(x, r, -1, floor=76).all()
                assert not LR.local_mask(x, r, 1).any()
    top = np.full((20, 20), 65535, np.uint16)                         # n * x = 1.7e10: beyond 32 bits
    assert not LR.local_mask(top, 255, 0).any() and LR.local_mask(top, 255, -1).all()
    assert int(LR.window_sum(top, 255)[0, 0]) == 511 * 511 * 65535


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dim_cells_need_the_local_threshold(seed):
    img, cells = dim_cell_scene(seed)
    bright = [(y, x) for y, x, _, peak in cells if peak > 1000]
    dim = [(y, x) for y, x, _, peak in cells if peak < 1000]
    assert len(bright) == len(dim) == 20
    t = R.otsu(img)
    otsu_mask = R.mask_of(img, t, fill_holes=False)
    local = LR.local_mask(img, SCENE_R, SCENE_DELTA)
    found = lambda m, pts: sum(int(bool(m[y, x])) for y, x in pts)
    assert found(otsu_mask, bright) == len(bright) and found(local, bright) == len(bright)
    assert found(local, dim) > found(otsu_mask, dim), (found(local, dim), found(otsu_mask, dim), t)
    assert found(LR.local_mask(img, SCENE_R, SCENE_DELTA, median=True), dim) > found(otsu_mask, dim)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_local_params_refuses_every_bad_value():
    for kw, exc in ((dict(local_radius=None), ValueError), (dict(local_radius=0), ValueError), (dict(local_radius=256), ValueError),
                    (dict(local_radius=-3), ValueError), (dict(local_radius=True), TypeError), (dict(local_radius=25.0), TypeError),
                    (dict(local_radius="25"), TypeError),
                    (dict(local_radius=25, local_delta=65536), ValueError), (dict(local_radius=25, local_delta=-65536), ValueError),
                    (dict(local_radius=25, local_delta=1.5), TypeError), (dict(local_radius=25, local_delta=True), TypeError),
                    (dict(local_radius=25, local_delta=None), TypeError),
                    (dict(local_radius=25, local_floor=-2), ValueError), (dict(local_radius=25, local_floor=65536), ValueError),
                    (dict(local_radius=25, local_floor=0.0), TypeError), (dict(local_radius=25, local_floor=False), TypeError),
                    (dict(local_radius=25, denoise=1), TypeError), (dict(local_radius=25, denoise=None), TypeError)):
        with pytest.raises(exc):
            S.local_params(**kw)
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, threshold="local", **kw)
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, threshold="local", **kw)
    p = S.local_params(np.int64(25), np.int32(-60), 65535, True)
    assert (p.radius, p.delta, p.floor, p.median) == (25, -60, 65535, 1) and C.sizeof(L.CSLocalParams) == 16
    p = S.local_params(255)
    assert (p.radius, p.delta, p.floor, p.median) == (255, 0, -1, 0)


def test_segmenter_modes_and_refusals_before_a_handle_exists():
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0, threshold="local")                    # no radius
    for kw in (dict(local_radius=25), dict(local_delta=5), dict(local_floor=0), dict(threshold=500, local_radius=25)):
        with pytest.raises(ValueError):
            S.ThresholdSegmenter(0, **kw)                             # local_* with another threshold
        with pytest.raises(ValueError):
            S.threshold_cell_extractor(0, **kw)
    with pytest.raises(ValueError):
        S.segment_params("local")                                     # the global parameters know no such mode
    s = S.ThresholdSegmenter(0, threshold="local", local_radius=25, local_delta=60, local_floor=100, denoise=True, connectivity=2,
                             fill_holes=False)
    assert (s._local.radius, s._local.delta, s._local.floor, s._local.median) == (25, 60, 100, 1) and s._background is None
    assert (s._params.threshold_mode, s._params.threshold, s._params.connectivity, s._params.fill_holes) == (L.THRESH_FIXED, 0, 2, 0)
    assert s.threshold == "local" and (s.local_radius, s.local_delta, s.local_floor) == (25, 60, 100)
    s = S.ThresholdSegmenter(0, threshold="local", local_radius=25, background_radius=51, denoise=True)
    assert (s._background.radius, s._background.median) == (51, 1) and s._local.median == 0       # the median runs once
    s = S.ThresholdSegmenter(0, threshold="local", local_radius=25, background_radius=51)
    assert s._background.median == 0 and s._local.median == 0
    img = np.zeros((1, 16, 16, 3), np.uint16)
    for im, ch, exc in ((img.astype(np.float32), None, TypeError), (img[..., :2].copy(), None, ValueError), (img, 3, ValueError),
                        (img[:, :, :8], None, ValueError), (np.zeros((1, 2, 4097), np.uint8), None, ValueError)):
        with pytest.raises(exc):
            s.local_mask_batch(im, channel=ch)
        with pytest.raises(exc):
            s.segment_batch(im, channel=ch)
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0).local_mask_batch(img)                 # no local threshold: no mask
    assert s._pre is None
    plain = S.ThresholdSegmenter(0)
    assert plain._local is None and plain.local_radius is None and (plain.local_delta, plain.local_floor) == (0, -1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "cs_segment_local") and hasattr(raw, "cs_segment_local_last_timing")
    assert "cs_segment_local" in L.SIGNATURES and "cs_segment_local_last_timing" in L.SIGNATURES


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    img = np.zeros((1, 32, 32, 3), np.uint16)
    out = np.full((1, 32, 32), 7, np.uint8)

    def params(radius=8, delta=0, floor=-1, median=0):
        p = L.CSLocalParams()
        p.radius, p.delta, p.floor, p.median = radius, delta, floor, median
        return C.pointer(p)

    base = dict(p=None, image=img.ctypes.data, pt=1, C=3, ch=2, B=1, H=32, W=32, kind=0, par=params(), out=out.ctypes.data, okind=0)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_local(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"], a["out"],
                                    a["okind"])

    invalid = [dict(par=None), dict(par=params(radius=0)), dict(par=params(radius=256)), dict(par=params(radius=-1)),
               dict(par=params(delta=65536)), dict(par=params(delta=-65536)), dict(par=params(floor=-2)), dict(par=params(floor=65536)),
               dict(par=params(median=2)), dict(par=params(median=-1)), dict(ch=3), dict(ch=-1), dict(C=0), dict(pt=2),
               dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(okind=2), dict(image=None), dict(out=None)]
    for kw in invalid:
        assert call(**kw) == -1, kw                               # CS_ERR_INVALID
    assert call(W=4097) == -6 and call(H=5000) == -6              # CS_ERR_UNSUPPORTED, as its neighbours
    assert b"4096" in lib.cs_last_error()
    assert call(B=65536) == -6
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(par=params(1, -65535, 65535, 1)), dict(par=params(255, 65535, -1, 0)), dict(okind=1)):
        assert call(**kw) == (-4 if no_dev else -1), kw           # no handle: no device here, else a NULL handle
    assert lib.cs_segment_local_last_timing(None, None, None) == -1
    assert (out == 7).all()
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, threshold="local", local_radius=8).local_mask_batch(img)
        assert ei.value.status == -4
