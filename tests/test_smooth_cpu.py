"""CPU tests of the segmenter's Gaussian smoothing (cs_segment_smooth, ThresholdSegmenter(smooth_sigma=...)): the restatement
of tests/smooth_reference.py against the 2-D sum taken straight from the definition and against SciPy's float64 gaussian_filter
(tests/golden/golden_smooth.npz), the rules of the weight table, the field of faint cells in noise that the option exists for,
and the wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import segment_reference as R
import smooth_reference as SM
from cellscreen import _lib as L
from cellscreen import segment as S
from test_local_cpu import inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_smooth.npz")
GOLDEN_SIGMAS = [0.25, 1.0, 2.0, 4.0, 8.0, 15.875]


def faint_cell_scene(seed, side=512, n_cells=40, peak=250.0, sigma=100.0):
    """A field of faint cells in noise: uint16, background 300 with Gaussian noise of `sigma` counts, n_cells separated
    flat-topped blobs of radius 9..15 (test_local_cpu.dim_cell_scene's layout rule), every one of peak `peak`: a signal of
    2.5 noise sigmas.  Returns (image, [(y, x, radius)])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    cells = []
    while len(cells) < n_cells:
        y, x = (int(v) for v in rng.integers(25, side - 25, 2))
        rad = int(rng.integers(9, 16))
        if all((y - cy) ** 2 + (x - cx) ** 2 > (rad + cr + 6) ** 2 for cy, cx, cr in cells):
            cells.append((y, x, rad))
    img = 300.0 + rng.normal(0.0, sigma, (side, side))
    for y, x, rad in cells:
        img += peak * np.exp(-((((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (rad / 1.6) ** 2)) ** 2))
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16), cells


SCENE_SIGMA = 2                         # a kernel of radius 8 against blobs of radius 9..15
EXTRACT_MIN_AREA = 200                  # the extraction's own area rule


# ---- the weight table -----------------------------------------------------------------------------------------------------------
def test_table_rules_hold_over_a_sigma_sweep():
    n = 0
    for i in range(int(round((15.875 - 0.25) / 0.005)) + 1):
        sigma = 0.25 + 0.005 * i
        w = S.smooth_weights(sigma)
        assert w == SM.smooth_weights(sigma)                           # the restatement's copy is identical
        r = len(w) - 1
        assert r == int(4.0 * sigma + 0.5) and 1 <= r <= 64, sigma
        assert all(isinstance(v, int) for v in w) and min(w) >= 0 and w[0] >= 1, sigma
        assert w[0] + 2 * sum(w[1:]) == 65536, sigma                   # the full, symmetric kernel sums to 2^16
        assert all(a >= b for a, b in zip(w, w[1:])), sigma            # non-increasing from the centre
        n += 1
    assert n == 3126
    assert len(S.smooth_weights(0.25)) == 2 and len(S.smooth_weights(15.875)) == 65
    assert len(S.smooth_weights(2.0, truncate=3.0)) == 7


def test_smooth_weights_equal_the_golden_tables():
    g = np.load(GOLDEN)
    assert "scipy 1.15.3" in list(g["versions"])
    assert [float(v) for v in g["sigmas"]] == GOLDEN_SIGMAS
    for s, sigma in enumerate(GOLDEN_SIGMAS):
        assert S.smooth_weights(sigma) == [int(v) for v in g[f"w_{s}"]], sigma
        assert min(abs(v - 0.5) for v in SM.remainders(sigma)) > 1e-6      # no tap within the last bits of exp of a half


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_restatement_equals_the_direct_2d_sum(dtype):
    tables = [S.smooth_weights(s) for s in (0.25, 0.6, 1.0, 2.0, 3.3)] + [[65536 - 2 * 11, 0, 5, 6], [2, 0, 32766, 0, 0, 1, 0]]
    for shape in ((1, 1), (1, 7), (7, 1), (5, 7), (9, 4), (12, 13)):       # radii 1..13: most reach or exceed a side
        for name, x in inputs(shape, dtype):
            for w in tables:
                assert np.array_equal(SM.smooth(x, w), SM.smooth_direct(x, w)), (shape, name, w[:3])


def test_derived_bound_against_the_library_on_every_pixel():
    g = np.load(GOLDEN)
    shapes, worst = set(), {}
    for i in range(int(g["n"])):
        x, rows, cols = g[f"x_{i}"], g[f"rows_{i}"], g[f"cols_{i}"]
        top = int(np.iinfo(x.dtype).max)
        shapes.add((x.dtype.name,) + x.shape)
        for s, sigma in enumerate(GOLDEN_SIGMAS):
            w = [int(v) for v in g[f"w_{s}"]]
            f = g[f"f_{s}_{i}"]
            assert f.dtype == np.float64 and f.shape == (len(rows), len(cols))
            y = SM.smooth(x, w)[np.ix_(rows, cols)].astype(np.float64)
            err = float(np.abs(y - f).max())
            worst[(x.dtype.name, sigma)] = max(worst.get((x.dtype.name, sigma), 0.0), err)
            assert err <= SM.bound(w, sigma, top), (i, sigma, err, SM.bound(w, sigma, top))
    assert {(t,) + s for t in ("uint8", "uint16") for s in ((1, 1), (3, 40), (17, 33), (37, 53), (130, 200))} <= shapes
    # the bound is derived, not measured: 0.5 for the rounding and the taps' quantisation against the largest pixel
    assert SM.bound(S.smooth_weights(0.25), 0.25, 255) < 0.51 and SM.bound(S.smooth_weights(15.875), 15.875, 65535) < 86.0
    print({k: round(v, 3) for k, v in sorted(worst.items())})


def test_constant_and_saturated_images_are_fixed_points():
    for dtype in (np.uint8, np.uint16):
        top = int(np.iinfo(dtype).max)
        for shape in ((1, 1), (9, 14), (40, 3)):
            for value in (0, 1, 77, top - 1, top):
                x = np.full(shape, value, dtype)
                for sigma in (0.25, 2.0, 15.875):
                    assert np.array_equal(SM.smooth_sigma(x, sigma), x), (dtype, shape, value, sigma)
                assert np.array_equal(SM.smooth(x, [2, 0, 32766, 0, 0, 1, 0] + [0] * 58), x)


def test_impulse_returns_the_rounded_product_of_two_taps():
    for dtype in (np.uint8, np.uint16):
        top = int(np.iinfo(dtype).max)
        for sigma in (0.25, 1.0, 2.0, 4.0):
            w = S.smooth_weights(sigma)
            r = len(w) - 1
            side = 2 * r + 5                                           # the kernel stays clear of the edges: no fold
            x = np.zeros((side, side), dtype)
            x[r + 2, r + 2] = top
            want = np.zeros((side, side), np.int64)
            for di in range(-r, r + 1):
                for dj in range(-r, r + 1):
                    want[r + 2 + di, r + 2 + dj] = (w[abs(di)] * w[abs(dj)] * top + (1 << 31)) >> 32
            assert np.array_equal(SM.smooth(x, w), want.astype(dtype)), (dtype, sigma)


def test_median_runs_before_the_gaussian():
    import background_reference as BR
    x = inputs((37, 53), np.uint16)[0][1]
    w = S.smooth_weights(1.0)
    assert np.array_equal(SM.smooth(x, w, median=True), SM.smooth(BR.median3(x), w))
    assert not np.array_equal(SM.smooth(x, w, median=True), SM.smooth(x, w))


@pytest.mark.parametrize("seed", [0, 1])
def test_faint_cells_need_the_smoothing(seed):
    img, cells = faint_cell_scene(seed)
    assert len(cells) == 40
    lab, n, _ = R.segment(img, "otsu", 1, True)
    big = int((np.bincount(lab.ravel())[1:] >= EXTRACT_MIN_AREA).sum())
    assert n > 1000 and big < 20, (n, big)                             # shattered: the extraction would keep fewer than half
    lab, n, _ = R.segment(SM.smooth_sigma(img, SCENE_SIGMA), "otsu", 1, True)
    assert n == 40, n                                                  # one component per painted cell
    assert all(lab[y, x] > 0 for y, x, _ in cells)
    assert len({int(lab[y, x]) for y, x, _ in cells}) == 40


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_smooth_params_refuses_every_bad_value():
    for kw, exc in ((dict(smooth_sigma=0), ValueError), (dict(smooth_sigma=0.2499), ValueError), (dict(smooth_sigma=15.876), ValueError),
                    (dict(smooth_sigma=16), ValueError), (dict(smooth_sigma=-2.0), ValueError), (dict(smooth_sigma=float("nan")), ValueError),
                    (dict(smooth_sigma=float("inf")), ValueError), (dict(smooth_sigma=True), TypeError),
                    (dict(smooth_sigma="2"), TypeError), (dict(smooth_sigma=(2,)), TypeError), (dict(smooth_sigma=2j), TypeError),
                    (dict(smooth_sigma=2, denoise=1), TypeError), (dict(smooth_sigma=2, denoise=None), TypeError),
                    (dict(smooth_sigma=None, denoise="yes"), TypeError)):
        with pytest.raises(exc):
            S.smooth_params(**kw)
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, **kw)
    assert S.smooth_params() is None and S.smooth_params(None, False) is None and S.smooth_params(None, True) is None
    assert C.sizeof(L.CSSmoothParams) == 4 * 68
    p = S.smooth_params(np.float32(2.0), True)
    assert (p.radius, p.median, p.reserved) == (8, 1, 0) and list(p.weights) == S.smooth_weights(2.0) + [0] * 56
    p = S.smooth_params(np.int64(3))
    assert (p.radius, p.median) == (12, 0)
    assert S.smooth_params(0.25).radius == 1 and S.smooth_params(15.875).radius == 64


def test_segmenter_modes_and_refusals_before_a_handle_exists():
    s = S.ThresholdSegmenter(0, smooth_sigma=2)
    assert s.smooth_sigma == 2.0 and s._smooth.radius == 8 and s._smooth.median == 0 and s._background is None and s._local is None
    # the median runs once, inside the first stage that exists: with smooth_sigma that is the smoothing
    s = S.ThresholdSegmenter(0, smooth_sigma=2, denoise=True)                     # new ground: no background_radius needed
    assert s._smooth.median == 1 and s._background is None and s.denoise is True
    s = S.ThresholdSegmenter(0, smooth_sigma=2, denoise=True, background_radius=51)
    assert s._smooth.median == 1 and (s._background.radius, s._background.median) == (51, 0)
    s = S.ThresholdSegmenter(0, smooth_sigma=1.5, denoise=True, threshold="local", local_radius=25, background_radius=51)
    assert s._smooth.median == 1 and s._background.median == 0 and s._local.median == 0
    s = S.ThresholdSegmenter(0, smooth_sigma=1.5, denoise=True, threshold="local", local_radius=25)
    assert s._smooth.median == 1 and s._background is None and s._local.median == 0
    # without smooth_sigma every call and every refusal is what it was
    plain = S.ThresholdSegmenter(0)
    assert plain._smooth is None and plain.smooth_sigma is None
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0, denoise=True)                          # "denoise=True needs background_radius"
    with pytest.raises(ValueError):
        S.threshold_cell_extractor(0, denoise=True)
    s = S.ThresholdSegmenter(0, threshold="local", local_radius=25, denoise=True)
    assert s._local.median == 1 and s._smooth is None
    s = S.ThresholdSegmenter(0, background_radius=51, denoise=True)
    assert s._background.median == 1
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0, smooth_sigma=2, local_radius=25)       # local_* still belong to threshold="local"
    img = np.zeros((1, 16, 16, 3), np.uint16)
    s = S.ThresholdSegmenter(0, smooth_sigma=2)
    for im, ch, exc in ((img.astype(np.float32), None, TypeError), (img[..., :2].copy(), None, ValueError), (img, 3, ValueError),
                        (img[:, :, :8], None, ValueError), (np.zeros((1, 2, 4097), np.uint8), None, ValueError)):
        with pytest.raises(exc):
            s.smooth_batch(im, channel=ch)
        with pytest.raises(exc):
            s.segment_batch(im, channel=ch)
    with pytest.raises(ValueError):
        plain.smooth_batch(img)                                        # no sigma: no plane
    assert s._pre is None and plain._pre is None
    S.threshold_cell_extractor(0, smooth_sigma=2, denoise=True)        # accepted; nothing is made before the first image


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "cs_segment_smooth") and hasattr(raw, "cs_segment_smooth_last_timing")
    assert "cs_segment_smooth" in L.SIGNATURES and "cs_segment_smooth_last_timing" in L.SIGNATURES


def table_params(radius=8, median=0, reserved=0, weights=None, **change):
    """cs_smooth_params of sigma = 2's table, with single taps changed: change = {"w3": value}."""
    p = L.CSSmoothParams()
    w = S.smooth_weights(2.0) if weights is None else list(weights)
    for k, v in enumerate(w):
        p.weights[k] = v
    for name, v in change.items():
        p.weights[int(name[1:])] = v
    p.radius, p.median, p.reserved = radius, median, reserved
    return C.pointer(p)


def invalid_tables():
    w = S.smooth_weights(2.0)
    return [table_params(radius=0), table_params(radius=65), table_params(radius=-1), table_params(median=2), table_params(median=-1),
            table_params(reserved=1),
            table_params(w8=-1, w0=w[0] + 2 * (w[8] + 1)),             # a negative weight, the sum kept
            table_params(weights=[0, 32768]),                          # w[0] < 1, the sum kept
            table_params(w9=1, w0=w[0] - 2),                           # a non-zero weight beyond the radius, the sum kept
            table_params(w64=1, w0=w[0] - 2),
            table_params(radius=7),                                    # the same: w[8] lies beyond a radius of 7
            table_params(w0=w[0] + 1), table_params(w0=w[0] - 1), table_params(w1=w[1] + 1),         # a sum other than 65536
            table_params(weights=[0] * 9)]


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    img = np.zeros((1, 32, 32, 3), np.uint16)
    out = np.full((1, 32, 32), 7, np.uint16)
    base = dict(p=None, image=img.ctypes.data, pt=1, C=3, ch=2, B=1, H=32, W=32, kind=0, par=table_params(), out=out.ctypes.data, okind=0)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_smooth(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"], a["out"],
                                     a["okind"])

    invalid = [dict(par=None)] + [dict(par=p) for p in invalid_tables()]
    invalid += [dict(ch=3), dict(ch=-1), dict(C=0), dict(pt=2), dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(okind=2),
                dict(image=None), dict(out=None)]
    for k, kw in enumerate(invalid):
        assert call(**kw) == -1, (k, kw)                          # CS_ERR_INVALID
    assert call(W=4097) == -6 and call(H=5000) == -6              # CS_ERR_UNSUPPORTED, as its neighbours
    assert b"4096" in lib.cs_last_error()
    assert call(B=65536) == -6
    no_dev = lib.cs_device_count() <= 0
    wide = S.smooth_params(15.875, True)
    for kw in (dict(), dict(par=C.pointer(wide)), dict(par=table_params(radius=1, weights=[65534, 1])),
               dict(par=table_params(radius=64, weights=[65536])), dict(okind=1)):
        assert call(**kw) == (-4 if no_dev else -1), kw           # no handle: no device here, else a NULL handle
    assert lib.cs_segment_smooth_last_timing(None, None, None) == -1
    assert (out == 7).all()
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, smooth_sigma=2).smooth_batch(img)
        assert ei.value.status == -4
