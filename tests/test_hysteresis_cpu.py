"""CPU tests of the segmenter's hysteresis threshold (cs_segment_hysteresis, ThresholdSegmenter(weak_threshold=...,
weak_delta=...)): the restatement of tests/hysteresis_reference.py against SciPy in the form of scikit-image's function body
(tests/golden/golden_hysteresis.npz), its degenerate cases, the integer rules of the weak threshold, the field of bright and dim
cells that the option was specified on, and the wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import hysteresis_reference as HR
import local_reference as LR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import segment as S
from test_local_cpu import SCENE_R, dim_cell_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_hysteresis.npz")
SCENE_WEAK, SCENE_STRONG = 40, 200      # local deltas in counts: 1.6 and 8 noise sigmas
MODES = (L.WEAK_ABSOLUTE, L.WEAK_FRACTION, L.WEAK_LOCAL)       # cs_hysteresis_params.mode: this module needs the stage
SCENE_LOW = 450                         # the global rule's weak threshold: 6 noise sigmas above the background of 300


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_golden_file():
    g = np.load(GOLDEN)
    assert "scipy 1.15.3" in list(g["versions"])
    shapes, kept_differs = set(), 0
    for i in range(int(g["n"])):
        shape = tuple(int(v) for v in g[f"shape_{i}"])
        size = shape[0] * shape[1]
        lo = np.unpackbits(g[f"lo_{i}"])[:size].reshape(shape)
        hi = np.unpackbits(g[f"hi_{i}"])[:size].reshape(shape)
        levels = (lo + hi).astype(np.uint8)
        shapes.add(shape)
        got = {}
        for c in (1, 2):
            want = np.unpackbits(g[f"h_{c}_{i}"])[:size].reshape(shape)
            got[c] = HR.hysteresis(levels, c)
            assert np.array_equal(got[c], want), (i, c)
            assert not (got[c] & ~lo).any() and not (hi & ~got[c]).any()       # strong <= result <= weak
        kept_differs += int(not np.array_equal(got[1], got[2]))
    assert {(1, 1), (1, 9), (9, 1), (37, 53), (17, 65), (40, 70), (130, 200)} <= shapes
    assert kept_differs >= 5                                                    # the connectivities are told apart


def test_golden_inputs_are_level_inputs():
    g = np.load(GOLDEN)
    i = 0
    for shape in ((1, 1), (1, 9), (9, 1), (37, 53), (17, 65), (40, 70), (130, 200)):
        for _, lv in HR.level_inputs(shape):
            assert np.array_equal(np.unpackbits(g[f"lo_{i}"])[:lv.size].reshape(shape), lv > 0)
            assert np.array_equal(np.unpackbits(g[f"hi_{i}"])[:lv.size].reshape(shape), lv == 2)
            i += 1
    assert i == int(g["n"])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_low_equal_to_high_is_the_plain_mask(dtype):
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(5)
    x = rng.integers(0, top + 1, (37, 53)).astype(dtype)
    for t in (0, 1, top // 2, top - 1, top):
        for c in (1, 2):
            lv = HR.levels_global(x, t, t)
            assert not (lv == 1).any()
            assert np.array_equal(HR.hysteresis(lv, c), (x > t).astype(np.uint8))
            plane, tt = HR.hysteresis_global(x, t, t, c)                        # weak_threshold = t in counts
            assert tt == t and np.array_equal(plane, (x > t).astype(np.uint8))
    with pytest.raises(ValueError):
        HR.levels_global(x, 5, 6)


def test_weak_delta_equal_to_local_delta_is_local_mask():
    rng = np.random.default_rng(6)
    for dtype in (np.uint8, np.uint16):
        x = rng.integers(0, int(np.iinfo(dtype).max) + 1, (37, 53)).astype(dtype)
        for r, d, floor, med in ((1, 0, -1, False), (4, 5, 100, False), (25, -3, -1, True), (255, 7, 20, False)):
            lv = HR.levels_local(x, r, d, d, floor, med)
            assert not (lv == 1).any()
            want = LR.local_mask(x, r, d, floor, med)
            for c in (1, 2):
                assert np.array_equal(HR.hysteresis(lv, c), want), (r, d, floor, med, c)
    with pytest.raises(ValueError):
        HR.levels_local(x, 4, 5, 6)


def test_tie_rule_holds_for_the_weak_comparison():
    for dtype in (np.uint8, np.uint16):
        for shape in ((1, 1), (9, 14), (40, 3)):
            x = np.full(shape, 77, dtype)                                       # n * x = S everywhere
            for r in (1, 6, 255):
                assert not HR.levels_local(x, r, 5, 0).any()                    # a tie under the weak delta is background
                lv = HR.levels_local(x, r, 0, -1)                               # weak passes by one count, strong ties
                assert (lv == 1).all() and not HR.hysteresis(lv).any()
                assert (HR.levels_local(x, r, -1, -1) == 2).all()
                assert not HR.levels_local(x, r, -1, -2, floor=77).any()        # the floor is common to both rules
                assert (HR.levels_local(x, r, -1, -2, floor=76) == 2).all()
    x = np.full((9, 9), 100, np.uint16)
    x[4, 4] = 109                                                               # r = 1: n = 9, margin 72 at the centre
    assert HR.levels_local(x, 1, 8, 7)[4, 4] == 1                               # 72 - 72 = 0: the strong rule ties, the weak one holds
    assert HR.levels_local(x, 1, 7, 7)[4, 4] == 2 and HR.levels_local(x, 1, 9, 8)[4, 4] == 0


def test_fraction_rule_at_its_edges():
    lo, hi = 1.0 / 65536, 65535.0 / 65536
    for t in (0, 1, 2, 255, 256, 2572, 65534, 65535):
        assert HR.weak_of(t, lo) == (t * 1) >> 16 == 0                          # q = 1
        assert HR.weak_of(t, hi) == (t * 65535) >> 16 == (t - 1 if t else 0)    # q = 65535: one count below, 0 stays 0
        assert HR.weak_of(t, 0.5) == t >> 1
        for w in (0, 1, t, 65535):
            assert HR.weak_of(t, w) == min(w, t)                                # counts: never above the strong threshold
    assert HR.weak_of(65535, 0.25) == 16383 and HR.weak_of(2572, 0.175) == (2572 * 11469) >> 16
    for f, q in ((lo, 1), (hi, 65535), (0.5, 32768), (0.5 / 65536, 1), (1.49 / 65536, 1), (1 - 0.51 / 65536, 65535)):
        p = S.hysteresis_params("otsu", f)
        assert (p.mode, p.weak) == (L.WEAK_FRACTION, q), f
    for f in (0.49 / 65536, 1e-9, 1 - 0.5 / 65536, 1 - 1e-9):                   # q = 0 and q = 65536
        with pytest.raises(ValueError):
            S.hysteresis_params("otsu", f)
        with pytest.raises(ValueError):
            HR.weak_of(100, f)


# ---- the scene the option was specified on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,strong_px,both_px,weak_components",
                         [(0, 16590, 19189, 5358), (1, 18320, 21063, 5291), (2, 16406, 18947, 6366)])
def test_scene_local_rule(seed, strong_px, both_px, weak_components):
    img, cells = dim_cell_scene(seed)
    lv = HR.levels_local(img, SCENE_R, SCENE_STRONG, SCENE_WEAK)
    plane = HR.hysteresis(lv, 1)
    assert R.label_mask(plane > 0, 1)[1] == 40
    assert sum(int(plane[y, x]) for y, x, _, _ in cells) == 40
    strong = LR.local_mask(img, SCENE_R, SCENE_STRONG)
    assert int(strong.sum()) == strong_px and int(plane.sum()) == both_px and both_px > strong_px
    n_weak = R.label_mask(LR.local_mask(img, SCENE_R, SCENE_WEAK) > 0, 1)[1]
    assert n_weak == weak_components and n_weak > 1000


@pytest.mark.parametrize("seed,strong_px,both_px", [(0, 6668, 12952), (1, 8086, 15663), (2, 6973, 13526)])
def test_scene_global_rule(seed, strong_px, both_px):
    img, cells = dim_cell_scene(seed)
    plane, t = HR.hysteresis_global(img, "otsu", SCENE_LOW, 1)
    assert 2572 <= t <= 2575
    assert R.label_mask(plane > 0, 1)[1] == 20
    assert int((img > t).sum()) == strong_px and int(plane.sum()) == both_px
    assert sum(int(plane[y, x]) for y, x, _, peak in cells if peak > 1000) == 20
    lab, n, tt = HR.segment(img, "otsu", SCENE_LOW, 1, fill_holes=False)
    assert (n, tt) == (20, t) and np.array_equal(lab > 0, plane > 0)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_hysteresis_params_refuses_every_bad_value():
    glob = [(dict(weak_threshold=True), TypeError), (dict(weak_threshold=np.bool_(False)), TypeError),
            (dict(weak_threshold="0.5"), TypeError), (dict(weak_threshold=[1]), TypeError),
            (dict(weak_threshold=-1), ValueError), (dict(weak_threshold=65536), ValueError),
            (dict(weak_threshold=float("nan")), ValueError), (dict(weak_threshold=0.0), ValueError),
            (dict(weak_threshold=1.0), ValueError), (dict(weak_threshold=-0.5), ValueError), (dict(weak_threshold=450.0), ValueError),
            (dict(weak_threshold=float("inf")), ValueError), (dict(weak_threshold=1e-9), ValueError),
            (dict(threshold=400, weak_threshold=401), ValueError),                # above the fixed threshold
            (dict(weak_delta=5), ValueError),                                     # weak_delta without "local"
            (dict(threshold=400, weak_delta=5), ValueError),
            (dict(weak_threshold=100, weak_delta=5), ValueError)]
    loc = [(dict(weak_threshold=100), ValueError), (dict(weak_threshold=0.5), ValueError),       # weak_threshold with "local"
           (dict(weak_delta=True), TypeError), (dict(weak_delta=1.0), TypeError), (dict(weak_delta="1"), TypeError),
           (dict(weak_delta=-65536), ValueError), (dict(weak_delta=65536), ValueError),
           (dict(local_delta=40, weak_delta=41), ValueError), (dict(weak_delta=1), ValueError),  # above local_delta (0 by default)
           (dict(local_delta=40, weak_delta=30, weak_threshold=5), ValueError)]
    for kw, exc in glob:
        with pytest.raises(exc):
            S.hysteresis_params(**dict(dict(threshold="otsu"), **kw))
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, **kw)
    for kw, exc in loc:
        with pytest.raises(exc):
            S.hysteresis_params(**dict(dict(threshold="local"), **kw))
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, threshold="local", local_radius=25, **kw)
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, threshold="local", local_radius=25, **kw)
    assert S.hysteresis_params() is None and S.hysteresis_params("local") is None and C.sizeof(L.CSHysteresisParams) == 16
    p = S.hysteresis_params(400, np.int64(400))
    assert (p.mode, p.weak, tuple(p.reserved)) == (L.WEAK_ABSOLUTE, 400, (0, 0))
    p = S.hysteresis_params("otsu", 65535)                                        # Otsu: any count, cut to t_b on the device
    assert (p.mode, p.weak) == (L.WEAK_ABSOLUTE, 65535)
    p = S.hysteresis_params(400, np.float32(0.5))
    assert (p.mode, p.weak) == (L.WEAK_FRACTION, 32768)
    p = S.hysteresis_params("local", None, np.int32(-65535), -65535)
    assert (p.mode, p.weak) == (L.WEAK_LOCAL, -65535)
    p = S.hysteresis_params("local", weak_delta=40, local_delta=200)
    assert (p.mode, p.weak) == (L.WEAK_LOCAL, 40)


def test_segmenter_carries_the_stage_and_refuses_before_a_handle_exists():
    s = S.ThresholdSegmenter(0, threshold="local", local_radius=25, local_delta=200, weak_delta=40, denoise=True, connectivity=2,
                             fill_holes=False)
    assert (s._hysteresis.mode, s._hysteresis.weak) == (L.WEAK_LOCAL, 40) and (s.weak_threshold, s.weak_delta) == (None, 40)
    assert (s._local.radius, s._local.delta, s._local.median) == (25, 200, 1)     # the median runs once, inside this stage
    a = s._after_hysteresis
    assert (a.threshold_mode, a.threshold, a.connectivity, a.fill_holes) == (L.THRESH_FIXED, 0, 2, 0)
    s = S.ThresholdSegmenter(0, weak_threshold=0.25)
    assert (s._hysteresis.mode, s._hysteresis.weak) == (L.WEAK_FRACTION, 16384) and s._local is None
    assert (s._params.threshold_mode, s._after_hysteresis.fill_holes) == (L.THRESH_OTSU, 1)
    img = np.zeros((1, 16, 16, 3), np.uint16)
    for im, ch, exc in ((img.astype(np.float32), None, TypeError), (img[..., :2].copy(), None, ValueError), (img, 3, ValueError),
                        (img[:, :, :8], None, ValueError), (np.zeros((1, 2, 4097), np.uint8), None, ValueError)):
        with pytest.raises(exc):
            s.hysteresis_mask_batch(im, channel=ch)
        with pytest.raises(exc):
            s.segment_batch(im, channel=ch)
    plain = S.ThresholdSegmenter(0)
    assert plain._hysteresis is None and plain.weak_threshold is None and plain.weak_delta is None
    with pytest.raises(ValueError):
        plain.hysteresis_mask_batch(img)                                          # neither option: no stage
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0, threshold="local", local_radius=8).hysteresis_mask_batch(img)
    assert s._pre is None and plain._pre is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "cs_segment_hysteresis") and hasattr(raw, "cs_segment_hysteresis_last_timing")
    assert "cs_segment_hysteresis" in L.SIGNATURES and "cs_segment_hysteresis_last_timing" in L.SIGNATURES
    assert MODES == (0, 1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cellscreen.h")).read()
    assert "CS_WEAK_ABSOLUTE = 0, CS_WEAK_FRACTION = 1, CS_WEAK_LOCAL = 2" in header and "#define CS_ABI_VERSION 2" in header


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    img = np.zeros((1, 32, 32, 3), np.uint16)
    out = np.full((1, 32, 32), 7, np.uint8)
    thr = np.full(1, 7, np.int32)

    def seg(mode=L.THRESH_OTSU, threshold=0, connectivity=1, fill_holes=1):
        p = L.CSSegmentParams()
        p.threshold_mode, p.threshold, p.connectivity, p.fill_holes = mode, threshold, connectivity, fill_holes
        return C.pointer(p)

    def loc(radius=8, delta=0, floor=-1, median=0):
        p = L.CSLocalParams()
        p.radius, p.delta, p.floor, p.median = radius, delta, floor, median
        return C.pointer(p)

    def hys(mode=L.WEAK_FRACTION, weak=32768, r0=0, r1=0):
        p = L.CSHysteresisParams()
        p.mode, p.weak, p.reserved[0], p.reserved[1] = mode, weak, r0, r1
        return C.pointer(p)

    base = dict(p=None, image=img.ctypes.data, pt=1, C=3, ch=2, B=1, H=32, W=32, kind=0, seg=seg(), loc=None, hys=hys(),
                out=out.ctypes.data, okind=0, thr=thr.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_hysteresis(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["seg"],
                                         a["loc"], a["hys"], a["out"], a["okind"], a["thr"])

    invalid = [dict(hys=None), dict(hys=hys(mode=3)), dict(hys=hys(mode=-1)), dict(hys=hys(r0=1)), dict(hys=hys(r1=1)),
               dict(hys=hys(L.WEAK_FRACTION, 0)), dict(hys=hys(L.WEAK_FRACTION, 65536)), dict(hys=hys(L.WEAK_FRACTION, -1)),
               dict(hys=hys(L.WEAK_ABSOLUTE, -1)), dict(hys=hys(L.WEAK_ABSOLUTE, 65536)),
               dict(hys=hys(L.WEAK_ABSOLUTE, 401), seg=seg(L.THRESH_FIXED, 400)),
               dict(hys=hys(L.WEAK_LOCAL, 0)),                                             # no cs_local_params
               dict(loc=loc()), dict(hys=hys(L.WEAK_ABSOLUTE, 5), loc=loc()),              # cs_local_params without CS_WEAK_LOCAL
               dict(hys=hys(L.WEAK_LOCAL, 1), loc=loc()),                                  # above the local delta
               dict(hys=hys(L.WEAK_LOCAL, -65536), loc=loc()), dict(hys=hys(L.WEAK_LOCAL, 65536), loc=loc(delta=65535)),
               dict(hys=hys(L.WEAK_LOCAL, 0), loc=loc(radius=0)), dict(hys=hys(L.WEAK_LOCAL, 0), loc=loc(radius=256)),
               dict(hys=hys(L.WEAK_LOCAL, 0), loc=loc(delta=65536)), dict(hys=hys(L.WEAK_LOCAL, -2), loc=loc(floor=-2)),
               dict(hys=hys(L.WEAK_LOCAL, 0), loc=loc(median=2)),
               dict(seg=seg(mode=2)), dict(seg=seg(L.THRESH_FIXED, 65536)), dict(seg=seg(connectivity=3)), dict(seg=seg(fill_holes=2)),
               dict(ch=3), dict(ch=-1), dict(C=0), dict(pt=2), dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(okind=2),
               dict(image=None), dict(out=None)]
    for kw in invalid:
        assert call(**kw) == -1, kw                               # CS_ERR_INVALID
        assert lib.cs_last_error() != b""
    assert call(W=4097) == -6 and call(H=5000) == -6              # CS_ERR_UNSUPPORTED, as its neighbours
    assert b"4096" in lib.cs_last_error()
    assert call(B=65536) == -6
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(seg=None), dict(thr=None), dict(hys=hys(L.WEAK_FRACTION, 1)), dict(hys=hys(L.WEAK_FRACTION, 65535)),
               dict(hys=hys(L.WEAK_ABSOLUTE, 65535)), dict(hys=hys(L.WEAK_ABSOLUTE, 400), seg=seg(L.THRESH_FIXED, 400)),
               dict(hys=hys(L.WEAK_LOCAL, -65535), loc=loc(255, 65535, 65535, 1)), dict(hys=hys(L.WEAK_LOCAL, 0), loc=loc()),
               dict(okind=1)):
        assert call(**kw) == (-4 if no_dev else -1), kw           # no handle: no device here, else a NULL handle
    assert lib.cs_segment_hysteresis_last_timing(None, None, None) == -1
    assert (out == 7).all() and (thr == 7).all()
    if no_dev:
        for kw in (dict(weak_threshold=0.5), dict(threshold="local", local_radius=8, weak_delta=-3)):
            with pytest.raises(L.CellScreenError) as ei:
                S.ThresholdSegmenter(0, **kw).hysteresis_mask_batch(img)
            assert ei.value.status == -4
