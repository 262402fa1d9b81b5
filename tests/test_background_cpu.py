"""CPU tests of the segmenter's background correction (cs_segment_background, ThresholdSegmenter(background_radius=...)):
the restatement of tests/background_reference.py against SciPy bit for bit, the uneven-illumination case that the correction
exists for, and the wrapper's and the C ABI's refusals before any device work."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import background_reference as BR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import segment as S

SHAPES = [(1, 1), (1, 300), (300, 1), (5, 7), (37, 53), (20, 20), (130, 200)]
RADII = [1, 2, 7, 20, 40, 63, 255]                      # 40, 63 and 255 exceed sides of the shapes above


def inputs(shape, dtype, seed=0):
    """(name, image): random over the full range, constant, one bright pixel, one dark pixel, a ramp."""
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(seed + 1000 * shape[0] + shape[1])
    H, W = shape
    bright = np.full(shape, top // 5, dtype)
    bright[H // 2, W // 3] = top
    dark = np.full(shape, top - top // 5, dtype)
    dark[H // 3, W // 2] = 0
    ramp = ((np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5) % (top + 1)).astype(dtype)
    return [("random", rng.integers(0, top + 1, shape).astype(dtype)), ("constant", np.full(shape, top // 3, dtype)),
            ("bright", bright), ("dark", dark), ("ramp", ramp)]


def illumination_image(seed, side=512, n_cells=40):
    """The uneven-illumination case: uint16, a background that rises linearly from 200 to 3000 along x, noise of 0..40, and
    n_cells separated disks of radius 9..14 painted at +600.  Returns (image, [(y, x, radius)])."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(200, 3000, side).astype(np.int64)
    img = np.broadcast_to(ramp, (side, side)) + rng.integers(0, 41, (side, side))
    yy, xx = np.mgrid[0:side, 0:side]
    cells = []
    while len(cells) < n_cells:
        y, x = (int(v) for v in rng.integers(17, side - 17, 2))
        rad = int(rng.integers(9, 15))
        if all((y - cy) ** 2 + (x - cx) ** 2 > (rad + cr + 4) ** 2 for cy, cx, cr in cells):
            cells.append((y, x, rad))
    for y, x, rad in cells:
        img = img + 600 * ((yy - y) ** 2 + (xx - x) ** 2 <= rad * rad)
    return img.astype(np.uint16), cells


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_scipy_bit_for_bit(dtype, shape):
    for name, x in inputs(shape, dtype):
        med = BR.median3(x)
        assert med.dtype == x.dtype and np.array_equal(med, ndimage.median_filter(x, size=3)), name
        for r in RADII:
            w = 2 * r + 1
            assert np.array_equal(BR.window_min(x, r), ndimage.grey_erosion(x, size=(w, w))), (name, r)
            assert np.array_equal(BR.window_max(x, r), ndimage.grey_dilation(x, size=(w, w))), (name, r)
            assert np.array_equal(BR.window_min_direct(x, r), BR.window_min(x, r)), (name, r)
            assert np.array_equal(BR.window_max_direct(x, r), BR.window_max(x, r)), (name, r)
            for denoise in (False, True):
                got = BR.correct(x, r, denoise)
                assert got.dtype == x.dtype
                assert np.array_equal(got, ndimage.white_tophat(med if denoise else x, size=(w, w))), (name, r, denoise)


def test_single_pixels_show_the_window_s_extent():
    x = np.zeros((41, 47), np.uint16)
    x[20, 23] = 9
    for r in (1, 2, 7):
        d = BR.window_max(x, r)
        assert d.sum() == 9 * (2 * r + 1) ** 2 and d[20 - r, 23 - r] == 9 and d[20 + r, 23 + r] == 9 and d[20 - r - 1, 23] == 0
        assert np.array_equal(BR.white_tophat(x, r), x)           # narrower than the square: all of it is kept
    assert not BR.white_tophat(np.full((9, 9), 7, np.uint8), 3).any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_uneven_illumination_needs_the_correction(seed):
    img, cells = illumination_image(seed)
    assert len(cells) == 40
    _, n_plain, t_plain = R.segment(img)
    assert n_plain != len(cells)                                  # one global threshold cuts the field in two
    assert 1000 < t_plain < 2500
    for r in (32, 20):
        for denoise in (False, True):
            lab, n, t = BR.segment(img, r, denoise)
            assert n == len(cells), (r, denoise, n)
            assert t < 600
            assert all(lab[y, x] > 0 for y, x, _ in cells)


def test_wrapper_refuses_bad_arguments_before_a_handle_exists():
    for kw, exc in ((dict(background_radius=0), ValueError), (dict(background_radius=256), ValueError),
                    (dict(background_radius=-3), ValueError), (dict(background_radius=True), TypeError),
                    (dict(background_radius=32.0), TypeError), (dict(background_radius="32"), TypeError),
                    (dict(background_radius=32, denoise=1), TypeError), (dict(denoise=True), ValueError)):
        with pytest.raises(exc):
            S.background_params(**kw)
        with pytest.raises(exc):
            S.ThresholdSegmenter(0, **kw)
        with pytest.raises(exc):
            S.threshold_cell_extractor(0, **kw)
    assert S.background_params() is None and S.background_params(None, False) is None
    p = S.background_params(np.int64(51), True)
    assert (p.radius, p.median) == (51, 1) and C.sizeof(L.CSBackgroundParams) == 8
    s = S.ThresholdSegmenter(0, background_radius=32)
    img = np.zeros((1, 16, 16, 3), np.uint16)
    for im, ch, exc in ((img.astype(np.float32), None, TypeError), (img[..., :2].copy(), None, ValueError), (img, 3, ValueError),
                        (img[:, :, :8], None, ValueError), (np.zeros((1, 2, 4097), np.uint8), None, ValueError)):
        with pytest.raises(exc):
            s.correct_batch(im, channel=ch)
        with pytest.raises(exc):
            s.segment_batch(im, channel=ch)
    with pytest.raises(ValueError):
        S.ThresholdSegmenter(0).correct_batch(img)                # no radius: nothing to correct
    assert s._pre is None
    plain = S.ThresholdSegmenter(0)
    assert plain._background is None and plain.background_radius is None and plain.denoise is False


def test_c_abi_refuses_and_reports_no_device():
    lib = L.load_library()
    img = np.zeros((1, 32, 32, 3), np.uint16)
    out = np.full((1, 32, 32), 7, np.uint16)

    def params(radius=32, median=0):
        p = L.CSBackgroundParams()
        p.radius, p.median = radius, median
        return C.pointer(p)

    base = dict(p=None, image=img.ctypes.data, pt=1, C=3, ch=2, B=1, H=32, W=32, kind=0, par=params(), out=out.ctypes.data, okind=0)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cs_segment_background(a["p"], a["image"], a["pt"], a["C"], a["ch"], a["B"], a["H"], a["W"], a["kind"], a["par"],
                                         a["out"], a["okind"])

    invalid = [dict(par=None), dict(par=params(radius=0)), dict(par=params(radius=256)), dict(par=params(radius=-1)),
               dict(par=params(median=2)), dict(par=params(median=-1)), dict(ch=3), dict(ch=-1), dict(C=0), dict(pt=2),
               dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(okind=2), dict(image=None), dict(out=None)]
    for kw in invalid:
        assert call(**kw) == -1, kw                               # CS_ERR_INVALID
    assert call(W=4097) == -6 and call(H=5000) == -6              # CS_ERR_UNSUPPORTED, as its neighbours
    assert b"4096" in lib.cs_last_error()
    no_dev = lib.cs_device_count() <= 0
    for kw in (dict(), dict(par=params(1, 1)), dict(par=params(255, 0)), dict(okind=1)):
        assert call(**kw) == (-4 if no_dev else -1), kw           # no handle: no device here, else a NULL handle
    assert lib.cs_segment_background_last_timing(None, None, None) == -1
    assert (out == 7).all()
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            S.ThresholdSegmenter(0, background_radius=8).correct_batch(img)
        assert ei.value.status == -4
