"""The segmenter's Gaussian smoothing on the device (cs_segment_smooth through cellscreen.segment) against the CPU restatement of
tests/smooth_reference.py, which tests/test_smooth_cpu.py holds to the 2-D sum of the definition and to SciPy.

Every output is an integer (planes, counts, labels), so every comparison is np.array_equal: no tolerances."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import background_reference as BR
import clean_reference as CR
import local_reference as LR
import segment_reference as R
import smooth_reference as SM
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import segment as S
from test_smooth_cpu import SCENE_SIGMA, faint_cell_scene, invalid_tables, table_params

pytestmark = pytest.mark.gpu

# csrc/segment.hip's own lengths: where the kernels take another path
SM_ROW_SEG = 768                                        # pixels of a row per workgroup (sm_rows), 2r more in LDS
SM_ROW_STEP = 384                                       # pixels a wave produces at a time: 64 lanes x 6 adjacent outputs
SM_ROW_LINES = 4                                        # rows per workgroup of sm_rows: one per wave
SM_COL_W = 64                                           # columns per workgroup of sm_cols: one per lane
SM_COL_TR = 128                                         # rows per workgroup of sm_cols, 2r more in LDS
SM_COL_STEP = 16                                        # rows the four waves produce at a time: 4 adjacent outputs each
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 200), (200, 3), (37, 53), (64, 64), (65, 257), (129, 1025), (300, 1100)]
SHAPES += [(5, SM_ROW_SEG - 1), (4, SM_ROW_SEG), (3, SM_ROW_SEG + 1)]       # one row segment to the last pixel, and one pixel of a
#                                                         second; 3, 4 and 5 rows: a workgroup short of, full of, past its lines
SHAPES += [(2, SM_ROW_STEP - 1), (2, SM_ROW_STEP + 1)]  # a wave's first step short by one, and one pixel of a second step
SHAPES += [(SM_COL_TR - 1, SM_COL_W + 2), (SM_COL_TR, 20), (SM_COL_STEP + 1, SM_COL_W - 1)]       # a column tile short of and full of
#                                                         its rows (129 rows above: one row of a second), one row of a second step
SIGMAS = [0.25, 1, 2, 4, 15.875]                        # radii 1, 4, 8, 16, 64: 64 exceeds the sides of most shapes above


@pytest.fixture(scope="module")
def segs():
    """ThresholdSegmenter per option set, made on demand, all on one handle and one stream, an extractor's."""
    made = {}
    ext = X.CellExtractor(0)

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, extractor=ext, **kw)
        return made[key]

    yield get
    ext.close()


def as_tensor(imgs):
    import torch
    return torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).to(torch.device("cuda", 0))


def plane_inputs(shape, dtype):
    """noise over the full range, a ramp, saturated, one bright pixel on a dark field"""
    top = int(np.iinfo(dtype).max)
    H, W = shape
    rng = np.random.default_rng(7 + 1000 * H + W)
    ramp = ((np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5) * (top // 256 + 1) % (top + 1)).astype(dtype)
    bright = np.full(shape, top // 5, dtype)
    bright[H // 2, W // 3] = top
    return [("noise", rng.integers(0, top + 1, shape).astype(dtype)), ("ramp", ramp), ("saturated", np.full(shape, top, dtype)),
            ("bright", bright)]


# ---- plane parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_plane_equals_the_restatement(segs, dtype, shape):
    named = plane_inputs(shape, dtype)
    stack = np.stack([x for _, x in named])                   # the four inputs as one batch
    for sigma in SIGMAS:
        got = segs(smooth_sigma=sigma).smooth_batch(stack)
        assert got.dtype == stack.dtype and got.shape == stack.shape
        w = SM.smooth_weights(sigma)
        for k, (name, x) in enumerate(named):
            want = SM.smooth(x, w)
            assert np.array_equal(got[k], want), (name, sigma, int((got[k] != want).sum()))
        assert np.array_equal(got[2], stack[2])                # saturated stays saturated: nothing overflows


def test_median_runs_before_the_gaussian(segs):
    for dtype in (np.uint8, np.uint16):
        stack = np.stack([x for _, x in plane_inputs((70, 90), dtype)])
        got = segs(smooth_sigma=1, denoise=True).smooth_batch(stack)
        for k in range(len(stack)):
            assert np.array_equal(got[k], SM.smooth_sigma(stack[k], 1, median=True)), (dtype, k)
        t = segs(smooth_sigma=1, denoise=True).last_timing()
        assert t["smooth_ms"] > 0.0 and t["smooth_median_ms"] > 0.0


# ---- stacks, batches, input kinds, runs -------------------------------------------------------------------------------------------
def test_each_channel_is_read_in_place_and_alone(segs):
    rng = np.random.default_rng(3)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        imgs = rng.integers(0, top + 1, (3, 70, 90, 3)).astype(dtype)
        s = segs(smooth_sigma=2)
        for ch in (None, 1):
            got = s.smooth_batch(imgs, channel=ch)
            eff = 2 if ch is None else ch                               # the segmentation channel by default
            assert np.array_equal(got, SM.smooth_batch(imgs, 2, channel=eff)), (dtype, ch)
            assert np.array_equal(got, s.smooth_batch(np.ascontiguousarray(imgs[..., eff])))
            other = imgs.copy()
            other[..., [c for c in range(3) if c != eff]] = rng.integers(0, top + 1, (3, 70, 90, 2)).astype(dtype)
            assert np.array_equal(s.smooth_batch(other, channel=ch), got)


def test_batch_independence_determinism_and_device_tensors(segs):
    import torch
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 65536, (3, 150, 131)).astype(np.uint16)
    imgs[1] = 777
    for sigma, denoise in ((1.5, True), (9, False)):
        s = segs(smooth_sigma=sigma, denoise=denoise)
        a, b = s.smooth_batch(imgs), s.smooth_batch(imgs)
        assert np.array_equal(a, b)                                # two calls are bit-identical
        assert (a[1] == 777).all()                                 # a constant image is a fixed point
        for k in range(3):
            assert np.array_equal(s.smooth_batch(imgs[k:k + 1])[0], a[k]), (sigma, k)
        t = as_tensor(imgs.copy())
        plane = s.smooth_batch(t)
        assert plane.is_cuda and plane.dtype == t.dtype and tuple(plane.shape) == imgs.shape
        assert np.array_equal(plane.cpu().numpy().view(np.uint16), a)
        assert torch.equal(plane, s.smooth_batch(t))
        tm = s.last_timing()
        assert tm["smooth_ms"] > 0.0 and ("smooth_median_ms" in tm) == denoise
    u8 = (imgs >> 8).astype(np.uint8)
    plane = segs(smooth_sigma=2).smooth_batch(as_tensor(u8))
    assert plane.dtype == torch.uint8 and np.array_equal(plane.cpu().numpy(), segs(smooth_sigma=2).smooth_batch(u8))


# ---- chains -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def painted():
    """96 x 128 uint16: nine disks of radius 6..9 (a touching pair among them) at +500 on a sloped background of 200..330 with
    noise of 40 counts and a few hot pixels."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:96, 0:128]
    disks = [(16, 18, 7), (16, 50, 6), (20, 90, 9), (48, 24, 8), (48, 39, 7), (50, 76, 6), (52, 110, 8), (80, 30, 9), (78, 84, 7)]
    img = 200.0 + xx + rng.normal(0.0, 40.0, (96, 128))
    for cy, cx, r in disks:
        img += 500.0 * ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
    img[rng.integers(0, 96, 12), rng.integers(0, 128, 12)] = 4000.0
    img = np.clip(np.rint(img), 0, 65535).astype(np.uint16)
    img.setflags(write=False)
    return img


def test_smooth_then_otsu_with_and_without_the_median(segs, painted):
    t = as_tensor(painted[None].copy())
    for denoise in (False, True):
        s = segs(smooth_sigma=1.5, denoise=denoise)
        plane = SM.smooth_sigma(painted, 1.5, median=denoise)          # the median runs first, inside the smoothing
        elab, en, et = R.segment(plane, "otsu", 1, True)
        lab, n, thr = s.segment_batch(painted[None])
        assert int(n[0]) == en and int(thr[0]) == et and np.array_equal(lab[0], elab), denoise
        dlab, dn, dthr = s.segment_batch(t)
        assert dlab.is_cuda and np.array_equal(dlab.cpu().numpy(), lab) and np.array_equal(dn, n) and np.array_equal(dthr, thr)
        tm = s.last_timing()
        assert set(tm) == {"threshold_ms", "label_ms", "smooth_ms"} | ({"smooth_median_ms"} if denoise else set())
        assert tm["smooth_ms"] > 0.0
    assert en >= 8


def test_smooth_then_background_correction(segs, painted):
    for denoise in (False, True):
        s = segs(smooth_sigma=1.5, background_radius=20, denoise=denoise)
        plane = BR.correct(SM.smooth_sigma(painted, 1.5, median=denoise), 20, False)     # the correction gets no second median
        assert np.array_equal(s.correct_batch(painted[None])[0], plane)
        elab, en, et = R.segment(plane, "otsu", 1, True)
        lab, n, thr = s.segment_batch(painted[None])
        assert int(n[0]) == en and int(thr[0]) == et and np.array_equal(lab[0], elab), denoise
        tm = s.last_timing()
        assert tm["median_ms"] == 0.0 and ("smooth_median_ms" in tm) == denoise and tm["background_ms"] > 0.0


def test_smooth_then_local_threshold_cleanup_and_split(segs, painted):
    kw = dict(smooth_sigma=1.5, threshold="local", local_radius=12, local_delta=40, min_area=20, split_touching=True)
    for denoise in (False, True):
        s = segs(denoise=denoise, **kw)
        plane = SM.smooth_sigma(painted, 1.5, median=denoise)
        emask = LR.local_mask(plane, 12, 40)                           # the local rule gets no second median
        assert np.array_equal(s.local_mask_batch(painted[None])[0], emask)
        cleaned = CR.clean(ndimage.binary_fill_holes(emask > 0), None, 2, 20, 1)
        assert np.array_equal(s.clean_mask_batch(painted[None])[0], cleaned)
        elab, en, edq = SR.split_mask(cleaned > 0, 1, 3)
        lab, n, thr, dist = s.segment_batch(painted[None], return_distance=True)
        assert int(thr[0]) == -1 and int(n[0]) == en and np.array_equal(lab[0], elab) and np.array_equal(dist[0], edq), denoise
        assert s.last_timing()["local_median_ms"] == 0.0
    assert en >= 9


def test_faint_cells_come_out_whole(segs):
    made = [faint_cell_scene(seed) for seed in range(2)]
    stack = np.stack([m[0] for m in made])
    lab, n, thr = segs(smooth_sigma=SCENE_SIGMA).segment_batch(stack)
    for k, (img, cells) in enumerate(made):
        elab, en, et = R.segment(SM.smooth_sigma(img, SCENE_SIGMA), "otsu", 1, True)
        assert int(n[k]) == en == 40 and int(thr[k]) == et and np.array_equal(lab[k], elab), k
        assert all(lab[k][y, x] > 0 for y, x, _ in cells)
    _, n_raw, _ = segs().segment_batch(stack)
    assert (n_raw > 1000).all()                                        # shattered without the smoothing
    assert "smooth_ms" not in segs().last_timing() and set(segs().last_timing()) == {"threshold_ms", "label_ms"}


def test_threshold_cell_extractor_smooths_the_segmentation_channel_only(tmp_path):
    img, cells = faint_cell_scene(0)
    path = str(tmp_path / "plate.npy")
    np.save(path, img)
    got, got_stats = S.threshold_cell_extractor(smooth_sigma=SCENE_SIGMA)(path)
    want, want_stats = X.label_cell_extractor(
        lambda seg: R.segment(SM.smooth_sigma(np.ascontiguousarray(seg), SCENE_SIGMA), "otsu", 1, True)[0])(path)
    assert len(got) == len(want) > 30
    assert np.array_equal(np.stack(got).view(np.uint32), np.stack(want).view(np.uint32))      # crops of the raw channel
    assert got_stats == want_stats
    plain, _ = S.threshold_cell_extractor()(path)
    assert len(plain) < 20                                             # most cells are lost without the smoothing


# ---- the C ABI with a device ------------------------------------------------------------------------------------------------------
def test_error_codes_with_a_handle():
    lib = L.load_library()
    h = C.c_void_p()
    assert lib.cs_preproc_create(0, C.byref(h)) == 0
    try:
        img = np.full((1, 32, 32), 300, np.uint16)
        out = np.full((1, 32, 32), 7, np.uint16)

        def call(par, H=32, W=32):
            return lib.cs_segment_smooth(h, img.ctypes.data, 1, 1, 0, 1, H, W, 0, par, out.ctypes.data, 0)

        for k, par in enumerate([None] + invalid_tables()):
            assert call(par) == -1, k                                 # CS_ERR_INVALID
        assert call(table_params(), W=4097) == -6 and call(table_params(), H=4097) == -6        # CS_ERR_UNSUPPORTED
        assert (out == 7).all()                                       # nothing ran
        assert call(table_params()) == 0 and (out == 300).all()       # and the handle still works: a constant image stays
        # any table that keeps the rules is applied exactly, a Gaussian or not
        odd = [2, 0, 32766, 0, 0, 1, 0]
        x = np.random.default_rng(5).integers(0, 65536, (32, 32)).astype(np.uint16)
        img[0] = x
        assert call(table_params(radius=6, weights=odd)) == 0 and np.array_equal(out[0], SM.smooth(x, odd))
        assert call(table_params(radius=64, weights=[65536])) == 0 and np.array_equal(out[0], x)
    finally:
        lib.cs_preproc_free(h)
