"""The segmenter's local mean threshold on the device (cs_segment_local through cellscreen.segment) against the CPU restatement
of tests/local_reference.py, which tests/test_local_cpu.py holds to windows summed one by one and to scikit-image.

Every output is an integer (planes, counts, labels), so every comparison is np.array_equal: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import background_reference as BR
import local_reference as LR
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import segment as S
from test_local_cpu import SCENE_DELTA, SCENE_R, dim_cell_scene, inputs

pytestmark = pytest.mark.gpu

# csrc/segment.hip's own lengths: where the kernels take another path
LT_ROW_SEG = 1024                                       # pixels of a row per workgroup (lt_rows), 2r more in LDS
LT_ROW_LINES = 4                                        # rows per workgroup of lt_rows: one per wave
LT_COL_W = 64                                           # columns per workgroup of lt_cols: one per lane
LT_COL_TILES = 4                                        # row tiles per workgroup of lt_cols: one per wave
LT_COL_TR_MIN, LT_COL_TR_MAX = 128, 512                 # rows of a column tile: 2r rounded up to 64, within these
LT_COL_U = 8                                            # rows of a tile that lt_cols loads at a time; the rest one by one
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (3, 4096), (4096, 3), (17, 65), (130, 200), (257, 513)]
SHAPES += [(5, LT_ROW_SEG - 1), (4, LT_ROW_SEG), (5, LT_ROW_SEG + 1)]       # one row segment to the last pixel, and one pixel of
#                                                         a second: its 2r halo positions are all but one of its line; 3, 4 and
#                                                         5 rows: a workgroup of lt_rows short of, full of and past its lines
SHAPES += [(16, LT_COL_W), (9, LT_COL_W - 1)]           # with (17, 65): a column workgroup short of, full of and past its lanes
SHAPES += [(LT_COL_TR_MIN - 1, 66), (LT_COL_TR_MIN, 20), (LT_COL_TILES * LT_COL_TR_MIN + 1, 70)]       # a tile short of and full
#                                                         of its rows, and 513 rows: one row of a second workgroup at r <= 64
RADII = [1, 2, 7, 31, 32, 33, 127, 128, 255]
RADII += [63, 64, 65]                                   # 2r passes LT_COL_TR_MIN: the column tile starts to grow
RADII += [96, 97, 224, 225, 254]                        # the tile goes 192 -> 256 rows at 96 | 97 and reaches LT_COL_TR_MAX at
#                                                         224 | 225; 254, 255: 510 halo rows of 512
# tiles of 1, 3, 5, 9 and 17 rows run LT_COL_U's one-by-one loop alone or after whole groups, 16 and 128 rows whole groups only.
# a line of lt_rows holds seg + 2r values in runs of ceil((seg + 2r) / 64) | 1 per lane: 3 values (one lane busy) at (1, 1) with
# r = 1, 1534 in runs of 25 at (3, 4096) with r = 255; (3, 4096) runs four row segments, (4096, 3) eight column workgroups of
# 512 rows at r <= 64 and two at r >= 225; 127 | 128 and 255 exceed most of the sides above, so the fold wraps more than once.
assert LT_COL_TR_MIN // 2 in RADII and LT_COL_TR_MIN // 2 + 1 in RADII and LT_COL_TR_MAX // 2 - 1 in RADII


@pytest.fixture(scope="module")
def segs():
    """ThresholdSegmenter per option set, made on demand.  The hundreds of option sets of this file share one handle and one
    stream, an extractor's, which is closed at the end."""
    made = {}
    ext = X.CellExtractor(0)

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, extractor=ext, **kw)
        return made[key]

    yield get
    ext.close()


def local(segs, r, delta=0, floor=-1, **kw):
    return segs(threshold="local", local_radius=r, local_delta=delta, local_floor=floor, **kw)


@pytest.fixture(scope="module")
def scenes():
    """Two fields of bright and dim cells as one [2,512,512] uint16 stack, and their painted cells."""
    made = [dim_cell_scene(seed) for seed in range(2)]
    stack = np.stack([m[0] for m in made])
    stack.setflags(write=False)
    return stack, [m[1] for m in made]


def as_tensor(imgs):
    import torch
    return torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).to(torch.device("cuda", 0))


# ---- plane parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_plane_equals_the_restatement(segs, dtype, shape):
    named = inputs(shape, dtype)                              # noise, constant, ramp, one bright pixel, saturated
    stack = np.stack([x for _, x in named])                   # the five inputs as one batch
    meds = [BR.median3(x) for x in stack]
    mid = int(np.iinfo(dtype).max) // 2
    for r in RADII:
        n = (2 * r + 1) ** 2
        for denoise in (False, True):
            plane = np.stack(meds if denoise else list(stack)).astype(np.int64)
            margin0 = n * plane - np.stack([LR.window_sum(p, r) for p in plane])         # n * x - S: the reference, computed once
            for delta in (-3, 0, 5):
                for floor in (-1, mid):
                    got = local(segs, r, delta, floor, denoise=denoise).local_mask_batch(stack)
                    assert got.dtype == np.uint8 and got.shape == stack.shape
                    want = ((margin0 > n * delta) & (plane > floor)).astype(np.uint8)
                    for k, (name, _) in enumerate(named):
                        assert np.array_equal(got[k], want[k]), (name, r, denoise, delta, floor, int((got[k] != want[k]).sum()))


def test_saturated_image_needs_64_bits(segs):
    """65535 everywhere under the widest window: n * x = S = 511^2 * 65535 = 1.7e10, a tie that 32 bits would not see as one."""
    x = np.full((2, 60, 80), 65535, np.uint16)
    x[1, 30, 40] = 65534
    assert not local(segs, 255, 0).local_mask_batch(x)[0].any()
    assert local(segs, 255, -1).local_mask_batch(x)[0].all()
    got = local(segs, 255, 0).local_mask_batch(x)[1]
    assert np.array_equal(got, LR.local_mask(x[1], 255, 0)) and got.sum() == got.size - 1     # all above the mean but the one


# ---- input kinds, channels, batches, runs -----------------------------------------------------------------------------------------
def test_each_channel_is_read_in_place_and_alone(segs):
    rng = np.random.default_rng(3)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        imgs = rng.integers(0, top + 1, (2, 70, 90, 3)).astype(dtype)
        for denoise in (False, True):
            s = local(segs, 7, 5, denoise=denoise)
            for ch in (0, 2):
                got = s.local_mask_batch(imgs, channel=ch)
                assert np.array_equal(got, s.local_mask_batch(np.ascontiguousarray(imgs[..., ch]))), (dtype, denoise, ch)
                assert np.array_equal(got, LR.local_mask_batch(imgs, 7, 5, -1, denoise, channel=ch)), (dtype, denoise, ch)
                other = imgs.copy()
                other[..., [c for c in range(3) if c != ch]] = rng.integers(0, top + 1, (2, 70, 90, 2)).astype(dtype)
                assert np.array_equal(s.local_mask_batch(other, channel=ch), got)
            assert np.array_equal(s.local_mask_batch(imgs), s.local_mask_batch(imgs, channel=2))     # the segmentation channel


def test_device_tensors_in_and_out(segs, scenes):
    import torch
    stack, _ = scenes
    for imgs in (stack, (stack[:1] >> 4).astype(np.uint8)):
        imgs = imgs.copy()
        t = as_tensor(imgs)
        s = local(segs, SCENE_R, SCENE_DELTA >> (0 if imgs.dtype == np.uint16 else 4), denoise=True, connectivity=2)
        mask = s.local_mask_batch(t)
        assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == imgs.shape
        host = s.local_mask_batch(imgs)
        assert np.array_equal(mask.cpu().numpy(), host)
        # the mask left on the device, labelled as a one-channel image at the fixed threshold 0, is the one-call form
        lab1, n1, t1 = s.segment_batch(t)
        lab2, n2, _ = segs(threshold=0, connectivity=2).segment_batch(mask, channel=0)
        assert lab1.is_cuda and torch.equal(lab1, lab2) and np.array_equal(n1, n2) and (t1 == -1).all()
        lab3, n3, t3 = s.segment_batch(imgs)
        assert np.array_equal(lab1.cpu().numpy(), lab3) and np.array_equal(n1, n3) and np.array_equal(t1, t3)


def test_batch_independence_and_determinism(segs):
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 65536, (3, 150, 131)).astype(np.uint16)
    imgs[1] = 777
    for r, denoise in ((5, True), (70, False)):
        s = local(segs, r, 0, denoise=denoise)
        a, b = s.local_mask_batch(imgs), s.local_mask_batch(imgs)
        assert np.array_equal(a, b)
        assert not a[1].any()                                      # a constant image is a tie everywhere: background
        for k in range(3):
            assert np.array_equal(s.local_mask_batch(imgs[k:k + 1])[0], a[k]), (r, k)
        t = s.last_timing()
        assert t["local_ms"] > 0.0 and (t["local_median_ms"] > 0.0) == denoise


# ---- segment_batch in local mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity,fill_holes", [(1, False), (1, True), (2, False), (2, True)])
def test_segment_batch_labels_the_restatement_s_mask(segs, scenes, connectivity, fill_holes):
    stack, cells = scenes
    for denoise in (False, True):
        s = local(segs, SCENE_R, SCENE_DELTA, denoise=denoise, connectivity=connectivity, fill_holes=fill_holes)
        lab, n, thr = s.segment_batch(stack)
        assert (thr == -1).all() and thr.dtype == np.int32
        for k in range(len(stack)):
            elab, en, _ = LR.segment(stack[k], SCENE_R, SCENE_DELTA, -1, denoise, connectivity, fill_holes)
            assert int(n[k]) == en and np.array_equal(lab[k], elab), (denoise, k)
            assert all(lab[k][y, x] > 0 for y, x, _, _ in cells[k])           # bright and dim cells alike
    t = s.last_timing()
    assert set(t) == {"threshold_ms", "label_ms", "local_median_ms", "local_ms"} and t["local_ms"] > 0.0 and t["local_median_ms"] > 0.0
    _, n_otsu, _ = segs(connectivity=connectivity, fill_holes=fill_holes).segment_batch(stack)
    assert all(int(a) < len(c) for a, c in zip(n_otsu, cells))    # Otsu's one number misses dim cells


def test_split_touching_behind_the_local_mask(segs):
    xx = np.mgrid[0:200, 0:300][1]
    img = (200 + 600 * SR.ten_disks()[0] * (1 + 4 * (xx < 150))).astype(np.uint16)      # ten disks, three touching pairs and a
    #                                                                 touching triple: at +3000 on the left, +600 on the right
    s = local(segs, 45, 100, split_touching=True)
    lab, n, thr, dist = s.segment_batch(img[None], return_distance=True)
    mask = LR.local_mask(img, 45, 100)
    elab, en, _, edq = SR.split(mask, 0)
    assert int(thr[0]) == -1 and int(n[0]) == en and np.array_equal(lab[0], elab) and np.array_equal(dist[0], edq)
    assert en == 10
    assert set(s.last_timing()) == {"threshold_ms", "distance_ms", "seed_ms", "flood_ms", "local_median_ms", "local_ms"}


def test_local_mask_behind_the_background_correction(segs, scenes):
    stack, cells = scenes
    slope = (np.arange(512, dtype=np.int64) * 4)[None, None, :]                       # 2000 counts of slope under the cells
    imgs = np.minimum(stack + slope, 65535).astype(np.uint16)
    for denoise in (False, True):
        s = local(segs, SCENE_R, SCENE_DELTA, background_radius=40, denoise=denoise)
        mask = s.local_mask_batch(imgs)
        lab, n, thr = s.segment_batch(imgs)
        assert (thr == -1).all()
        for k in range(len(imgs)):
            plane = BR.correct(imgs[k], 40, denoise)                                  # the median runs once, inside the correction
            emask = LR.local_mask(plane, SCENE_R, SCENE_DELTA)
            elab, en, _ = LR.label_plane(emask)
            assert np.array_equal(mask[k], emask) and int(n[k]) == en and np.array_equal(lab[k], elab), (denoise, k)
        assert set(s.last_timing()) == {"threshold_ms", "label_ms", "median_ms", "background_ms", "local_median_ms", "local_ms"}
        assert s.last_timing()["local_median_ms"] == 0.0 and (s.last_timing()["median_ms"] > 0.0) == denoise
    # the plane left on the device by the correction is a valid input of the local rule
    t = as_tensor(imgs)
    plane = segs(background_radius=40).correct_batch(t)
    assert np.array_equal(local(segs, SCENE_R, SCENE_DELTA).local_mask_batch(plane).cpu().numpy(),
                          local(segs, SCENE_R, SCENE_DELTA, background_radius=40).local_mask_batch(imgs))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_threshold_cell_extractor_returns_the_dim_cells_too(tmp_path, scenes):
    stack, cells = scenes
    img, painted = stack[0], cells[0]
    path = str(tmp_path / "plate.npy")
    np.save(path, img)
    kw = dict(threshold="local", local_radius=SCENE_R, local_delta=SCENE_DELTA, denoise=True)
    got, got_stats = S.threshold_cell_extractor(**kw)(path)
    want, want_stats = X.label_cell_extractor(
        lambda seg: LR.segment(np.ascontiguousarray(seg), SCENE_R, SCENE_DELTA, -1, True)[0])(path)
    assert len(got) == len(want)
    assert np.array_equal(np.stack(got).view(np.uint32), np.stack(want).view(np.uint32))
    assert got_stats == want_stats
    plain, _ = S.threshold_cell_extractor()(path)
    n_bright = sum(1 for c in painted if c[3] > 1000)
    assert len(plain) <= n_bright < len(got) <= len(painted)       # Otsu returns bright cells only; the local rule dim ones too


# ---- the C ABI with a device ------------------------------------------------------------------------------------------------------
def test_error_codes_with_a_handle():
    lib = L.load_library()
    h = C.c_void_p()
    assert lib.cs_preproc_create(0, C.byref(h)) == 0
    try:
        img = np.zeros((1, 32, 32), np.uint16)
        out = np.full((1, 32, 32), 7, np.uint8)

        def params(radius=8, delta=0, floor=-1, median=0):
            p = L.CSLocalParams()
            p.radius, p.delta, p.floor, p.median = radius, delta, floor, median
            return C.pointer(p)

        def call(par, H=32, W=32):
            return lib.cs_segment_local(h, img.ctypes.data, 1, 1, 0, 1, H, W, 0, par, out.ctypes.data, 0)

        for par in (None, params(radius=0), params(radius=256), params(delta=65536), params(delta=-65536), params(floor=-2),
                    params(floor=65536), params(median=2)):
            assert call(par) == -1                                    # CS_ERR_INVALID
        assert call(params(), W=4097) == -6 and call(params(), H=4097) == -6              # CS_ERR_UNSUPPORTED
        assert (out == 7).all()                                       # nothing ran
        assert call(params(delta=-1)) == 0 and (out == 1).all()       # and the handle still works: zeros, one count below
        assert call(params(delta=0)) == 0 and (out == 0).all()
    finally:
        lib.cs_preproc_free(h)
