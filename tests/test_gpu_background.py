"""The segmenter's background correction on the device (cs_segment_background through cellscreen.segment) against the CPU
restatement of tests/background_reference.py, which tests/test_background_cpu.py holds to SciPy bit for bit.

Every output is an integer (planes, thresholds, counts, labels), so every comparison is np.array_equal: no tolerances."""
import numpy as np
import pytest

import background_reference as BR
import segment_reference as R
import split_reference as SR
from cellscreen import extract as X
from cellscreen import segment as S
from cellscreen import synth
from test_background_cpu import illumination_image, inputs

pytestmark = pytest.mark.gpu

# csrc/segment.hip's own lengths: where the kernels take another path
BG_ROW_SEG = 1024                                       # pixels of a row per workgroup (bg_rows)
BG_ROW_CHUNK = 8 * 64                                   # BG_E * 64: positions of one doubling chunk of a row
BG_COL_CHUNK = 8 * 16                                   # BG_E * (1024 / 64): rows of one doubling chunk of a column tile
BG_COL_TR_MIN, BG_COL_TR_MAX = 128, 512                 # rows of a column tile: 2r rounded up to 64, within these
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (3, 4096), (4096, 3), (16, 64), (17, 65), (130, 200), (257, 513)]
RADII = [1, 2, 7, 31, 32, 33, 127, 128, 255]
RADII += [15, 16, 63, 64, 65]                           # 2r + 1 passes a power of two (one more doubling step) at r = 2^k;
#                                                         2r passes BG_COL_TR_MIN at 64 | 65: the column tile starts to grow
RADII += [96, 97, 224, 225, 254]                        # the column tile goes 192 -> 256 rows at 96 | 97, and reaches
#                                                         BG_COL_TR_MAX at 224 | 225; 254, 255: 510 halo rows of 512
# with (257, 513) the radii up to 64 run three column tiles of BG_COL_TR_MIN rows, 96 two of 192; (3, 4096) runs four row
# segments of BG_ROW_SEG; a window of 2r + 1 >= 257 spans more than two BG_COL_CHUNKs, one of 511 four of them, and a row
# of BG_ROW_SEG + 2r positions up to three BG_ROW_CHUNKs; 127 | 128 and 255 exceed most of the sides above.
assert BG_COL_TR_MIN // 2 in RADII and BG_COL_TR_MIN // 2 + 1 in RADII and BG_COL_TR_MAX // 2 - 1 in RADII


@pytest.fixture(scope="module")
def segs():
    """ThresholdSegmenter per option set, made on demand, closed at the end."""
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, **kw)
        return made[key]

    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def illum():
    """The three uneven-illumination images as one [3,512,512] uint16 stack, and their painted cells."""
    made = [illumination_image(seed) for seed in range(3)]
    stack = np.stack([m[0] for m in made])
    stack.setflags(write=False)
    return stack, [m[1] for m in made]


# ---- plane parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_plane_equals_the_restatement(segs, dtype, shape):
    named = inputs(shape, dtype)
    stack = np.stack([x for _, x in named])                   # the five inputs as one batch
    meds = [BR.median3(x) for x in stack]
    for r in RADII:
        for denoise in (False, True):
            got = segs(background_radius=r, denoise=denoise).correct_batch(stack)
            assert got.dtype == stack.dtype and got.shape == stack.shape
            for k, (name, x) in enumerate(named):
                want = BR.white_tophat(meds[k] if denoise else x, r)
                assert np.array_equal(got[k], want), (name, r, denoise, int((got[k] != want).sum()))


def test_blocks_show_the_exact_window(segs):
    """A bright block that holds the square survives the opening, so the top-hat removes it; one pixel narrower on either axis
    and the opening removes it, so the top-hat keeps all of it: one pixel more or less in the window on any side would show."""
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        for r in (1, 2, 31, 64, 130):
            w = 2 * r + 1
            stack = np.full((3, 300, 280), top // 7, dtype)
            stack[0, 10:10 + w, 8:8 + w] = top
            stack[1, 10:10 + w - 1, 8:8 + w] = top
            stack[2, 10:10 + w, 8:8 + w - 1] = top
            got = segs(background_radius=r).correct_batch(stack)
            assert not got[0].any(), (dtype, r)
            assert np.array_equal(got[1], stack[1] - top // 7) and np.array_equal(got[2], stack[2] - top // 7), (dtype, r)
            assert np.array_equal(got, BR.correct_batch(stack, r))


# ---- channels, batches, runs ------------------------------------------------------------------------------------------------------
def test_each_channel_is_read_in_place_and_alone(segs):
    rng = np.random.default_rng(3)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        imgs = rng.integers(0, top + 1, (2, 70, 90, 3)).astype(dtype)
        for denoise in (False, True):
            s = segs(background_radius=7, denoise=denoise)
            for ch in range(3):
                got = s.correct_batch(imgs, channel=ch)
                assert np.array_equal(got, BR.correct_batch(imgs, 7, denoise, channel=ch)), (dtype, denoise, ch)
                other = imgs.copy()
                other[..., [c for c in range(3) if c != ch]] = rng.integers(0, top + 1, (2, 70, 90, 2)).astype(dtype)
                assert np.array_equal(s.correct_batch(other, channel=ch), got)
            assert np.array_equal(s.correct_batch(imgs), s.correct_batch(imgs, channel=2))     # the segmentation channel


def test_batch_independence_and_determinism(segs):
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 65536, (3, 150, 131)).astype(np.uint16)
    imgs[1] = 777
    for r, denoise in ((5, True), (70, False)):
        s = segs(background_radius=r, denoise=denoise)
        a, b = s.correct_batch(imgs), s.correct_batch(imgs)
        assert np.array_equal(a, b)
        assert not a[1].any()                                      # a constant image has no foreground over its background
        for k in range(3):
            assert np.array_equal(s.correct_batch(imgs[k:k + 1])[0], a[k]), (r, k)
        t = s.last_timing()
        assert t["background_ms"] > 0.0 and (t["median_ms"] > 0.0) == denoise


# ---- device tensors -------------------------------------------------------------------------------------------------------------
def test_device_tensors_in_and_out(segs, illum):
    import torch
    dev = torch.device("cuda", 0)
    stack, _ = illum
    for imgs in (stack[:2], (stack[:1] >> 4).astype(np.uint8)):
        imgs = imgs.copy()
        t = torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).to(dev)
        s = segs(background_radius=32, denoise=True, connectivity=2)
        plane = s.correct_batch(t)
        assert plane.is_cuda and plane.dtype == t.dtype and tuple(plane.shape) == imgs.shape
        host = s.correct_batch(imgs)
        assert np.array_equal(plane.cpu().numpy().view(imgs.dtype), host)
        # the plane left on the device, segmented as a one-channel image, is the one-call form
        lab1, n1, t1 = s.segment_batch(t)
        lab2, n2, t2 = segs(connectivity=2).segment_batch(plane, channel=0)
        assert lab1.is_cuda and torch.equal(lab1, lab2) and np.array_equal(n1, n2) and np.array_equal(t1, t2)
        lab3, n3, t3 = s.segment_batch(imgs)
        assert np.array_equal(lab1.cpu().numpy(), lab3) and np.array_equal(n1, n3) and np.array_equal(t1, t3)


# ---- segment_batch with the option ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity,fill_holes", [(1, False), (1, True), (2, False), (2, True)])
def test_segment_batch_on_uneven_illumination(segs, illum, connectivity, fill_holes):
    stack, cells = illum
    for r, denoise in ((32, False), (20, True)):
        lab, n, thr = segs(background_radius=r, denoise=denoise, connectivity=connectivity, fill_holes=fill_holes).segment_batch(stack)
        elab, en, ethr = BR.segment_batch(stack, r, denoise, connectivity=connectivity, fill_holes=fill_holes)
        assert np.array_equal(thr, ethr) and np.array_equal(n, en) and np.array_equal(lab, elab)
        assert list(n) == [len(c) for c in cells]
    _, n_plain, _ = segs(connectivity=connectivity, fill_holes=fill_holes).segment_batch(stack)
    assert all(int(a) != len(c) for a, c in zip(n_plain, cells))  # the uncorrected segmenter does not find the cells


@pytest.mark.parametrize("connectivity,fill_holes", [(1, True), (2, False)])
def test_segment_batch_on_a_synthetic_field(segs, connectivity, fill_holes):
    imgs, _ = synth.label_images(61, 2, hw=(256, 256), n_cells=24)
    slope = (np.arange(256, dtype=np.uint32) * 20)[None, None, :]                   # a slope under the cells
    imgs[..., 2] = np.minimum(imgs[..., 2] + slope, 65535).astype(np.uint16)
    s = segs(background_radius=40, connectivity=connectivity, fill_holes=fill_holes)
    lab, n, thr = s.segment_batch(imgs)
    elab, en, ethr = BR.segment_batch(imgs, 40, False, connectivity=connectivity, fill_holes=fill_holes)
    assert np.array_equal(thr, ethr) and np.array_equal(n, en) and np.array_equal(lab, elab) and n.min() >= 5
    t = s.last_timing()
    assert set(t) == {"threshold_ms", "label_ms", "median_ms", "background_ms"} and t["background_ms"] > 0.0 and t["median_ms"] == 0.0


def test_split_touching_behind_the_correction(segs):
    xx = np.mgrid[0:200, 0:300][1]
    img = (200 + 3 * xx + 600 * SR.ten_disks()[0]).astype(np.uint16)      # a slope of 900 under ten disks at +600: three
    #                                                                       touching pairs and a touching triple
    s = segs(background_radius=45, split_touching=True)
    lab, n, thr, dist = s.segment_batch(img[None], return_distance=True)
    elab, en, ethr, edq = SR.split(BR.correct(img, 45))
    assert int(thr[0]) == ethr and int(n[0]) == en and np.array_equal(lab[0], elab) and np.array_equal(dist[0], edq)
    assert en == 10
    assert set(s.last_timing()) == {"threshold_ms", "distance_ms", "seed_ms", "flood_ms", "median_ms", "background_ms"}


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_threshold_cell_extractor_on_uneven_illumination(tmp_path, illum):
    stack, cells = illum
    img, painted = stack[0], cells[0]
    path = str(tmp_path / "plate.npy")
    np.save(path, img)
    H, W = img.shape
    # the painted cells that pass the extraction's rules: a disk of radius 9..14 passes the area and eccentricity rules, its
    # bounding box [y - r, y + r + 1) the border rule of 10 px or not
    passing = sum(1 for y, x, r in painted if y - r >= 10 and x - r >= 10 and y + r + 1 <= H - 10 and x + r + 1 <= W - 10)
    assert passing >= 20
    got, got_stats = S.threshold_cell_extractor(background_radius=32)(path)
    want, want_stats = X.label_cell_extractor(lambda seg: BR.segment(np.ascontiguousarray(seg), 32)[0])(path)
    assert len(got) == len(want) == passing
    assert np.array_equal(np.stack(got).view(np.uint32), np.stack(want).view(np.uint32))
    assert got_stats == want_stats
    plain, _ = S.threshold_cell_extractor()(path)
    assert len(plain) != passing
