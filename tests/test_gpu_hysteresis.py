"""The segmenter's hysteresis threshold on the device (cs_segment_hysteresis through cellscreen.segment) against the CPU
restatement of tests/hysteresis_reference.py, which tests/test_hysteresis_cpu.py holds to SciPy.

Every output is an integer (planes, thresholds, counts, labels), so every comparison is np.array_equal: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import background_reference as BR
import clean_reference as CR
import hysteresis_reference as HR
import local_reference as LR
import segment_reference as R
import smooth_reference as MR
import split_intensity_reference as IR
import split_reference as SR
from cellscreen import _lib as L
from cellscreen import extract as X
from cellscreen import segment as S
from test_hysteresis_cpu import SCENE_LOW, SCENE_STRONG, SCENE_WEAK
from test_local_cpu import SCENE_R, dim_cell_scene

pytestmark = pytest.mark.gpu

# csrc/segment.hip's own lengths: where the kernels take another path
SG_TW, SG_TH = 64, 16                                   # a tile of the union-find that the weak components come from
SG_CHUNK = 1024                                         # pixels per workgroup of hy_levels / hy_mark / hy_keep
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53)]
SHAPES += [(SG_TH - 1, SG_TW - 1), (SG_TH, SG_TW), (SG_TH + 1, SG_TW + 1)]          # one short of, equal to, one past a tile
SHAPES += [(1, SG_CHUNK - 1), (1, SG_CHUNK), (1, SG_CHUNK + 1)]                     # ... a chunk
SHAPES += [(3, 4096), (4096, 3), (257, 513)]
CUTS = {np.uint8: (100, 40), np.uint16: (30000, 257)}   # (strong, weak) fixed thresholds of the painted inputs
SCENE = dict(threshold="local", local_radius=SCENE_R, local_delta=SCENE_STRONG, weak_delta=SCENE_WEAK)


@pytest.fixture(scope="module")
def segs():
    """ThresholdSegmenter per option set, made on demand, all on one handle and one stream: an extractor's."""
    made = {}
    ext = X.CellExtractor(0)

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, extractor=ext, **kw)
        return made[key]

    get.extractor = ext
    yield get
    ext.close()


@pytest.fixture(scope="module")
def scenes():
    """Two speckled fields of bright and dim cells as one [2,512,512] uint16 stack, their painted cells, and the restatement's
    planes under the local rule with deltas 200 / 40."""
    made = [dim_cell_scene(seed) for seed in range(2)]
    stack = np.stack([m[0] for m in made])
    planes = np.stack([HR.hysteresis(HR.levels_local(x, SCENE_R, SCENE_STRONG, SCENE_WEAK), 1) for x in stack])
    stack.setflags(write=False)
    planes.setflags(write=False)
    return stack, [m[1] for m in made], planes


def as_tensor(imgs):
    import torch
    return torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).to(torch.device("cuda", 0))


def painted(segs, levels, dtype, connectivity=1, **kw):
    """The device's plane of a stack of level planes, painted as images of `dtype` and cut at CUTS[dtype]."""
    t, low = CUTS[dtype]
    imgs = np.stack([HR.image_of(lv, dtype, t, low) for lv in levels])
    for img, lv in zip(imgs, levels):
        assert np.array_equal(HR.levels_global(img, t, low), lv)
    return segs(threshold=t, weak_threshold=low, connectivity=connectivity, fill_holes=False, **kw).hysteresis_mask_batch(imgs)


def serpentine(cut=False):
    """Levels of a 130 x 200 image: one weak line through every 64 x 16 tile, rows 8, 24, .. 120 and 129, joined at alternate
    ends, with its only strong pixel at its end in the last tile.  cut: two pixels taken out at every tile border, which leaves
    pieces that stay inside one tile each."""
    H, W = 130, 200
    m = np.zeros((H, W), np.uint8)
    rows = list(range(8, H, SG_TH))[:8] + [H - 1]
    for j, y in enumerate(rows):
        m[y, :] = 1
        if j:
            m[rows[j - 1]:y + 1, (W - 1) if j % 2 else 0] = 1
    if cut:
        m[:, SG_TW::SG_TW] = 0
        m[SG_TH::SG_TH, :] = 0
        m[:, SG_TW - 1::SG_TW] = 0                         # and the pixel before it: no diagonal step across either
        m[SG_TH - 1::SG_TH, :] = 0
    m[H - 1, W - 1] = 2
    return m


# ---- the link step on painted level planes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_planes_equal_the_restatement(segs, shape):
    named = HR.level_inputs(shape)                          # noise at two densities, bridged blobs, one strong pixel at each corner
    levels = [lv for _, lv in named]                        # (corner 0 is the component's root), none, no weak pixel, checkerboard
    for dtype in (np.uint8, np.uint16):
        got = {}
        for c in (1, 2):
            got[c] = painted(segs, levels, dtype, c)
            assert got[c].dtype == np.uint8 and got[c].shape == (len(levels),) + shape
            for i, (name, lv) in enumerate(named):
                want = HR.hysteresis(lv, c)
                assert np.array_equal(got[c][i], want), (name, dtype.__name__, c, int((got[c][i] != want).sum()))
        by_name = {name: i for i, (name, _) in enumerate(named)}
        for c in (1, 2):
            assert not got[c][by_name["weak_only"]].any() and not got[c][by_name["empty"]].any()
            for k in range(4):
                assert got[c][by_name[f"corner{k}"]].all()
        if min(shape) > 1:
            i = by_name["checker"]                          # 4 neighbours: only the strong squares; 8: the whole colour
            assert np.array_equal(got[1][i], (levels[i] == 2).astype(np.uint8)) and np.array_equal(got[2][i], levels[i] > 0)
            assert not np.array_equal(got[1][i], got[2][i])


@pytest.mark.parametrize("connectivity", [1, 2])
def test_one_component_through_every_tile(segs, connectivity):
    whole, cut = serpentine(), serpentine(cut=True)
    got = painted(segs, [whole, cut], np.uint16, connectivity)
    assert np.array_equal(got[0], whole > 0) and int(got[0].sum()) > 9 * 200       # the whole line survives
    assert np.array_equal(got[0], HR.hysteresis(whole, connectivity))
    assert np.array_equal(got[1], HR.hysteresis(cut, connectivity))
    ys, xs = np.nonzero(got[1])                                                    # only the piece with the strong pixel
    assert 0 < len(ys) < SG_TW and ys.min() >= 128 and xs.min() >= 192 and got[1][129, 199] == 1


def test_no_flag_leaks_between_the_images_of_a_batch(segs):
    with_strong = [serpentine(), HR.level_inputs((130, 200))[0][1]]
    for first in with_strong:
        second = np.minimum(first, 1)                       # the same weak plane without a strong pixel
        assert second.any() and (first == 2).any()
        for order in ((first, second), (second, first), (first, second, first, second)):
            got = painted(segs, list(order), np.uint8, 1)
            for b, lv in enumerate(order):
                assert np.array_equal(got[b], HR.hysteresis(lv, 1)), b
                assert got[b].any() == bool((lv == 2).any())


# ---- the global rules -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weak", [0.175, 0.5, 1.0 / 65536, 65535.0 / 65536, SCENE_LOW, 0, 65535])
def test_otsu_thresholds_per_image(segs, scenes, weak):
    stack = scenes[0]
    imgs = np.stack([stack[0], stack[1] // 2 + 100, stack[0] // 3]).astype(np.uint16)
    _, _, thr0 = segs(fill_holes=False).segment_batch(imgs)
    s = segs(weak_threshold=weak, fill_holes=False)
    mask = s.hysteresis_mask_batch(imgs)
    lab, n, thr = s.segment_batch(imgs)
    assert np.array_equal(thr, thr0) and len(set(thr.tolist())) == 3 and thr.dtype == np.int32
    for b in range(3):
        t = R.otsu(imgs[b])
        low = HR.weak_of(t, weak)
        want = HR.hysteresis(HR.levels_global(imgs[b], t, low), 1)
        elab, en = R.label_mask(want > 0, 1)
        assert int(thr[b]) == t and np.array_equal(mask[b], want) and int(n[b]) == en and np.array_equal(lab[b], elab), (b, t, low)
    if weak == SCENE_LOW:
        assert int(n[0]) == 20 and int(mask[0].sum()) == 12952
    if weak == 65535:                                       # cut to t_b on the device: the plain mask
        assert np.array_equal(mask, np.stack([imgs[b] > thr0[b] for b in range(3)]))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_fixed_threshold_with_an_absolute_and_a_relative_weak_threshold(segs, dtype):
    top = int(np.iinfo(dtype).max)
    img = MR.smooth_sigma(np.random.default_rng(11).integers(0, top + 1, (97, 300)).astype(dtype), 2.0)
    imgs = np.ascontiguousarray(np.stack([img, img[::-1], np.zeros_like(img)], axis=-1)[None])    # the plane in channels 0 and 1
    t = int(np.percentile(img, 97))
    for weak in (int(np.percentile(img, 60)), t, 0, 0.9, 0.97):
        for c in (1, 2):
            s = segs(threshold=t, weak_threshold=weak, connectivity=c)
            for ch in (0, 1):
                x = np.ascontiguousarray(imgs[0, :, :, ch])
                want = HR.hysteresis(HR.levels_global(x, t, HR.weak_of(t, weak)), c)
                assert want.any() and np.array_equal(s.hysteresis_mask_batch(imgs, channel=ch)[0], want), (weak, c, ch)
            lab, n, thr = s.segment_batch(imgs, channel=0)
            elab, en, et = HR.segment(np.ascontiguousarray(imgs[0, :, :, 0]), t, weak, c, True)
            assert int(thr[0]) == t == et and int(n[0]) == en and np.array_equal(lab[0], elab)
    lv = HR.levels_global(img, t, int(np.percentile(img, 60)))
    assert (lv == 1).any() and not np.array_equal(HR.hysteresis(lv, 1), lv > 0) and not np.array_equal(HR.hysteresis(lv, 1), lv == 2)


# ---- the local rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 25, 255])
def test_local_rule_equals_the_restatement(segs, radius):
    rng = np.random.default_rng(radius)
    for dtype, deltas in ((np.uint8, ((20, 5), (-2, -10), (3, 3))), (np.uint16, ((3000, 500), (-100, -2000), (65535, -65535)))):
        top = int(np.iinfo(dtype).max)
        for shape in ((1, 1), (37, 53), (17, 65), (130, 200)):                     # all smaller than the window at 255
            smooth = MR.smooth_sigma(rng.integers(0, top + 1, shape).astype(dtype), 1.0)
            stack = np.stack([smooth, rng.integers(0, top + 1, shape).astype(dtype)])
            for delta, weak in deltas:
                for floor, denoise, c in ((-1, False, 1), (top // 2, True, 2)):
                    s = segs(threshold="local", local_radius=radius, local_delta=delta, weak_delta=weak, local_floor=floor,
                             denoise=denoise, connectivity=c, fill_holes=False)
                    got = s.hysteresis_mask_batch(stack)
                    lab, n, thr = s.segment_batch(stack)
                    assert (thr == -1).all()
                    for b in range(2):
                        lv = HR.levels_local(stack[b], radius, delta, weak, floor, denoise)
                        want = HR.hysteresis(lv, c)
                        assert np.array_equal(got[b], want), (dtype.__name__, shape, delta, weak, floor, b)
                        elab, en = R.label_mask(want > 0, c)
                        assert int(n[b]) == en and np.array_equal(lab[b], elab)
    x = MR.smooth_sigma(np.random.default_rng(3).integers(0, 65536, (130, 200)).astype(np.uint16), 1.0)
    lv = HR.levels_local(x, radius, 3000, 500)
    assert set(np.unique(lv)) == {0, 1, 2} and not np.array_equal(HR.hysteresis(lv, 1), lv > 0)


def test_local_tie_is_background_for_both_rules(segs):
    x = np.full((1, 40, 70), 77, np.uint16)
    for r in (1, 6, 255):
        kw = dict(threshold="local", local_radius=r, fill_holes=False)
        assert not segs(local_delta=5, weak_delta=0, **kw).hysteresis_mask_batch(x).any()       # the weak rule ties
        assert not segs(local_delta=0, weak_delta=-1, **kw).hysteresis_mask_batch(x).any()      # all weak, the strong rule ties
        assert segs(local_delta=-1, weak_delta=-1, **kw).hysteresis_mask_batch(x).all()
        assert not segs(local_delta=-1, weak_delta=-2, local_floor=77, **kw).hysteresis_mask_batch(x).any()
    y = np.full((1, 9, 9), 100, np.uint16)
    y[0, 4, 4] = 109
    assert not segs(threshold="local", local_radius=1, local_delta=8, weak_delta=7).hysteresis_mask_batch(y).any()
    assert segs(threshold="local", local_radius=1, local_delta=7, weak_delta=7).hysteresis_mask_batch(y).sum() == 1


# ---- the stages before and after ----------------------------------------------------------------------------------------------------
def test_behind_the_smoothing_and_the_background_correction(segs, scenes):
    stack = scenes[0]
    slope = (np.arange(512, dtype=np.int64) * 4)[None, None, :]
    imgs = np.minimum(stack + slope, 65535).astype(np.uint16)
    s = segs(smooth_sigma=1.5, background_radius=40, weak_threshold=0.3)
    mask = s.hysteresis_mask_batch(imgs)
    lab, n, thr = s.segment_batch(imgs)
    _, _, thr_plain = segs(smooth_sigma=1.5, background_radius=40).segment_batch(imgs)
    assert np.array_equal(thr, thr_plain)
    for b in range(2):
        plane = BR.correct(MR.smooth_sigma(imgs[b], 1.5), 40, False)
        want, t = HR.hysteresis_global(plane, "otsu", 0.3, 1)
        elab, en, _ = LR.label_plane(want, 1, True)
        assert int(thr[b]) == t and np.array_equal(mask[b], want) and int(n[b]) == en and np.array_equal(lab[b], elab), b
    s = segs(background_radius=40, denoise=True, **SCENE)                          # the median runs once, in the correction
    got = s.hysteresis_mask_batch(imgs[:1])
    plane = BR.correct(imgs[0], 40, True)
    assert np.array_equal(got[0], HR.hysteresis(HR.levels_local(plane, SCENE_R, SCENE_STRONG, SCENE_WEAK), 1))


def test_in_front_of_the_hole_filling_and_the_cleanup(segs, scenes):
    stack, cells, planes = scenes
    holes = stack.copy()
    for b in range(2):
        for y, x, _, peak in cells[b][:6]:
            holes[b, y - 2:y + 3, x - 2:x + 3] = 0                                  # a hole in three bright and three dim cells
    for kw in (dict(), dict(min_area=50), dict(open_radius=2, open_connectivity=1, min_area=300, connectivity=2)):
        c = kw.get("connectivity", 1)
        s = segs(**SCENE, **kw)
        lab, n, thr = s.segment_batch(holes)
        plane = s.hysteresis_mask_batch(holes)
        assert (thr == -1).all()
        for b in range(2):
            want = HR.hysteresis(HR.levels_local(holes[b], SCENE_R, SCENE_STRONG, SCENE_WEAK), c)
            filled = R.ndimage.binary_fill_holes(want > 0)
            assert np.array_equal(plane[b], want) and filled.sum() >= want.sum() + 6 * 25      # taken before the hole filling
            m = CR.clean(filled, kw.get("open_radius"), kw.get("open_connectivity", 2), kw.get("min_area"), c) if kw else filled
            if kw:
                assert np.array_equal(s.clean_mask_batch(holes)[b], m)
            elab, en = R.label_mask(m > 0, c)
            assert en > 0 and int(n[b]) == en and np.array_equal(lab[b], elab), (kw, b)
        keys = {"threshold_ms", "label_ms", "hysteresis_level_ms", "hysteresis_link_ms"} | ({"open_ms", "min_area_ms"} if kw else set())
        t = s.last_timing()
        assert set(t) == keys and t["hysteresis_level_ms"] > 0.0 and t["hysteresis_link_ms"] > 0.0
    lab, n, _ = segs(**SCENE).segment_batch(stack)
    for b in range(2):
        assert int(n[b]) == 40 and np.array_equal(lab[b] > 0, R.ndimage.binary_fill_holes(planes[b] > 0))
        assert all(lab[b][y, x] > 0 for y, x, _, _ in cells[b])


def test_split_touching_sees_the_linked_mask(segs):
    disks = SR.ten_disks()[0]
    rng = np.random.default_rng(5)
    levels = np.where(disks, 2, (rng.random(disks.shape) < 0.03).astype(np.uint8)).astype(np.uint8)    # ten disks under weak speckle
    levels[100, :] = np.maximum(levels[100, :], 1)                                 # and a weak thread through the field
    t, low = CUTS[np.uint8]
    img = HR.image_of(levels, np.uint8, t, low)
    s = segs(threshold=t, weak_threshold=low, fill_holes=False, split_touching=True)
    lab, n, thr, dist = s.segment_batch(img[None], return_distance=True)
    plane = HR.hysteresis(levels, 1)
    assert plane.sum() > disks.sum() and plane.sum() < (levels > 0).sum()          # the thread joins, loose speckle goes
    elab, en, edq = SR.split_mask(plane > 0, 1, 3)
    assert int(n[0]) == en and int(thr[0]) == t and np.array_equal(lab[0], elab) and np.array_equal(dist[0], edq)
    assert set(s.last_timing()) == {"threshold_ms", "distance_ms", "seed_ms", "flood_ms", "hysteresis_level_ms", "hysteresis_link_ms"}


def test_split_by_intensity_keeps_its_guide(segs):
    img = IR.scene(60.0)
    for kw, deltas in ((dict(weak_threshold=0.5), None), (dict(threshold="local", local_radius=30, local_delta=400, weak_delta=100), 1)):
        s = segs(split_touching=True, split_by="intensity", smooth_sigma=1.5, **kw)
        lab, n, thr, hq = s.segment_batch(img[None], return_distance=True)
        x = MR.smooth_sigma(img, 1.5)
        if deltas is None:
            plane, t = HR.hysteresis_global(x, "otsu", 0.5, 1)
        else:
            plane, t = HR.hysteresis(HR.levels_local(x, 30, 400, 100), 1), -1
        m = R.ndimage.binary_fill_holes(plane > 0)
        elab, en, ehq = IR.split_intensity(m, x, 1, 16, 0)
        assert int(thr[0]) == t and np.array_equal(hq[0], ehq) and int(n[0]) == en and np.array_equal(lab[0], elab), kw
        assert en > R.label_mask(m, 1)[1]                                           # something was split
        assert not np.array_equal(ehq, IR.heights(m, plane, 1, 0))                  # not the 0 / 1 plane's heights


def test_cell_extractor_end_to_end(tmp_path, scenes):
    stack, cells, planes = scenes
    path = str(tmp_path / "plate.npy")
    np.save(path, stack[0])
    got, got_stats = S.threshold_cell_extractor(**SCENE)(path)                      # the reference's own quality rules
    assert len(got) == len(got_stats) == 40                                         # exactly the painted cells
    want, want_stats = X.label_cell_extractor(lambda seg: HR.segment_local(np.ascontiguousarray(seg), SCENE_R, SCENE_STRONG,
                                                                           SCENE_WEAK)[0])(path)
    assert got_stats == want_stats and np.array_equal(np.stack(got).view(np.uint32), np.stack(want).view(np.uint32))
    assert sum(s["area"] for s in got_stats) == 19190
    strong_only = S.threshold_cell_extractor(threshold="local", local_radius=SCENE_R, local_delta=SCENE_STRONG)(path)[1]
    assert len(strong_only) == 39 and sum(s["area"] for s in strong_only) == 16406  # without the rims a dim cell misses the area rule
    glob, glob_stats = S.threshold_cell_extractor(weak_threshold=SCENE_LOW)(path)
    assert len(glob) == 20


# ---- transport ----------------------------------------------------------------------------------------------------------------
def test_device_tensors_in_and_out_and_two_runs(segs, scenes):
    import torch
    stack, _, planes = scenes
    t = as_tensor(stack.copy())
    for kw in (dict(SCENE), dict(SCENE, connectivity=2, min_area=50), dict(weak_threshold=0.175), dict(threshold=2572, weak_threshold=450)):
        s = segs(**kw)
        mask = s.hysteresis_mask_batch(t)
        assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == stack.shape
        host = s.hysteresis_mask_batch(stack)
        assert host.any() and np.array_equal(mask.cpu().numpy(), host) and torch.equal(s.hysteresis_mask_batch(t), mask)
        out_d, out_h, again = s.segment_batch(t), s.segment_batch(stack), s.segment_batch(t)
        assert out_d[0].is_cuda and np.array_equal(out_d[0].cpu().numpy(), out_h[0]) and torch.equal(out_d[0], again[0])
        assert np.array_equal(out_d[1], out_h[1]) and np.array_equal(out_d[1], again[1])
        assert np.array_equal(out_d[2], out_h[2]) and np.array_equal(out_d[2], again[2])
        if "min_area" not in kw:
            # the plane left on the device, labelled as a one-channel image at the fixed threshold 0, is the one-call form
            lab2, n2, _ = segs(threshold=0, connectivity=kw.get("connectivity", 1)).segment_batch(mask, channel=0)
            assert torch.equal(lab2, out_d[0]) and np.array_equal(n2, out_d[1])
    assert np.array_equal(segs(**SCENE).hysteresis_mask_batch(t).cpu().numpy(), planes)


def test_stage_off_is_the_segmenter_as_it_was(segs, scenes):
    stack = scenes[0]
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, (2, 130, 200, 3)).astype(np.uint8)
    for kw in (dict(), dict(connectivity=2, fill_holes=False), dict(threshold=90)):
        s = segs(**kw)
        assert s._hysteresis is None
        for imgs in (stack, noise):
            lab, n, thr = s.segment_batch(imgs)
            elab, en, ethr = R.segment_batch(imgs, **kw)
            assert np.array_equal(lab, elab) and np.array_equal(n, en) and np.array_equal(thr, ethr)
        assert set(s.last_timing()) == {"threshold_ms", "label_ms"}
        with pytest.raises(ValueError):
            s.hysteresis_mask_batch(stack)
    s = segs(threshold="local", local_radius=SCENE_R, local_delta=60)
    lab, n, thr = s.segment_batch(stack)
    for b in range(2):
        elab, en, _ = LR.segment(stack[b], SCENE_R, 60)
        assert int(n[b]) == en and np.array_equal(lab[b], elab) and int(thr[b]) == -1
    assert set(s.last_timing()) == {"threshold_ms", "label_ms", "local_median_ms", "local_ms"}
    # and the stage with equal numbers is the plain rule
    same = segs(threshold="local", local_radius=SCENE_R, local_delta=60, weak_delta=60).segment_batch(stack)
    assert np.array_equal(same[0], lab) and np.array_equal(same[1], n)
    lab90 = segs(threshold=90).segment_batch(noise)
    same = segs(threshold=90, weak_threshold=90).segment_batch(noise)
    assert np.array_equal(same[0], lab90[0]) and np.array_equal(same[1], lab90[1]) and np.array_equal(same[2], lab90[2])


# ---- one handle through every stage --------------------------------------------------------------------------------------------
# Three configurations on one handle, so that its upload buffer, median plane and host-staging plane are shared between every
# stage, called in turn on inputs that grow, shrink and change element size, channel count and batch: each buffer is reused too
# small, then too large.  The sizes are the smallest that cross a 64 x 16 tile border both ways with widths no multiple of 64.
WALK_SHAPES = [(np.uint16, (2, 48, 80, 3)), (np.uint8, (3, 72, 200)), (np.uint16, (2, 48, 80, 3))]
WALK_CONFIGS = [dict(smooth_sigma=1, denoise=True, background_radius=5),
                dict(threshold="local", local_radius=4, local_delta=3, weak_delta=0, min_area=4, open_radius=1),
                dict(split_touching=True, split_by="intensity", smooth_sigma=1)]
WALK_OFF = [("median_ms",), (), ()]                     # the steps that are off: the median ran in the smoothing, not in the correction


def walk_input(dtype, shape, seed):
    """A few Gaussian blobs (two of them overlapping) on noise, in every channel, from a seed."""
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    B, H, W = shape[:3]
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty(shape, dtype)
    for idx in np.ndindex(B, *shape[3:]):
        f = top * 0.1 + rng.normal(0.0, top * 0.01, (H, W))
        centres = [(int(rng.integers(8, H - 8)), int(rng.integers(8, W - 8))) for _ in range(5)]
        centres.append((centres[0][0], centres[0][1] + 6))
        for cy, cx in centres:
            f += top * 0.5 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.5 ** 2))
        out[(idx[0], Ellipsis) + idx[1:]] = np.clip(f, 0, top).astype(dtype)
    return out


def walk_expected(imgs):
    """[(labels, n_labels, thresholds)] of WALK_CONFIGS from the host restatements, composed as the tests above compose them;
    the third with the heights as a fourth."""
    chan = imgs if imgs.ndim == 3 else imgs[..., 2]
    a, b = [], []
    for raw in chan:
        raw = np.ascontiguousarray(raw)
        a.append(R.segment(BR.correct(MR.smooth_sigma(raw, 1.0, True), 5, False), "otsu", 1, True))
        filled = R.ndimage.binary_fill_holes(HR.hysteresis(HR.levels_local(raw, 4, 3, 0), 1) > 0)
        b.append(R.label_mask(CR.clean(filled, 1, 2, 4, 1) > 0, 1) + (-1,))
    stacked = [(np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32))
               for out in (a, b)]
    return stacked + [IR.segment_batch(imgs, smooth_sigma=1)[:4]]


@pytest.fixture(scope="module")
def walk():
    inputs = [walk_input(dtype, shape, 11 + k) for k, (dtype, shape) in enumerate(WALK_SHAPES[:2])]
    expected = [walk_expected(x) for x in inputs]
    for per_input in expected:
        for want in per_input:
            assert (want[1] >= 2).all()                                           # no case is vacuous
    for x in inputs:
        x.setflags(write=False)
    return inputs + inputs[:1], expected + expected[:1]


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensor"])
def test_one_handle_through_every_stage_growing_and_shrinking(segs, walk, on_device):
    inputs, expected = walk
    for imgs, per_input in zip(inputs, expected):
        x = as_tensor(imgs.copy()) if on_device else imgs
        for kw, off, want in zip(WALK_CONFIGS, WALK_OFF, per_input):
            s = segs(**kw)
            got = s.segment_batch(x, return_distance=len(want) == 4)
            if on_device:
                got = tuple(g.cpu().numpy() if hasattr(g, "is_cuda") else g for g in got)
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (kw, imgs.shape)
            if on_device:
                t = s.last_timing()
                assert all(t[key] == 0.0 for key in off) and t == s.last_timing(), (kw, t)


# ---- the C ABI with a device ------------------------------------------------------------------------------------------------------
def test_error_codes_with_a_handle():
    lib = L.load_library()
    h = C.c_void_p()
    assert lib.cs_preproc_create(0, C.byref(h)) == 0
    try:
        img = np.full((1, 32, 32), 50, np.uint16)
        img[0, 16, 16] = 200
        out = np.full((1, 32, 32), 7, np.uint8)
        thr = np.full(1, 7, np.int32)
        par = L.CSSegmentParams()
        par.threshold_mode, par.threshold, par.connectivity, par.fill_holes = L.THRESH_FIXED, 100, 1, 0
        lp = L.CSLocalParams()
        lp.radius, lp.delta, lp.floor, lp.median = 8, 0, -1, 0

        def hys(mode=L.WEAK_ABSOLUTE, weak=40, r0=0):
            p = L.CSHysteresisParams()
            p.mode, p.weak, p.reserved[0] = mode, weak, r0
            return C.pointer(p)

        def call(hy, local=None, H=32, W=32):
            return lib.cs_segment_hysteresis(h, img.ctypes.data, 1, 1, 0, 1, H, W, 0, C.byref(par), local, hy, out.ctypes.data, 0,
                                             thr.ctypes.data)

        for hy, local in ((None, None), (hys(3), None), (hys(r0=1), None), (hys(L.WEAK_ABSOLUTE, 101), None),
                          (hys(L.WEAK_ABSOLUTE, -1), None), (hys(L.WEAK_FRACTION, 0), None), (hys(L.WEAK_FRACTION, 65536), None),
                          (hys(L.WEAK_LOCAL, 0), None), (hys(L.WEAK_ABSOLUTE, 40), C.pointer(lp)), (hys(L.WEAK_LOCAL, 1), C.pointer(lp))):
            assert call(hy, local) == -1                              # CS_ERR_INVALID
        assert call(hys(), W=4097) == -6 and call(hys(), H=4097) == -6                   # CS_ERR_UNSUPPORTED
        assert (out == 7).all() and (thr == 7).all()                  # nothing ran
        assert call(hys()) == 0 and (out == 1).all() and int(thr[0]) == 100              # and the handle still works
        assert call(hys(L.WEAK_ABSOLUTE, 100)) == 0 and out.sum() == 1 and out[0, 16, 16] == 1
        assert call(hys(L.WEAK_FRACTION, 32768)) == 0 and out.sum() == 1                 # low = 50: the plane's own value ties
        assert call(hys(L.WEAK_FRACTION, 32767)) == 0 and (out == 1).all()               # low = 49
        thr[:] = 7
        assert call(hys(L.WEAK_LOCAL, -1), C.pointer(lp)) == 0 and (out == 1).all() and int(thr[0]) == -1
        assert call(hys(L.WEAK_LOCAL, 0), C.pointer(lp)) == 0 and out.sum() == 1 and out[0, 16, 16] == 1     # the rest ties
        ms = [C.c_double(-1.0) for _ in range(2)]
        assert lib.cs_segment_hysteresis_last_timing(h, *(C.byref(v) for v in ms)) == 0
        assert ms[0].value > 0.0 and ms[1].value > 0.0
    finally:
        lib.cs_preproc_free(h)
