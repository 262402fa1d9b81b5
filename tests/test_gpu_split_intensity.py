"""The segmenter's split_by="intensity" option on the device (cs_segment_split_intensity through cellscreen.segment) against the
CPU restatement of tests/split_intensity_reference.py, which tests/golden/golden_split_intensity.npz records.

Every output is an integer (labels, region counts, thresholds, the heights Hq), so every comparison is np.array_equal: there
are no tolerances."""
import numpy as np
import pytest

import extract_reference as XR
import segment_reference as R
import smooth_reference as MR
import split_intensity_reference as IR
import split_reference as SR
from cellscreen import segment as S
from test_gpu_segment import _spiral

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def segs():
    """Intensity-splitting ThresholdSegmenters per argument set, made on demand, closed at the end."""
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, split_touching=True, split_by="intensity", **kw)
        return made[key]

    yield get
    for s in made.values():
        s.close()


def check(segs, images, channel=None, depth=16, contrast=0, **kw):
    """One device call on a stack against the restatement's batch function, image by image; returns the device's outputs.
    kw: the stage options, spelled as ThresholdSegmenter spells them."""
    lab, n, thr, hq = segs(split_depth=depth, split_contrast=contrast, **kw).segment_batch(images, channel=channel, return_distance=True)
    elab, en, ethr, ehq, _ = IR.segment_batch(images, channel=channel, depth=depth, min_contrast=contrast, **kw)
    assert lab.dtype == np.int32 and lab.shape == elab.shape and hq.dtype == np.uint8 and hq.shape == elab.shape
    assert n.dtype == np.int32 and np.array_equal(thr, ethr), (thr, ethr)
    for b in range(len(elab)):
        assert np.array_equal(hq[b], ehq[b]), ("Hq", b, int((hq[b] != ehq[b]).sum()))
    assert np.array_equal(n, en), (n, en)
    for b in range(len(elab)):
        assert np.array_equal(lab[b], elab[b]), ("labels", b, int((lab[b] != elab[b]).sum()))
    return lab, n, hq


# ---- the scene the option is for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_scene(segs, dtype):
    img = IR.scene(60.0, dtype=dtype)[None]
    counts = {}
    for c in (1, 2):
        for d in (4, 16, 64):
            counts[c, d] = int(check(segs, img, depth=d, connectivity=c, smooth_sigma=1.5)[1][0])
    assert counts[1, 16] == 10 and counts[2, 16] == 10 and counts[1, 64] == 9
    if dtype == np.uint16:
        lab = segs(split_depth=16, split_contrast=0, smooth_sigma=1.5).segment_batch(img)[0][0]
        assert list(np.bincount(lab.ravel())[1:]) == [534, 510, 256, 205, 340, 1123, 531, 480, 407, 334]
        dist = S.ThresholdSegmenter(0, split_touching=True, smooth_sigma=1.5)
        assert dist.segment_batch(img)[1][0] == 5                             # not one neck: the distance split finds nothing
        dist.close()


# ---- shapes the tiling must survive: 64 x 16 tiles, 1024-pixel chunks, partial waves ----------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (17, 65), (33, 130), (16, 64), (130, 200)])
def test_shapes(segs, shape):
    """A random guide under an 80 % random mask, under a full mask and under an empty one.  The mask is image > t with the guide
    drawn above t where the mask is set and at or below it elsewhere."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for dtype, t, top in ((np.uint16, 1000, 65536), (np.uint8, 20, 256)):
        guide = rng.integers(t + 1, top, shape)
        for mask in (rng.random(shape) < 0.8, np.ones(shape, bool), np.zeros(shape, bool)):
            img = np.where(mask, guide, rng.integers(0, t + 1, shape)).astype(dtype)[None]
            for c, d in ((1, 16), (2, 4)):
                _, n, hq = check(segs, img, depth=d, threshold=t, connectivity=c, fill_holes=False)
                if not mask.any():
                    assert n[0] == 0 and not hq.any()
                if mask.all():
                    assert hq.min() >= 1 and (hq.max() == 255 or mask.size == 1)


@pytest.mark.parametrize("connectivity", [1, 2])
def test_one_component_through_many_tiles_and_chunks(segs, connectivity):
    """A one-pixel spiral of 300 x 517 under a ramp: the per-root atomics of one component come from hundreds of workgroups."""
    m = _spiral(300, 517)
    yy, xx = np.mgrid[0:300, 0:517]
    img = np.where(m, 1000 + 37 * yy + 11 * xx, 0).astype(np.uint16)[None]
    assert R.label_mask(m, connectivity)[1] == 1
    _, n, hq = check(segs, img, threshold=0, connectivity=connectivity, fill_holes=False)
    assert n[0] > 1 and hq.max() == 255 and hq[0][m].min() == 1


def test_zero_and_65535_in_one_component(segs):
    """The 32-bit product (G - lo) * 254 at its largest: a ring of 65535 around a filled hole of 0."""
    yy, xx = np.mgrid[0:40, 0:60]
    d = np.sqrt((yy - 20.0) ** 2 + (xx - 30.0) ** 2)
    img = np.clip(65535 - (d - 14) * 3000, 0, 65535)
    img[np.abs(d - 12) <= 2] = 65535
    img[d < 10] = 0
    img = np.rint(img).astype(np.uint16)[None]
    for c in (1, 2):
        _, n, hq = check(segs, img, threshold=100, connectivity=c, fill_holes=True)
        assert hq[0, 20, 30] == 1 and hq[0, 20, 42] == 255 and n[0] >= 1


def test_contrast_floor_and_depth_254_give_the_plain_labels(segs):
    """split_contrast 0 splits the scene; a floor that leaves every component fewer levels than the depth (65535 counts on
    ranges below 2600: 10 levels against a depth of 16) and a depth of 254 both give ThresholdSegmenter's own labels."""
    img = IR.scene(60.0)[None]
    plain = S.ThresholdSegmenter(0, smooth_sigma=1.5)
    pl, pn, pt = plain.segment_batch(img)
    plain.close()
    assert pn[0] == 5
    _, n, _ = check(segs, img, contrast=0, smooth_sigma=1.5)
    assert n[0] == 10
    lab, n, hq = check(segs, img, contrast=65535, smooth_sigma=1.5)
    assert n[0] == 5 and np.array_equal(lab, pl) and hq.max() <= 11
    check(segs, img, contrast=1500, smooth_sigma=1.5)
    for c in (1, 2):
        plain = S.ThresholdSegmenter(0, connectivity=c, smooth_sigma=1.5)
        pl, pn, pt = plain.segment_batch(img)
        plain.close()
        s = segs(split_depth=254, split_contrast=0, connectivity=c, smooth_sigma=1.5)
        lab, n, thr = s.segment_batch(img)
        assert np.array_equal(lab, pl) and np.array_equal(n, pn) and np.array_equal(thr, pt)


def _batch():
    a, b = IR.scene(60.0), IR.scene(150.0, seed=3)
    imgs = np.stack([a[:96, :130], b[60:156, 100:230], np.full((96, 130), 500, np.uint16), a[:96, :130] + np.uint16(2000),
                     np.ascontiguousarray(b[:96, 130:260])])
    return np.ascontiguousarray(imgs)


def test_batch_independence_determinism_and_timing(segs):
    imgs = _batch()                                                           # [2] is constant (empty), [3] all foreground
    for c, d in ((1, 16), (2, 4)):
        lab, n, hq = check(segs, imgs, depth=d, threshold=700, connectivity=c, smooth_sigma=1.5)
        assert n[2] == 0 and (lab[3] > 0).all() and n[0] > 1
        s = segs(split_depth=d, split_contrast=0, threshold=700, connectivity=c, smooth_sigma=1.5)
        lab2, n2, thr2, hq2 = s.segment_batch(imgs, return_distance=True)
        assert np.array_equal(lab, lab2) and np.array_equal(n, n2) and np.array_equal(hq, hq2) and np.all(thr2 == 700)
        for b in range(5):
            l1, n1, _, h1 = s.segment_batch(imgs[b:b + 1], return_distance=True)
            assert np.array_equal(l1[0], lab[b]) and n1[0] == n[b] and np.array_equal(h1[0], hq[b]), (c, d, b)
        t = s.last_timing()
        assert set(t) == {"threshold_ms", "height_ms", "seed_ms", "flood_ms", "smooth_ms"} and min(t.values()) > 0.0
        assert s.last_host_syncs() >= 3                                       # a reconstruction read, a flood read and the final one


def test_device_tensors_in_and_out(segs):
    import torch
    dev = torch.device("cuda", 0)
    for dtype in (np.uint16, np.uint8):
        img = IR.scene(60.0, dtype=dtype)
        imgs = np.ascontiguousarray(np.stack([img, img[::-1]]))
        for kw in (dict(smooth_sigma=1.5), dict(threshold=int(R.otsu(img)), fill_holes=False)):       # a guide plane of its own; image = guide
            s = segs(split_depth=16, split_contrast=0, **kw)
            lab, n, thr, hq = s.segment_batch(imgs, return_distance=True)
            t = torch.from_numpy(imgs.view(np.int16) if dtype == np.uint16 else imgs).to(dev)
            tl, tn, tt, th = s.segment_batch(t, return_distance=True)
            assert tl.is_cuda and tl.dtype == torch.int32 and th.is_cuda and th.dtype == torch.uint8 and tuple(th.shape) == lab.shape
            assert np.array_equal(tl.cpu().numpy(), lab) and np.array_equal(th.cpu().numpy(), hq)
            assert np.array_equal(tn, n) and np.array_equal(tt, thr) and isinstance(tn, np.ndarray)
            out = s.segment_batch(t)
            assert len(out) == 3 and np.array_equal(out[0].cpu().numpy(), lab)
    chan = np.zeros((1,) + IR.SCENE_SHAPE + (3,), np.uint16)                  # the guide read from channel 2 of an interleaved image
    chan[0, ..., 2] = MR.smooth_sigma(IR.scene(60.0), 1.5)
    chan[0, ..., 0] = 60000
    lab, n, _ = check(segs, chan)
    assert n[0] == 10
    check(segs, chan, channel=0)


# ---- plumbing: which plane is the guide ---------------------------------------------------------------------------------------
def test_guide_is_the_smoothed_plane_under_the_local_threshold_and_the_cleanup(segs):
    """smooth_sigma with threshold="local" and min_area: the mask comes from a 0 / 1 plane, the heights from the smoothed plane.
    With the raw channel as the guide the restatement finds other labels (every noise peak a seed), and without min_area too."""
    img = IR.scene(150.0)[None]
    kw = dict(threshold="local", local_radius=30, local_delta=40, smooth_sigma=1.5)
    raw = IR.segment_batch(img, min_area=50, raw_guide=True, **kw)
    assert raw[1][0] > 40 and IR.segment_batch(img, **kw)[1][0] > 40
    lab, n, _ = check(segs, img, min_area=50, **kw)
    assert n[0] == 10 and not np.array_equal(lab, raw[0])
    t = segs(split_depth=16, split_contrast=0, min_area=50, **kw).last_timing()
    assert {"threshold_ms", "height_ms", "seed_ms", "flood_ms", "smooth_ms", "local_ms", "min_area_ms"} <= set(t)


def test_guide_is_the_corrected_plane(segs):
    yy, xx = np.mgrid[0:IR.SCENE_SHAPE[0], 0:IR.SCENE_SHAPE[1]]
    noise = np.random.default_rng(1).normal(0.0, 60.0, IR.SCENE_SHAPE)
    img = np.rint(np.clip(IR.scene(0.0) + 8.0 * xx + 5.0 * yy + noise, 0, 65535)).astype(np.uint16)[None]
    kw = dict(smooth_sigma=1.5, background_radius=30)
    raw = IR.segment_batch(img, raw_guide=True, **kw)
    uncorrected = IR.segment_batch(img, smooth_sigma=1.5)
    lab, n, hq = check(segs, img, **kw)
    assert n[0] == 10 and not np.array_equal(hq, raw[3]) and not np.array_equal(lab, uncorrected[0])
    check(segs, img, background_radius=30, denoise=True)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def scene_file_image(seed=5):
    """[170, 260, 3] uint16: the scene in channel 2, channel 1 textured as test_gpu_split.touching_pairs_image paints its cells."""
    rng = np.random.default_rng(seed)
    H, W = IR.SCENE_SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    ana = rng.uniform(0.02, 0.08, (H, W))
    for cy, cx, r, _ in IR.CELLS:
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= (0.8 * r) ** 2
        ana[m] = rng.uniform(0.3, 0.8) + 0.15 * np.exp(-((yy[m] - cy) ** 2 + (xx[m] - cx) ** 2) / (2 * (0.4 * r) ** 2))
    ana += rng.normal(0.0, 0.02, (H, W))
    img = np.zeros((H, W, 3), np.uint16)
    img[..., 1] = np.round(np.clip(ana, 0, 1) * 65535)
    img[..., 2] = IR.scene(60.0)
    return img


def test_cell_extractor_end_to_end_counts_more_cells(tmp_path):
    img = scene_file_image()
    np.save(tmp_path / "scene.npy", img)
    elab, en, _, _, _ = IR.segment_batch(img[None], smooth_sigma=1.5)
    crops, regs, status = XR.extract(elab[0], img[..., 1])
    assert status == XR.IMAGE_OK and en[0] == 10
    cells, stats = S.threshold_cell_extractor(split_touching=True, split_by="intensity", smooth_sigma=1.5)(str(tmp_path / "scene.npy"))
    assert len(cells) == len(stats) == len(crops) == 10
    assert [s["area"] for s in stats] == [r["area"] for r in regs if r["failed"] == 0]
    dist_cells, _ = S.threshold_cell_extractor(split_touching=True, split_by="distance", smooth_sigma=1.5)(str(tmp_path / "scene.npy"))
    dlab = SR.split(MR.smooth_sigma(np.ascontiguousarray(img[..., 2]), 1.5), "otsu", 1, True, 3)[0]
    assert len(dist_cells) == len(XR.extract(dlab, img[..., 1])[0]) == 5 and len(cells) > len(dist_cells)
