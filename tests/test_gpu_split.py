"""The segmenter's split_touching option on the device (cs_segment_split through cellscreen.segment) against the CPU
restatement of tests/split_reference.py, which tests/golden/golden_split.npz pins to SciPy and scikit-image 0.18.3.

Every output is an integer (labels, region counts, the quantised distance Dq), so every comparison is np.array_equal: there
are no tolerances."""
import numpy as np
import pytest

import extract_reference as XR
import segment_reference as R
import split_reference as SR
from cellscreen import segment as S
from cellscreen import synth
from test_gpu_segment import _comb, _rings, _spiral

pytestmark = pytest.mark.gpu

OPTIONS = [(c, h) for c in (1, 2) for h in (1, 3, 8)]


@pytest.fixture(scope="module")
def segs():
    """Splitting ThresholdSegmenters per (threshold, connectivity, fill_holes, h), made on demand, closed at the end."""
    made = {}

    def get(threshold=0, connectivity=1, fill_holes=False, h=3):
        key = (threshold, connectivity, fill_holes, h)
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, threshold, connectivity, fill_holes, split_touching=True, split_h=h)
        return made[key]

    yield get
    for s in made.values():
        s.close()


def check(segs, images, channel=None, threshold=0, connectivity=1, fill_holes=False, h=3):
    """One device call on a stack against the restatement, image by image; returns the device's outputs."""
    lab, n, thr, dq = segs(threshold, connectivity, fill_holes, h).segment_batch(images, channel=channel, return_distance=True)
    elab, en, ethr, edq = SR.split_batch(images, channel=channel, threshold=threshold, connectivity=connectivity, fill_holes=fill_holes,
                                         h=h)
    assert lab.dtype == np.int32 and lab.shape == elab.shape and dq.dtype == np.uint8 and dq.shape == elab.shape
    assert n.dtype == np.int32 and np.array_equal(thr, ethr)
    for b in range(len(elab)):
        assert np.array_equal(dq[b], edq[b]), ("Dq", b, int((dq[b] != edq[b]).sum()))
    assert np.array_equal(n, en), (n, en)
    for b in range(len(elab)):
        assert np.array_equal(lab[b], elab[b]), ("labels", b, int((lab[b] != elab[b]).sum()))
    return lab, n, dq


def check_mask(segs, mask, options=OPTIONS):
    """A boolean mask as a uint8 image under the fixed threshold 0, for both connectivities and every h."""
    img = np.ascontiguousarray(mask, np.uint8)[None]
    return {(c, h): int(check(segs, img, connectivity=c, h=h)[1][0]) for c, h in options}


def disk_field(seed, H, W, n, rmin, rmax):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(rmin, rmax)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m


# ---- the scenes the option is for ------------------------------------------------------------------------------------------
def test_ten_disk_scene(segs):
    mask, _ = SR.ten_disks()
    counts = check_mask(segs, mask)
    assert counts[1, 3] == 10 and counts[1, 1] >= 11 and counts[1, 8] < 10
    lab = segs(0, 1, False, 3).segment_batch(np.ascontiguousarray(mask, np.uint8)[None])[0][0]
    assert list(np.bincount(lab.ravel())[1:]) == [1226, 1226, 148, 112, 1961, 2833, 628, 573, 792, 294]


@pytest.mark.parametrize("seed,shape,n,radii", [(1, (300, 417), 60, (3, 22)), (2, (512, 512), 120, (6, 26)), (3, (200, 1000), 150, (2, 9)),
                                                (4, (700, 600), 25, (20, 70))])
def test_random_disk_fields(segs, seed, shape, n, radii):
    counts = check_mask(segs, disk_field(seed, *shape, n, *radii))
    base = R.label_mask(disk_field(seed, *shape, n, *radii), 1)[1]
    assert counts[1, 1] >= counts[1, 3] >= counts[1, 8] >= base and counts[1, 3] > base


def test_golden_masks(segs):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_split.npz"))
    for i in range(int(g["n"])):
        m = g[f"mask_{i}"]
        for c, h in OPTIONS:
            lab, n, dq = check(segs, np.ascontiguousarray(m, np.uint8)[None], connectivity=c, h=h)
            assert np.array_equal(lab[0], g[f"lab_{c}_{h}_{i}"]) and np.array_equal(dq[0], g[f"dq_{i}"])


# ---- shapes and patterns the tiling must survive -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (37, 53), (4096, 3), (3, 4096), (16, 64), (17, 65), (130, 200)])
def test_small_and_thin_shapes(segs, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for m in (rng.random(shape) < 0.8, np.ones(shape, bool), np.zeros(shape, bool)):
        counts = check_mask(segs, m)
        if m.all():
            assert set(counts.values()) == {1}
        if not m.any():
            assert set(counts.values()) == {0}


def test_all_foreground_and_all_background_images(segs):
    for shape in ((200, 333), (64, 128)):
        for c, h in OPTIONS:
            lab, n, dq = check(segs, np.ones((1,) + shape, np.uint8), connectivity=c, h=h)
            assert n[0] == 1 and (lab == 1).all() and (dq == 255).all()
            lab, n, dq = check(segs, np.zeros((1,) + shape, np.uint8), connectivity=c, h=h)
            assert n[0] == 0 and not lab.any() and not dq.any()


def test_checkerboard(segs):
    yy, xx = np.mgrid[0:150, 0:203]
    m = (yy + xx) % 2 == 0
    counts = check_mask(segs, m)
    assert counts[1, 3] == int(m.sum()) and counts[2, 3] == 1


@pytest.mark.parametrize("make,shape", [(_spiral, (300, 517)), (_spiral, (1025, 1100)), (_comb, (301, 700)), (_rings, (256, 256)),
                                        (_rings, (700, 531))])
def test_long_winding_components_and_nested_rings(segs, make, shape):
    m = make(*shape)
    check_mask(segs, m, options=[(1, 3), (2, 1), (2, 8)])
    check_mask(segs, ~m, options=[(1, 3), (2, 1)])


def test_thick_winding_component(segs):
    """A 9-pixel-wide serpentine: one ridge plateau more than 2000 pixels long that the reconstruction and the flood must
    follow through dozens of tiles."""
    m = np.zeros((200, 330), bool)
    for k, r in enumerate(range(4, 190, 14)):
        m[r:r + 9, 4:326] = True
        m[r + 9:r + 14, (317 if k % 2 == 0 else 4):(326 if k % 2 == 0 else 13)] = True
    counts = check_mask(segs, m, options=[(1, 3), (2, 3), (1, 1)])
    assert R.label_mask(m, 1)[1] == 1 and counts[1, 3] >= 1


@pytest.mark.parametrize("density", [0.5, 0.593, 0.8])
@pytest.mark.parametrize("shape", [(512, 512), (600, 711)])
def test_random_noise_near_the_percolation_threshold(segs, density, shape):
    rng = np.random.default_rng(int(density * 1000) + shape[0])
    check_mask(segs, rng.random(shape) < density, options=[(1, 3), (2, 3), (1, 1), (2, 8)])


def test_blobs_straddling_tile_borders(segs):
    """Touching pairs whose necks and centres sit on the corners and edges of the 64 x 16 tiles."""
    yy, xx = np.mgrid[0:160, 0:400]
    m = np.zeros((160, 400), bool)
    for cy, cx, r, dy, dx in ((32, 64, 11, 0, 19), (64, 192, 12, 21, 0), (96, 320, 10, 13, 13), (127.5, 127.5, 9, 0, 16), (48, 300, 14, 3, 24)):
        for s in (-0.5, 0.5):
            m |= (yy - cy - s * dy) ** 2 + (xx - cx - s * dx) ** 2 <= r * r
    counts = check_mask(segs, m)
    assert counts[1, 3] == 10 and R.label_mask(m, 1)[1] == 5


def test_blob_deeper_than_127_pixels(segs):
    """A 330-pixel disk touching a 40-pixel one: the big core is one plateau of Dq = 255 (one seed), the small one splits
    off; two cores deeper than 127 px joined by a wide bridge stay one region."""
    yy, xx = np.mgrid[0:420, 0:480]
    m = ((yy - 200) ** 2 + (xx - 190) ** 2 <= 165 ** 2) | ((yy - 200) ** 2 + (xx - 390) ** 2 <= 40 ** 2)
    counts = check_mask(segs, m, options=[(1, 3), (2, 3)])
    assert counts[1, 3] == 2
    yy, xx = np.mgrid[0:300, 0:620]
    m = ((yy - 150) ** 2 + (xx - 150) ** 2 <= 140 ** 2) | ((yy - 150) ** 2 + (xx - 470) ** 2 <= 140 ** 2)
    m[20:280, 150:470] = True
    lab, n, dq = check(segs, np.ascontiguousarray(m, np.uint8)[None])
    assert dq.max() == 255 and n[0] == 1


# ---- options, dtypes, batches, runs, device tensors --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("channels", [1, 3])
def test_synthetic_images_with_otsu_and_hole_filling(segs, dtype, channels):
    imgs, _ = synth.label_images(61 + channels, 3, hw=(256, 256), n_cells=40, dtype=dtype, channels=channels)
    if channels == 1:
        imgs = np.ascontiguousarray(synth.label_images(61, 3, hw=(256, 256), n_cells=40, dtype=dtype)[0][..., 2])
    for c in (1, 2):
        for f in (False, True):
            _, n, _ = check(segs, imgs, threshold="otsu", connectivity=c, fill_holes=f, h=3)
            plain = R.segment_batch(imgs, connectivity=c, fill_holes=f)[1]
            assert np.all(n >= plain) and n.sum() > plain.sum()
    if channels == 3:
        check(segs, imgs, channel=1, threshold="otsu", h=8)


def test_batch_independence_and_determinism(segs):
    imgs, _ = synth.label_images(52, 5, n_cells=40)
    rng = np.random.default_rng(52)
    imgs[3, ..., 2] = np.where(rng.random((256, 256)) < 0.7, 40000, 100)
    imgs[4, ..., 2] = 777                                                          # one constant image
    for c, h in ((1, 3), (2, 1)):
        s = segs("otsu", c, True, h)
        lab, n, thr, dq = s.segment_batch(imgs, return_distance=True)
        lab2, n2, thr2, dq2 = s.segment_batch(imgs, return_distance=True)
        assert np.array_equal(lab, lab2) and np.array_equal(n, n2) and np.array_equal(thr, thr2) and np.array_equal(dq, dq2)
        for b in range(5):
            l1, n1, t1, d1 = s.segment_batch(imgs[b:b + 1], return_distance=True)
            assert np.array_equal(l1[0], lab[b]) and n1[0] == n[b] and t1[0] == thr[b] and np.array_equal(d1[0], dq[b]), (c, h, b)
        assert n[4] == 0 and thr[4] == 777
        t = s.last_timing()
        assert set(t) == {"threshold_ms", "distance_ms", "seed_ms", "flood_ms"} and min(t.values()) > 0.0


def test_device_tensors_in_and_out(segs):
    import torch
    dev = torch.device("cuda", 0)
    for dtype in (np.uint16, np.uint8):
        imgs, _ = synth.label_images(53, 2, n_cells=40, dtype=dtype)
        s = segs("otsu", 1, True, 3)
        lab, n, thr, dq = s.segment_batch(imgs, return_distance=True)
        t = torch.from_numpy(imgs.view(np.int16) if dtype == np.uint16 else imgs).to(dev)
        tl, tn, tt, td = s.segment_batch(t, return_distance=True)
        assert tl.is_cuda and tl.dtype == torch.int32 and td.is_cuda and td.dtype == torch.uint8 and tuple(td.shape) == lab.shape
        assert np.array_equal(tl.cpu().numpy(), lab) and np.array_equal(td.cpu().numpy(), dq)
        assert np.array_equal(tn, n) and np.array_equal(tt, thr) and isinstance(tn, np.ndarray)
        out = s.segment_batch(t)
        assert len(out) == 3 and np.array_equal(out[0].cpu().numpy(), lab)


def test_without_the_option_the_plain_segmenter_answers():
    imgs, _ = synth.label_images(54, 2, n_cells=40)
    plain = S.ThresholdSegmenter(0, "otsu", 1, True)
    off = S.ThresholdSegmenter(0, "otsu", 1, True, split_touching=False, split_h=9)
    on = S.ThresholdSegmenter(0, "otsu", 1, True, split_touching=True, split_h=255)
    a, b = plain.segment_batch(imgs), off.segment_batch(imgs)
    elab, en, ethr = R.segment_batch(imgs, connectivity=1, fill_holes=True)
    assert len(b) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(b[0], elab) and np.array_equal(b[1], en) and np.array_equal(b[2], ethr)
    assert set(off.last_timing()) == {"threshold_ms", "label_ms"}
    with pytest.raises(ValueError):
        off.segment_batch(imgs, return_distance=True)
    c = on.segment_batch(imgs)                                 # no saddle is 127 px deep: one seed per component, the same labels
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    for s in (plain, off, on):
        s.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
def touching_pairs_image(seed=5, side=320):
    """[side, side, 3] uint16: touching pairs of round cells and a few single ones, channel 2 bright where the cells are,
    channel 1 textured as synth.label_images paints its cells."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    ana = rng.uniform(0.02, 0.08, (side, side))
    cells = np.zeros((side, side), bool)
    centres = []
    for gy in range(3):
        for gx in range(3):
            cy, cx = 60 + gy * 100 + rng.uniform(-6, 6), 60 + gx * 100 + rng.uniform(-6, 6)
            if (gy + gx) % 3 == 2:
                centres.append((cy, cx, 14.0))
            else:
                a = rng.uniform(0, np.pi)
                centres += [(cy - 11.5 * np.sin(a), cx - 11.5 * np.cos(a), 13.0), (cy + 11.5 * np.sin(a), cx + 11.5 * np.cos(a), 13.0)]
    for cy, cx, r in centres:
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        cells |= m
        ana[m] = rng.uniform(0.3, 0.8) + 0.15 * np.exp(-((yy[m] - cy) ** 2 + (xx[m] - cx) ** 2) / (2 * (0.4 * r) ** 2))
    ana += rng.normal(0.0, 0.02, (side, side))
    seg = np.where(cells, 0.7, 0.05) + rng.normal(0.0, 0.02, (side, side))
    img = np.zeros((side, side, 3), np.uint16)
    img[..., 1] = np.round(np.clip(ana, 0, 1) * 65535)
    img[..., 2] = np.round(np.clip(seg, 0, 1) * 65535)
    return img, len(centres)


def test_cell_extractor_end_to_end_counts_more_cells(tmp_path):
    """threshold_cell_extractor(split_touching=True) on a file of touching pairs yields as many cells as the restatement
    followed by tests/extract_reference.py, and more than without the option."""
    img, n_painted = touching_pairs_image()
    np.save(tmp_path / "pairs.npy", img)
    elab, en, _, _ = SR.split(np.ascontiguousarray(img[..., 2]), "otsu", 1, True, 3)
    crops, regs, status = XR.extract(elab, img[..., 1])
    assert status == XR.IMAGE_OK and en == n_painted == 15
    cells, stats = S.threshold_cell_extractor(split_touching=True)(str(tmp_path / "pairs.npy"))
    assert len(cells) == len(stats) == len(crops)
    assert [s["area"] for s in stats] == [r["area"] for r in regs if r["failed"] == 0]
    plain_cells, _ = S.threshold_cell_extractor()(str(tmp_path / "pairs.npy"))
    assert len(cells) > len(plain_cells) and len(cells) >= 12
    pcrops, _, pstatus = XR.extract(R.segment(np.ascontiguousarray(img[..., 2]))[0], img[..., 1])
    assert pstatus == XR.IMAGE_OK and len(plain_cells) == len(pcrops)
