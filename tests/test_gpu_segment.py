"""The built-in segmenter on the device (csrc/segment.hip through cellscreen.segment) against the CPU restatement of
tests/segment_reference.py, which tests/golden/golden_segment.npz pins to scikit-image 0.18.3 and SciPy.

Every output is an integer (thresholds, component counts, label images), so every comparison is np.array_equal: there are no
tolerances.  The end-to-end tests compare the CSV files byte for byte."""
import os

import numpy as np
import pytest

import segment_reference as R
from cellscreen import extract as X
from cellscreen import segment as S
from cellscreen import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_segment.npz")
OPTIONS = [(c, f) for c in (1, 2) for f in (False, True)]


@pytest.fixture(scope="module")
def segs():
    """ThresholdSegmenter per (threshold, connectivity, fill_holes), made on demand, closed at the end."""
    made = {}

    def get(threshold="otsu", connectivity=1, fill_holes=True):
        key = (threshold, connectivity, fill_holes)
        if key not in made:
            made[key] = S.ThresholdSegmenter(0, threshold, connectivity, fill_holes)
        return made[key]

    yield get
    for s in made.values():
        s.close()


def check(segs, images, channel=None, threshold="otsu", connectivity=1, fill_holes=True):
    """One device call on a stack against the restatement, image by image; returns the device's outputs."""
    lab, n, thr = segs(threshold, connectivity, fill_holes).segment_batch(images, channel=channel)
    elab, en, ethr = R.segment_batch(images, channel=channel, threshold=threshold, connectivity=connectivity, fill_holes=fill_holes)
    assert lab.dtype == np.int32 and lab.shape == elab.shape and n.dtype == np.int32 and thr.dtype == np.int32
    assert np.array_equal(thr, ethr), (thr, ethr)
    assert np.array_equal(n, en), (n, en)
    for b in range(len(elab)):
        assert np.array_equal(lab[b], elab[b]), (b, int((lab[b] != elab[b]).sum()))
    return lab, n, thr


def check_mask(segs, mask):
    """A boolean mask as a uint8 image under the fixed threshold 0, for every connectivity and hole-filling option."""
    img = np.ascontiguousarray(mask, np.uint8)[None]
    counts = {}
    for c, f in OPTIONS:
        _, n, _ = check(segs, img, threshold=0, connectivity=c, fill_holes=f)
        counts[c, f] = int(n[0])
    return counts


# ---- thresholds, counts and labels on the golden images and on synthetic cell images ---------------------------------------
def test_golden_images(segs):
    g = np.load(GOLDEN)
    for i in range(int(g["n"])):
        img = g[f"image_{i}"]
        for c, f in OPTIONS:
            lab, n, thr = check(segs, img[None], connectivity=c, fill_holes=f)
            assert int(thr[0]) == int(g[f"thr_{i}"])
            assert np.array_equal(lab[0], g[f"{'f' if f else ''}lab{c}_{i}"])
            fixed = int(g[f"thr_{i}"]) // 2 if i % 2 else min(int(g[f"thr_{i}"]) + 3, int(img.max()))
            check(segs, img[None], threshold=fixed, connectivity=c, fill_holes=f)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("side,n_cells,batch", [(256, 24, 3), (1024, 300, 2)])
def test_synthetic_images(segs, dtype, channels, side, n_cells, batch):
    imgs, _ = synth.label_images(41 + side + channels, batch, hw=(side, side), n_cells=n_cells, dtype=dtype, channels=channels)
    if channels == 1:
        # one channel is the analysis channel; give it the segmentation channel's look (bright cells on a dark background)
        imgs = np.ascontiguousarray(synth.label_images(41 + side, batch, hw=(side, side), n_cells=n_cells, dtype=dtype)[0][..., 2])
    for c, f in OPTIONS:
        _, n, thr = check(segs, imgs, connectivity=c, fill_holes=f)
        assert n.min() >= 5
        check(segs, imgs, threshold=int(thr[0]) - 1, connectivity=c, fill_holes=f)
    if channels == 3:
        check(segs, imgs, channel=1)                              # another channel of the same stack, read in place
        check(segs, np.ascontiguousarray(imgs[..., 2:3]))         # [B,H,W,1]


def test_otsu_on_constant_two_valued_and_full_range_images(segs):
    for dt, top in ((np.uint8, 255), (np.uint16, 65535)):
        rng = np.random.default_rng(top)
        stack = np.stack([np.full((50, 70), top // 3, dt), np.full((50, 70), 0, dt), np.full((50, 70), top, dt),
                          np.where(rng.random((50, 70)) < 0.4, top, 0).astype(dt),
                          np.where(rng.random((50, 70)) < 0.7, 17, 16).astype(dt),
                          rng.integers(0, top + 1, (50, 70)).astype(dt)])
        lab, n, thr = check(segs, stack, fill_holes=False)
        assert list(thr[:4]) == [top // 3, 0, top, 0] and list(n[:3]) == [0, 0, 0] and not lab[:3].any()


# ---- shapes the tiling must survive (fixed-threshold masks) -------------------------------------------------------------------
def _spiral(H, W):
    """A one-pixel-wide rectangular spiral with one-pixel gaps between its turns: one component of about H * W / 2 pixels."""
    m = np.zeros((H, W), bool)
    inside = lambda r, c: 0 <= r < H and 0 <= c < W
    r, c, dr, dc = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        moved = False
        while (inside(r + dr, c + dc) and not m[r + dr, c + dc]
               and not (inside(r + 2 * dr, c + 2 * dc) and m[r + 2 * dr, c + 2 * dc])):
            r, c = r + dr, c + dc
            m[r, c] = True
            moved = True
        if not moved:
            return m
        dr, dc = dc, -dr


def _comb(H, W):
    """A serpentine: full rows every other line, joined alternately at the right and at the left end."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, r in enumerate(range(1, H, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = True
    return m


def _rings(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.maximum(np.abs(yy - H // 2), np.abs(xx - W // 2))
    m = (d % 6 < 2) & (d < min(H, W) // 2 - 3)                    # nested square rings: holes inside holes
    d2 = np.hypot(yy - H // 4, xx - W // 4)
    return m | ((d2 < 20) & (d2.astype(int) % 5 == 0) & (d % 6 >= 3))


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (37, 53), (4096, 3), (3, 4096), (16, 64), (17, 65), (130, 200)])
def test_small_and_thin_shapes(segs, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for m in (rng.random(shape) < 0.55, np.ones(shape, bool), np.zeros(shape, bool)):
        counts = check_mask(segs, m)
        if m.all():
            assert set(counts.values()) == {1}
        if not m.any():
            assert set(counts.values()) == {0}


def test_checkerboard(segs):
    yy, xx = np.mgrid[0:150, 0:203]
    m = (yy + xx) % 2 == 0
    counts = check_mask(segs, m)
    assert counts[1, False] == int(m.sum()) and counts[2, False] == 1 and counts[1, True] < 10


@pytest.mark.parametrize("make,shape", [(_spiral, (300, 517)), (_spiral, (1025, 1100)), (_comb, (301, 700)), (_comb, (1024, 2048)),
                                        (_rings, (256, 256)), (_rings, (700, 531))])
def test_long_winding_components_and_nested_holes(segs, make, shape):
    m = make(*shape)
    counts = check_mask(segs, m)
    if make is not _rings:
        assert counts[1, False] == 1 and counts[1, True] == 1 and m.sum() > m.size // 3
    if make is _rings:
        assert counts[1, True] < counts[1, False]                 # filling merged the rings with what they enclose
    check_mask(segs, ~m)


@pytest.mark.parametrize("density", [0.3, 0.5, 0.593])
@pytest.mark.parametrize("shape", [(512, 512), (1000, 1111)])
def test_random_noise_near_the_percolation_threshold(segs, density, shape):
    rng = np.random.default_rng(int(density * 1000) + shape[0])
    check_mask(segs, rng.random(shape) < density)


# ---- batches, runs, device tensors ------------------------------------------------------------------------------------------
def test_batch_independence_and_determinism(segs):
    imgs, _ = synth.label_images(52, 5)
    rng = np.random.default_rng(52)
    imgs[3, ..., 2] = np.where(rng.random((256, 256)) < 0.593, 40000, 100)       # one image of long winding components
    imgs[4, ..., 2] = 777                                                          # one constant image
    for c, f in OPTIONS:
        s = segs("otsu", c, f)
        lab, n, thr = s.segment_batch(imgs)
        lab2, n2, thr2 = s.segment_batch(imgs)
        assert np.array_equal(lab, lab2) and np.array_equal(n, n2) and np.array_equal(thr, thr2)
        for b in range(5):
            l1, n1, t1 = s.segment_batch(imgs[b:b + 1])
            assert np.array_equal(l1[0], lab[b]) and n1[0] == n[b] and t1[0] == thr[b], (c, f, b)
        assert n[4] == 0 and thr[4] == 777


def test_device_tensors_in_and_out(segs):
    import torch
    dev = torch.device("cuda", 0)
    for dtype in (np.uint16, np.uint8):
        imgs, _ = synth.label_images(53, 2, dtype=dtype)
        s = segs("otsu", 2, True)
        lab, n, thr = s.segment_batch(imgs)
        t = torch.from_numpy(imgs.view(np.int16) if dtype == np.uint16 else imgs).to(dev)
        tl, tn, tt = s.segment_batch(t)
        assert tl.is_cuda and tl.dtype == torch.int32 and tuple(tl.shape) == lab.shape
        assert np.array_equal(tl.cpu().numpy(), lab) and np.array_equal(tn, n) and np.array_equal(tt, thr)
        assert isinstance(tn, np.ndarray) and isinstance(tt, np.ndarray)


def test_extraction_reads_the_device_labels_without_a_host_copy():
    import torch
    dev = torch.device("cuda", 0)
    imgs, _ = synth.label_images(7, 2)
    ext = X.CellExtractor(0)
    seg = S.ThresholdSegmenter(0, "otsu", 1, False, extractor=ext)
    t = torch.from_numpy(imgs.view(np.int16)).to(dev)
    labels, n, _ = seg.segment_batch(t)
    assert labels.is_cuda and list(n) == [10, 10]
    r = ext.extract_batch(t, labels)                              # channel 1 is analysed, channel 2 was segmented
    elab, en, _ = R.segment_batch(imgs, connectivity=1, fill_holes=False)
    e = ext.extract_batch(imgs, elab)
    assert np.array_equal(r.regions, e.regions) and np.array_equal(r.status, e.status) and np.array_equal(r.cell_image, e.cell_image)
    assert len(e.cells) >= 2 and np.array_equal(r.cells.cpu().numpy().view(np.uint32), e.cells.view(np.uint32))
    assert [int((e.regions["area"][e.regions["image"] == b] >= 200).sum()) for b in range(2)] == [9, 10]
    assert seg._handle is ext._handle and seg.last_timing()["label_ms"] > 0.0
    ext.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _restatement_segmenter(**kw):
    return lambda seg: R.segment(np.ascontiguousarray(seg), **kw)[0]


@pytest.mark.parametrize("opts", [dict(threshold="otsu", connectivity=1, fill_holes=False), dict()])
def test_screening_end_to_end(tmp_path, golden_cae, golden_det, opts):
    """ProductionMutantScreening over folders of .npy images with threshold_cell_extractor writes, byte for byte, the CSVs
    that label_cell_extractor(<the restatement as the segmenter>) writes."""
    import helpers as H
    import pandas as pd
    from cellscreen import model_io
    from cellscreen.screening import ProductionMutantScreening
    mdir = str(tmp_path / "models")
    model_io.save_model_dir(mdir, H.cae_from_golden(golden_cae), None, H.det_from_golden(golden_det))
    folders = {}
    for k, (seed, n) in enumerate(((7, 2), (22, 3))):
        d = tmp_path / f"strain{k}"
        d.mkdir()
        imgs, _ = synth.label_images(seed, n)
        for i in range(n):
            np.save(d / f"img{i}.npy", imgs[i])
        folders[f"S{k}"] = str(d)
    ropts = dict(dict(threshold="otsu", connectivity=1, fill_holes=True), **opts)
    a = ProductionMutantScreening(mdir, cell_extractor=S.threshold_cell_extractor(**opts), file_pattern="*.npy")
    a.screen_mutant_samples(folders, str(tmp_path / "a"))
    b = ProductionMutantScreening(mdir, cell_extractor=X.label_cell_extractor(_restatement_segmenter(**ropts)), file_pattern="*.npy")
    b.screen_mutant_samples(folders, str(tmp_path / "b"))
    for name in ("detailed_cell_results.csv", "screening_summary.csv"):
        fa, fb = open(tmp_path / "a" / name, "rb").read(), open(tmp_path / "b" / name, "rb").read()
        assert fa == fb, name
    summary = pd.read_csv(tmp_path / "a" / "screening_summary.csv", index_col=0)
    assert list(summary.index) == ["S0", "S1"] and list(summary["files_processed"]) == [2, 3]
    assert (summary["total_cells"] >= 1).all()                   # at least one cell passes per sample


def test_create_training_dataset_end_to_end(tmp_path):
    from cellscreen.training import ImprovedAnomalyDetectionTraining
    d = tmp_path / "train"
    d.mkdir()
    imgs, _ = synth.label_images(7, 2)
    for i in range(2):
        np.save(d / f"f{i}.npy", imgs[i])
    np.save(d / "g_gray.npy", np.ascontiguousarray(synth.label_images(33, 1, dtype=np.uint8)[0][0, ..., 2]))     # a 2-D uint8 image
    opts = dict(threshold="otsu", connectivity=1, fill_holes=False)
    outs = []
    for name, extractor in (("a", S.threshold_cell_extractor(**opts)), ("b", X.label_cell_extractor(_restatement_segmenter(**opts)))):
        tr = ImprovedAnomalyDetectionTraining(str(tmp_path / name))
        cells, df = tr.create_training_dataset(str(d), extractor, file_pattern="*.npy")
        outs.append((cells, df))
    assert len(outs[0][0]) >= 2 and np.array_equal(outs[0][0], outs[1][0])
    for name in ("cell_statistics.csv", "file_summary.csv"):
        fa, fb = open(tmp_path / "a" / name, "rb").read(), open(tmp_path / "b" / name, "rb").read()
        assert fa == fb and len(fa.splitlines()) >= 3, name


def test_extractor_errors_are_label_cell_extractor_s(tmp_path):
    ex = S.threshold_cell_extractor()
    np.save(tmp_path / "two.npy", np.zeros((32, 32, 2), np.uint16))
    np.save(tmp_path / "flt.npy", np.zeros((32, 32), np.float32))
    with pytest.raises(ValueError):
        ex(str(tmp_path / "two.npy"))
    with pytest.raises(TypeError):
        ex(str(tmp_path / "flt.npy"))
    with pytest.raises(ValueError):
        ex(str(tmp_path / "image.png"))
    np.save(tmp_path / "dark.npy", np.zeros((64, 64, 3), np.uint16))              # constant: no labels, no cells, no error
    cells, stats = ex(str(tmp_path / "dark.npy"))
    assert cells == [] and stats == []
