"""The label expansion on the device (cs_label_expand through cellscreen.expand, ThresholdSegmenter(expand_distance=...) and
label_cell_extractor(expand_distance=...)) against the CPU restatement of tests/expand_reference.py, which tests/test_expand_cpu.py
holds to skimage.segmentation.expand_labels.

Labels and d2 are integers, so every comparison is np.array_equal: no tolerances.

The column pass takes 16 rows per step, the row pass a strip of 256 columns with a halo of isqrt(max_d2) on either side; SHAPES
crosses each one short, equal and one past, and has the single row and the single column.  The distances cover r = 1 (1 and 1.5:
max_d2 1 and 2), 2 (2.9: max_d2 8), 5 and 12."""
import functools

import numpy as np
import pytest

import expand_reference as ER
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import extract as X
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (70, 300), (1, 1)]
DISTANCES = [1, 1.5, 2.9, 5, 12]


@pytest.fixture(scope="module")
def expander():
    e = EX.LabelExpander(0)
    yield e
    e.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def to_np(a):
    if isinstance(a, np.ndarray):
        return a
    import torch
    if a.dtype == torch.uint16:
        return a.view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


@functools.lru_cache(maxsize=None)
def contents(shape, seed):
    """int32 [2,H,W]: random disks, and single pixels with five labels between them, which tie often."""
    H, W = shape
    rng = np.random.default_rng(seed)
    pts = np.zeros(shape, np.int32)
    for _ in range(max(1, H * W // 60)):
        pts[rng.integers(0, H), rng.integers(0, W)] = int(rng.integers(1, 6))
    out = np.stack([ER.disks(shape, max(1, H * W // 700), seed), pts])
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def nearest(shape, seed):
    return ER.nearest(contents(shape, seed))                            # the costly part, once per content whatever the distance


def wanted(shape, seed, max_d2):
    return ER.cut(nearest(shape, seed), max_d2)


def check(got, want):
    (g, d), (wg, wd) = got, want
    g, d = to_np(g), to_np(d)
    assert g.dtype == np.int32 and d.dtype == np.uint16 and g.shape == wg.shape and d.shape == wd.shape
    assert np.array_equal(g, wg) and np.array_equal(d, wd)


@pytest.mark.parametrize("shape", SHAPES)
def test_labels_and_d2_equal_the_restatement(expander, shape):
    seed = 7 * shape[0] + shape[1]
    lab = contents(shape, seed)
    for distance in DISTANCES:
        check(expander.expand_batch(lab, distance, return_d2=True), wanted(shape, seed, ER.max_d2_of(distance)))
    only = expander.expand_batch(lab, 5)                                # without the d2 plane
    assert isinstance(only, np.ndarray) and np.array_equal(only, wanted(shape, seed, 25)[0])


def test_two_labels_at_distance_127(expander):
    lab = np.zeros((1, 64, 64), np.int32)
    lab[0, 0, 0], lab[0, 63, 63] = 2, 1
    g, d = expander.expand_batch(lab, 127, return_d2=True)
    check((g, d), ER.expand(lab, 127 * 127))
    yy, xx = np.mgrid[0:64, 0:64]
    assert (g[0][yy + xx < 63] == 2).all() and (g[0][yy + xx >= 63] == 1).all()         # the anti-diagonal ties go to label 1
    assert int(d.max()) < ER.FAR
    lab[0, 63, 63] = 0                                                  # one label: the far corner is 2 * 63^2 = 7938 away, within 127
    check(expander.expand_batch(lab, 127, return_d2=True), ER.expand(lab, 127 * 127))
    far, d = expander.expand_batch(lab, 89, return_d2=True)             # 89^2 = 7921 < 7938: the far corner stays background
    assert far[0, 63, 63] == 0 and d[0, 63, 63] == ER.FAR and far[0, 63, 62] == 2 and d[0, 63, 62] == 63 * 63 + 62 * 62
    check((far, d), ER.expand(lab, 89 * 89))


def test_hand_made_ties_go_to_the_smallest_label(expander):
    def grown(lab, distance):
        g, d = expander.expand_batch(lab[None], distance, return_d2=True)
        check((g, d), ER.expand(lab[None], ER.max_d2_of(distance)))
        return g[0], d[0]

    row = np.zeros((7, 9), np.int32)
    row[3, 2], row[3, 6] = 5, 3                                         # four pixels apart in a row
    g, d = grown(row, 2)
    assert (g[3, 4], d[3, 4]) == (3, 4) and g[3, 3] == 5 and g[3, 5] == 3
    g, d = grown(np.ascontiguousarray(row.T), 2)                        # the same in a column: the up and the down candidate
    assert (g[4, 3], d[4, 3]) == (3, 4) and g[3, 3] == 5 and g[5, 3] == 3
    for col_label, row_label in ((7, 2), (2, 7)):                       # a column candidate against a row candidate, both at D2 = 9
        lab = np.zeros((9, 9), np.int32)
        lab[1, 4], lab[4, 7] = col_label, row_label
        g, d = grown(lab, 3)
        assert (g[4, 4], d[4, 4]) == (2, 9)
    # the pixel's own column gives best = 9 first; the window must still look at dx^2 == 9, where g = 0 and the label is smaller
    lab = np.zeros((9, 9), np.int32)
    lab[1, 4], lab[4, 1] = 7, 2
    g, d = grown(lab, 5)
    assert (g[4, 4], d[4, 4]) == (2, 9)
    lab[4, 7] = 1                                                       # and on the other side a smaller one still
    g, d = grown(lab, 5)
    assert (g[4, 4], d[4, 4]) == (1, 9)
    lab = np.zeros((9, 9), np.int32)                                    # four at D2 = 5 around (4, 4), knight's moves
    lab[2, 3], lab[3, 6], lab[6, 5], lab[5, 2] = 9, 8, 4, 6
    g, d = grown(lab, 2.9)
    assert (g[4, 4], d[4, 4]) == (4, 5)


def test_edge_cases(expander):
    corners = np.zeros((1, 20, 300), np.int32)
    corners[0, 0, 0], corners[0, 0, 299], corners[0, 19, 0], corners[0, 19, 299] = 4, 3, 2, 1
    for distance in (1, 5, 12, 127):
        check(expander.expand_batch(corners, distance, return_d2=True), ER.expand(corners, ER.max_d2_of(distance)))
    empty = np.zeros((2, 17, 257), np.int32)
    g, d = expander.expand_batch(empty, 12, return_d2=True)
    assert not g.any() and (d == ER.FAR).all()
    full = np.arange(1, 2 * 17 * 257 + 1, dtype=np.int32).reshape(2, 17, 257)
    g, d = expander.expand_batch(full, 12, return_d2=True)
    assert np.array_equal(g, full) and not d.any()
    big = np.zeros((1, 33, 270), np.int32)                              # ids up to 2^31 - 1, sparse, and the order of ids decides ties
    for k, v in enumerate((2 ** 31 - 1, 2 ** 31 - 2, 1000003, 7, 2 ** 30, 65536, 2 ** 24 + 1, 99)):
        big[0, 4 + 3 * k, 20 + 31 * k] = v
        big[0, 30 - 3 * k, 22 + 31 * k] = v // 2 + 1
    for distance in (2.9, 12, 127):
        g, d = expander.expand_batch(big, distance, return_d2=True)
        check((g, d), ER.expand(big, ER.max_d2_of(distance)))
        assert set(np.unique(g)) <= set(np.unique(big))                 # nothing is renumbered
    assert g.max() == 2 ** 31 - 1


def test_batch_equals_images_one_by_one(expander):
    shape = (70, 300)
    lab = np.stack([ER.disks(shape, n, n) for n in (3, 17, 40)])
    whole, wd = expander.expand_batch(lab, 12, return_d2=True)
    check((whole, wd), ER.expand(lab, 144))
    for b in range(3):
        one, od = expander.expand_batch(lab[b:b + 1].copy(), 12, return_d2=True)
        assert np.array_equal(one[0], whole[b]) and np.array_equal(od[0], wd[b])
    assert len({int((whole[b] > 0).sum()) for b in range(3)}) == 3


def test_in_place_input_kinds_and_repeatability(expander):
    import torch
    shape, seed = (70, 300), 11
    lab = contents(shape, seed)
    want = wanted(shape, seed, 144)
    a, ad = expander.expand_batch(lab, 12, return_d2=True)
    b, bd = expander.expand_batch(lab, 12, return_d2=True)
    check((a, ad), want)
    assert np.array_equal(a, b) and np.array_equal(ad, bd)              # bit-identical run to run
    t = expander.last_timing()
    assert set(t) == {"expand_columns_ms", "expand_rows_ms"} and all(np.isfinite(v) and v > 0.0 for v in t.values())
    host = lab.copy()
    r, d = expander.expand_batch(host, 12, return_d2=True, out=host)    # numpy, in place
    assert r is host
    check((host, d), want)
    dev = as_tensor(lab.copy())
    r, d = expander.expand_batch(dev, 12, return_d2=True)               # a tensor in: tensors out, the input untouched
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.int32 and d.dtype == torch.uint16 and d.is_cuda
    check((r, d), want)
    assert np.array_equal(to_np(dev), lab)
    r2, d2 = expander.expand_batch(dev, 12, return_d2=True, out=dev)    # a tensor, in place
    assert r2 is dev
    check((dev, d2), want)
    other = torch.empty_like(dev)
    assert expander.expand_batch(as_tensor(lab.copy()), 12, out=other) is other and np.array_equal(to_np(other), want[0])
    with pytest.raises(TypeError):
        expander.expand_batch(lab.copy(), 12, out=other)
    with pytest.raises(ValueError):
        expander.expand_batch(as_tensor(lab.copy())[:, :, ::2], 12)


def test_a_negative_label_is_an_error_status_and_the_handle_stays_usable(expander):
    shape, seed = (17, 257), 5
    lab = contents(shape, seed)
    for where in ((0, 0, 0), (1, 16, 256), (0, 9, 255)):
        bad = lab.copy()
        bad[where] = -1
        for arg in (bad, as_tensor(bad)):
            with pytest.raises(L.CellScreenError) as ei:
                expander.expand_batch(arg, 5)
            assert ei.value.status == -1 and "negative label" in str(ei.value)
            check(expander.expand_batch(lab, 5, return_d2=True), wanted(shape, seed, 25))


def nuclei_scene():
    """uint16 [2,96,128]: five bright blobs per image on a noisy background."""
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.empty((2, H, W), np.uint16)
    for b in range(2):
        f = 300.0 + rng.normal(0.0, 10.0, (H, W))
        for y, x, r in ((24, 25, 9), (30, 80, 12), (70, 40, 10), (70, 100, 7 + 4 * b), (50, 62, 5)):
            f += 4000.0 * np.exp(-(((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (r / 1.6) ** 2)) ** 2)
        imgs[b] = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
    return imgs


@pytest.mark.parametrize("kw", [dict(), dict(split_touching=True)], ids=["labels", "split"])
def test_segmenter_grows_its_own_labels_in_place(kw):
    imgs = nuclei_scene()
    plain = S.ThresholdSegmenter(0, **kw)
    base, base_n, base_thr = plain.segment_batch(imgs)
    base_dist = plain.segment_batch(imgs, return_distance=True)[3] if kw else None
    if not kw:
        assert np.array_equal(base, R.segment_batch(imgs)[0])
    assert "expand_rows_ms" not in plain.last_timing()
    plain.close()
    for distance in (2.9, 6):
        want = ER.expand(base, ER.max_d2_of(distance))[0]
        seg = S.ThresholdSegmenter(0, expand_distance=distance, **kw)
        for images in (imgs, as_tensor(imgs.view(np.int16))):
            labels, n_labels, thr = seg.segment_batch(images)
            assert np.array_equal(to_np(labels), want) and np.array_equal(n_labels, base_n) and np.array_equal(thr, base_thr)
            t = seg.last_timing()
            assert {"expand_columns_ms", "expand_rows_ms", "threshold_ms"} <= set(t) and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        assert (want > 0).sum() > (base > 0).sum()
        if kw:
            labels, n_labels, thr, dist = seg.segment_batch(imgs, return_distance=True)         # the distances are the split's own
            assert np.array_equal(labels, want) and np.array_equal(dist, base_dist)
        truth = np.ascontiguousarray(want)
        stats, lab2, n2 = seg.score_batch(imgs, truth, thresholds=(0.5, 0.9))                   # the grown labels are what is scored
        assert np.array_equal(lab2, want) and stats["total"]["by_threshold"][1]["tp"] == int(base_n.sum())
        assert stats["total"]["by_threshold"][1]["fp"] == 0
        seg.close()


def test_extraction_behind_it_sees_larger_regions():
    imgs = nuclei_scene()
    ext = X.CellExtractor(0, min_area=20, min_mean=0.0, min_std=0.0)
    plain = S.ThresholdSegmenter(0, extractor=ext)
    dev = as_tensor(imgs.view(np.int16))
    before = ext.extract_batch(dev, plain.segment_batch(dev)[0]).regions
    for distance in (2.9, 6):
        seg = S.ThresholdSegmenter(0, extractor=ext, expand_distance=distance)
        after = ext.extract_batch(dev, seg.segment_batch(dev)[0]).regions
        assert len(after) == len(before) >= 8
        assert np.array_equal(after["image"], before["image"]) and np.array_equal(after["label"], before["label"])
        k = int(np.ceil(distance))
        for lo in ("minr", "minc"):
            assert (after[lo] <= before[lo]).all() and (after[lo] >= before[lo] - k).all()
        for hi in ("maxr", "maxc"):
            assert (after[hi] >= before[hi]).all() and (after[hi] <= before[hi] + k).all()
        assert (after["area"] >= before["area"]).all() and (after["area"] > before["area"]).any()
    ext.close()


def test_label_cell_extractor_grows_the_caller_s_labels_on_the_device(tmp_path):
    img = nuclei_scene()[0]
    path = str(tmp_path / "field.npy")
    np.save(path, img)
    nuclei = R.segment_batch(img[None])[0][0].astype(np.int64) * 1000          # a caller's own ids, int64 and sparse
    qc = dict(min_area=120, min_mean=0.0, min_std=0.0)                  # the smallest nucleus passes only once it has grown
    cells, stats = X.label_cell_extractor(lambda seg: nuclei, expand_distance=6, **qc)(path)
    grown = ER.expand(nuclei, 36)[0]
    ext = X.CellExtractor(0, **qc)
    want = ext.extract_batch(img[None], grown[None])
    assert len(cells) == len(want.cells) == len(stats) > 0 and stats == X.region_stats(want.regions)
    assert all(np.array_equal(c, w) for c, w in zip(cells, want.cells))
    plain_cells, plain_stats = X.label_cell_extractor(lambda seg: nuclei, **qc)(path)
    assert len(stats) > len(plain_stats) > 0 and min(s["area"] for s in stats) > min(s["area"] for s in plain_stats)
    with pytest.raises(ValueError):
        X.label_cell_extractor(lambda seg: nuclei << 32, expand_distance=6, **qc)(path)           # ids beyond int32
    ext.close()
