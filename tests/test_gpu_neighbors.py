"""The per-object neighbour records on the device (cs_label_neighbors through cellscreen.neighbors) against the CPU restatement of
tests/neighbors_reference.py, which tests/test_neighbors_cpu.py holds to its slow form, to SciPy's records and to closed forms.

Every record is an integer: np.array_equal on geom, objects, offsets and pairs, the rows of absent objects included.

The tile of nb_scan (csrc/neighbors.hip) is 32 rows x 64 columns per workgroup, with a halo of floor(sqrt(max_d2)) <= 32 pixels on
every side in LDS; a thread of its first pass owns 8 columns of one row.  SHAPES crosses the 32 rows and the 64 columns one short,
equal and one past, keeps the shapes of the other label tools (their tile is 64 x 256), and has the single row, the single column and
the single pixel.  The tile's pair table in LDS has 512 slots and its object table 128: an image where every pixel is its own label
overflows both.  The halo tests put pairs on opposite sides of the tile corner at (64, 64), at D2 exactly max_d2 and at the smallest
squared distance between two pixels above it: that is max_d2 + 1 for 1024, 1009 for 1000 and 4 for 2, since 1001 and 3 are no sums of
two squares."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import neighbors_reference as NR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import neighbors as NB
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1), (31, 63), (32, 64), (33, 65)]
MAX_D2 = (1, 2, 25, 1024)
NAMES = ("geom", "objects", "offsets", "pairs")
DTYPES = (np.int64, np.int32, np.int64, np.int32)
CORNER = (64, 64)                                                        # a corner of four tiles


@pytest.fixture(scope="module")
def measurer():
    m = NB.NeighborMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def batch_of(shape, seed):
    """(name, labels int32 [2,H,W]) per kind of content, the two images different"""
    out = []
    for (name, a), (_, b) in zip(NR.contents(shape, seed), NR.contents(shape, seed + 1)):
        lab = np.stack([a, b[::-1, ::-1]])
        lab.flags.writeable = False
        out.append((name, lab))
    return out


def same(got, want, what=""):
    assert len(got) == len(want) == 4, what
    for k in range(4):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype == DTYPES[k] and g.shape == w.shape, (what, NAMES[k])
        assert np.array_equal(g, w), (what, NAMES[k])


def check(measurer, lab, max_d2, max_label=None, what="", **kw):
    """measure_dense against the restatement; returns the device's records"""
    got = measurer.measure_dense(lab, math.sqrt(max_d2), max_label, **kw)
    same(got, NR.measure(lab, max_d2, max_label), f"{what} max_d2={max_d2}")
    return got


def rows_of(rec):
    geom, objects, offsets, pairs = rec
    B, M = geom.shape[:2]
    return {(b, a): pairs[offsets[b * M + a - 1]:offsets[b * M + a]].tolist() for b in range(B) for a in range(1, M + 1)}


def above(max_d2):
    """the smallest squared distance between two pixels above max_d2, and the offsets at max_d2 and at it"""
    sums = {}
    for dr in range(0, 34):
        for dc in range(0, 34):
            sums.setdefault(dr * dr + dc * dc, []).append((dr, dc))
    nxt = min(s for s in sums if s > max_d2)
    return nxt, sums[max_d2], sums[nxt]


@pytest.mark.parametrize("shape", SHAPES)
def test_records_equal_the_restatement_across_the_tiles(measurer, shape):
    seed = 7 * shape[0] + shape[1]
    for name, lab in batch_of(shape, seed):
        for max_d2 in MAX_D2:
            got = check(measurer, lab, max_d2, what=f"{shape} {name}")
    t = measurer.measure_batch(lab, 32)
    d = NR.derive(*got)
    assert len(t) == len(d["label"]) and all(np.array_equal(getattr(t, k), v, equal_nan=True) for k, v in d.items())
    assert np.array_equal(t.pairs, got[3])


@pytest.mark.parametrize("max_d2", [1024, 1000, 2])
def test_halo_pairs_across_a_tile_corner(measurer, max_d2):
    nxt, at, over = above(max_d2)
    assert (max_d2, nxt) in ((1024, 1025), (1000, 1009), (2, 4)) and at and over
    shape, images, near = (132, 140), [], []
    for offs, is_near in ((at, True), (over, False)):
        for dr, dc in offs:
            for sr, sc in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                for ar, ac in ((CORNER[0] - 1, CORNER[1] - 1), CORNER, (CORNER[0] - 1, CORNER[1]), (CORNER[0], CORNER[1] - 1)):
                    lab = np.zeros(shape, np.int32)                      # single pixels: a at the corner, b across an edge or the corner
                    lab[ar, ac], lab[ar + sr * dr, ac + sc * dc] = 1, 2
                    images.append(lab)
                    near.append(is_near)
    lab = np.stack(images)
    geom, objects, offsets, pairs = check(measurer, lab, max_d2, what="pixel pairs")
    near = np.array(near).astype(np.int32)
    assert np.array_equal(objects[:, 0], objects[:, 1]) and (objects[:, 0, 0] == 1).all()
    assert np.array_equal(objects[:, 0, 2], near) and np.array_equal(objects[:, 0, 1], near)
    assert pairs.shape[0] == 2 * near.sum() and (pairs[:, 1] == max_d2).all() and (pairs[:, 2] == 1).all()
    # disks of radius 2 in place of the pixels, their centres 2 further out along the longer side of the offset: the nearest pixels
    # of the two are the pair above, so D2 is max_d2 or the distance just above it again
    images, near = [], []
    rr, cc = np.indices(shape)
    for offs, is_near in ((at, True), (over, False)):
        for dr, dc in offs:
            for sr, sc in ((1, 1), (-1, -1), (1, -1)):
                for ar, ac in ((CORNER[0] - 1, CORNER[1] - 1), CORNER):
                    lab = np.zeros(shape, np.int32)
                    br, bc = ar + sr * dr, ac + sc * dc
                    ur, uc = (0, 2 * sc) if dc >= dr else (2 * sr, 0)
                    for label, (r, c) in ((3, (ar - ur, ac - uc)), (1, (br + ur, bc + uc))):
                        lab[(rr - r) ** 2 + (cc - c) ** 2 <= 4] = label
                    images.append(lab)
                    near.append(is_near)
    geom, objects, offsets, pairs = check(measurer, np.stack(images), max_d2, what="disks")
    near = np.array(near).astype(np.int32)
    assert (geom[:, 0, 0] == 13).all() and np.array_equal(objects[:, 2, 2], near) and np.array_equal(objects[:, 0, 2], near)
    assert pairs.shape[0] == 2 * near.sum() and (pairs[:, 1] == max_d2).all()


def test_halo_image_corners_and_an_object_between_two_others(measurer):
    shape = (70, 130)
    lab = np.zeros((2,) + shape, np.int32)
    for k, (r, c) in enumerate(((0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1))):
        lab[0, r, c] = k + 1                                             # a pixel in every corner of the image, a second object near it
        lab[0, min(max(r, 3), shape[0] - 4), min(max(c, 4), shape[1] - 5)] = k + 5
    lab[1, :3, :3], lab[1, -2:, -2:], lab[1, :2, -4:], lab[1, -5:, :1] = 1, 2, 3, 4   # blocks in the corners
    lab[1, 20:50, 40:44], lab[1, 25:45, 60:70], lab[1, 20:50, 80:84] = 5, 6, 7        # 6 lies between 5 and 7
    for max_d2 in (1, 2, 25, 1000, 1024):
        rec = check(measurer, lab, max_d2, what="corners")
    rows = rows_of(rec)
    assert [5, 25, 1] in rows[(0, 1)] and [1, 25, 1] in rows[(0, 5)]   # the pixel at (0, 0) and the one at (3, 4)
    assert [r[:2] for r in rows[(1, 5)]] == [[6, 17 ** 2]] and [r[:2] for r in rows[(1, 7)]] == [[6, 11 ** 2]]         # 5 and 7 are 37 px apart
    wide = np.zeros((1, 40, 60), np.int32)
    wide[0, 5:35, 10:14], wide[0, 8:30, 17:19], wide[0, 5:35, 22:26] = 1, 2, 3       # 2 lies between 1 and 3, which are 9 px apart
    rows = rows_of(check(measurer, wide, 81, what="bars", table_log2=12))
    assert [r[:2] for r in rows[(0, 1)]] == [[2, 16], [3, 81]] and [r[:2] for r in rows[(0, 3)]] == [[1, 81], [2, 16]]
    assert [r[:2] for r in rows_of(check(measurer, wide, 80, what="bars"))[(0, 1)]] == [[2, 16]]


def test_one_long_row(measurer):
    n = 700
    lab = np.zeros((2, 3, n + 2), np.int32)
    lab[:, 1, 1:n + 1] = 1                                               # the bar
    lab[0, 0, 1:n + 1] = np.arange(2, n + 2)                             # a single-pixel object beside every pixel of it
    lab[1, 2, 1:n + 1] = np.arange(n + 1, 1, -1)                         # below it and in the other order
    geom, objects, offsets, pairs = check(measurer, lab, 1, what="long row")
    for b in range(2):
        assert objects[b, 0].tolist() == [n, n, n]
        row = pairs[offsets[b * (n + 1)]:offsets[b * (n + 1) + 1]]
        assert row.shape == (n, 3) and np.array_equal(row[:, 0], np.arange(2, n + 2)) and (row[:, 1] == 1).all() and (row[:, 2] == 1).all()
    assert (objects[:, 1:, 2] >= 2).all() and (objects[:, 1:, 2] <= 3).all()             # the bar and one or two pixels beside


@functools.lru_cache(maxsize=None)
def own_labels():
    """every pixel its own label on 64 x 256, the second image in another order; the restatement's records at max_d2 = 2"""
    shape = (64, 256)
    n = shape[0] * shape[1]
    lab = np.stack([np.arange(1, n + 1, dtype=np.int32).reshape(shape), np.arange(n, 0, -1, dtype=np.int32).reshape(shape).T.reshape(shape)])
    lab.flags.writeable = False
    return lab, NR.measure(lab, 2)


def test_more_labels_and_pairs_in_a_tile_than_the_lds_tables_have_slots(measurer):
    lab, want = own_labels()
    got = measurer.measure_dense(lab, math.sqrt(2))
    same(got, want, "own labels")
    geom, objects, offsets, pairs = got
    H, W = lab.shape[1:]
    rr, cc = np.indices((H, W))
    sides = ((rr == 0) | (rr == H - 1)).astype(int) + ((cc == 0) | (cc == W - 1)).astype(int)
    degree = np.choose(sides, [8, 5, 3])
    for b in range(2):
        assert np.array_equal(objects[b, lab[b].ravel() - 1, 2], degree.ravel())          # 3 / 5 / 8 by position
    assert (objects[:, :, 0] == 1).all() and (objects[:, :, 1] == 1).all() and set(np.unique(pairs[:, 1])) == {1, 2}
    assert set(np.unique(pairs[:, 2])) == {0, 1} and pairs[:, 2].sum() == 2 * H * W and (pairs[pairs[:, 2] == 1, 1] == 1).all()
    P = np.pad(lab[0], 1, constant_values=1 << 30)                        # n_near is 1 for the smallest-labelled 4-neighbour
    least = np.minimum(np.minimum(P[:-2, 1:-1], P[2:, 1:-1]), np.minimum(P[1:-1, :-2], P[1:-1, 2:]))
    first = pairs[:offsets[H * W]]
    assert np.array_equal(first[first[:, 2] == 1, 0], least.ravel())


def test_global_table_growth_leaves_the_records_unchanged(measurer):
    lab, want = own_labels()
    got = measurer.measure_dense(lab, math.sqrt(2), table_log2=10)
    log2, grows = measurer.last_table()
    same(got, want, "table_log2=10")
    assert grows > 0 and log2 == 10 + grows and (1 << log2) >= want[3].shape[0]
    same(measurer.measure_dense(lab, math.sqrt(2)), want, "automatic")
    log2, grows = measurer.last_table()
    assert log2 >= 16 and grows >= 0


def test_a_4096_plane(measurer):
    side = 4096
    lab = np.ones((1, side, side), np.int32)
    lab[0, :, side // 2:] = 2
    geom, objects, offsets, pairs = measurer.measure_dense(lab, 1)
    border = 2 * side + 2 * (side // 2) - 4
    assert objects[0].tolist() == [[border, side, 1], [border, side, 1]] and offsets.tolist() == [0, 1, 2]
    assert pairs.tolist() == [[2, 1, side], [1, 1, side]]
    half = side * side // 2
    assert geom[0].tolist() == [[half, half * (side - 1) // 2, half * (side // 2 - 1) // 2], [half, half * (side - 1) // 2, half * (3 * side // 2 - 1) // 2]]
    lab[:] = 1
    geom, objects, offsets, pairs = measurer.measure_dense(lab, 1)
    assert objects[0].tolist() == [[4 * side - 4, 0, 0]] and offsets.tolist() == [0, 0] and pairs.shape == (0, 3)
    assert geom[0, 0].tolist() == [side * side, side * side * (side - 1) // 2, side * side * (side - 1) // 2]


def test_scalar_path_for_odd_widths_and_unaligned_tensor_views(measurer):
    import torch
    for shape in ((33, 258), (20, 7), (9, 301)):                         # widths that are no multiple of 4
        for name, lab in batch_of(shape, 3):
            check(measurer, lab, 25, what=f"{shape} {name}")
    shape = (40, 264)                                                    # a multiple of 4: only the pointer differs
    lab = batch_of(shape, 4)[3][1]
    dev = torch.device("cuda", 0)
    want = NR.measure(lab, 13)
    same(measurer.measure_dense(as_tensor(lab), math.sqrt(13)), want, "aligned")
    for by in (1, 2, 3):
        flat = torch.empty(lab.size + by, dtype=torch.int32, device=dev)
        view = flat[by:].view(lab.shape)
        view.copy_(as_tensor(lab))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        same(measurer.measure_dense(view, math.sqrt(13)), want, f"shifted by {by}")


def test_input_kinds_repeatability_and_batch_independence(measurer):
    shape = (70, 300)
    lab = np.stack([NR.disks(shape, 40, k, radii=(3, 9)) for k in (1, 2, 3)])
    a = check(measurer, lab, 50, what="numpy in")
    b = measurer.measure_dense(lab, math.sqrt(50))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))               # bit-identical run to run
    t = measurer.last_timing()
    assert set(t) == {"neighbors_scan_ms", "neighbors_rows_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())
    dev = measurer.measure_dense(as_tensor(lab), math.sqrt(50))
    assert all(np.array_equal(x, y) for x, y in zip(a, dev))             # CUDA tensors in equal numpy in
    m = int(lab.max())
    geom, objects, offsets, pairs = a
    for k in range(3):                                                   # an image alone equals its rows in the batch
        g, o, f, p = measurer.measure_dense(lab[k:k + 1].copy(), math.sqrt(50), max_label=m)
        lo, hi = offsets[k * m], offsets[(k + 1) * m]
        assert np.array_equal(g[0], geom[k]) and np.array_equal(o[0], objects[k]) and np.array_equal(f, offsets[k * m:(k + 1) * m + 1] - lo)
        assert np.array_equal(p, pairs[lo:hi])
    g, o, f, p = measurer.measure_dense(lab, math.sqrt(50), max_label=m + 100)           # a larger table: zeros behind the rows
    assert np.array_equal(g[:, :m], geom) and not g[:, m:].any() and np.array_equal(o[:, :m], objects) and not o[:, m:].any()
    assert np.array_equal(p, pairs)
    d = np.diff(f).reshape(3, m + 100)
    assert np.array_equal(d[:, :m], np.diff(offsets).reshape(3, m)) and not d[:, m:].any()
    t = measurer.measure_batch(lab, math.sqrt(50))
    i = int(np.flatnonzero(t.number_of_neighbors > 0)[0])
    nb, d2, nn = t.neighbors_of(i)
    assert len(nb) == t.number_of_neighbors[i] and nn.sum() == t.touching[i] and d2.min() == round(t.nearest_edge_distance[i] ** 2)
    with pytest.raises(ValueError):
        measurer.measure_dense(as_tensor(lab)[:, :, ::2], 3)


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (33, 65)
    name, lab = batch_of(shape, 5)[0]
    m = int(lab.max())
    want = NR.measure(lab, 25, m)
    for where, value in (((0, 0, 0), -1), ((1, 32, 64), -7), ((0, 0, 0), m + 1), ((1, 32, 64), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                                               # range-checked on the device: never an index or a key
        for arg in (bad, as_tensor(bad)):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_dense(arg, 5, max_label=m)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            same(measurer.measure_dense(lab, 5, max_label=m), want, "the next good call")
    neg = np.zeros_like(lab)
    neg[0, 2, 2] = -3
    with pytest.raises(L.CellScreenError):
        measurer.measure_batch(neg, 2)                                   # max_label=None on a batch without objects


def test_bad_arguments_with_a_handle():
    fresh = NB.NeighborMeasurer(0)
    lib, h = fresh._lib, fresh._handle
    lab = np.zeros((1, 8, 8), np.int32)
    lab[0, 2, 2], lab[0, 2, 3], lab[0, 5, 5] = 1, 2, 3
    out = np.zeros(4, np.int32)
    assert lib.cs_label_neighbors_pairs(h, out.ctypes.data, 4, 0) == -1 and b"no pair list" in lib.cs_last_error()        # no call yet
    geom, objects, offsets, n = np.zeros((1, 3, 3), np.int64), np.zeros((1, 3, 3), np.int32), np.zeros(4, np.int64), C.c_int64(-7)
    for max_d2, status in ((0, -1), (1025, -6)):                         # refused before any device work: nothing is written
        prm = L.CSNeighborsParams()
        prm.max_d2 = max_d2
        assert lib.cs_label_neighbors(h, lab.ctypes.data, 1, 8, 8, 0, 3, C.byref(prm), geom.ctypes.data, objects.ctypes.data, offsets.ctypes.data,
                                      0, C.byref(n)) == status
        assert n.value == -7 and not geom.any() and not offsets.any()
        assert lib.cs_label_neighbors_pairs(h, out.ctypes.data, 4, 0) == -1
    got = fresh.measure_dense(lab, 1)
    assert got[3].tolist() == [[2, 1, 1], [1, 1, 1]]
    out = np.full(8, -1, np.int32)
    assert lib.cs_label_neighbors_pairs(h, out.ctypes.data, 1, 0) == -1 and b"capacity 1" in lib.cs_last_error() and (out == -1).all()
    assert lib.cs_label_neighbors_pairs(h, out.ctypes.data, 2, 0) == 0 and out.tolist() == [2, 1, 1, 1, 1, 1, -1, -1]
    bad = lab.copy()
    bad[0, 0, 0] = -1
    with pytest.raises(L.CellScreenError):
        fresh.measure_dense(bad, 1, max_label=3)
    assert lib.cs_label_neighbors_pairs(h, out.ctypes.data, 8, 0) == -1                    # a failed call leaves no list
    fresh.close()


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


def test_segment_expand_neighbors_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = torch.from_numpy(imgs.view(np.int16)).to(torch.device("cuda", 0))
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev)                         # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)
    meas = NB.NeighborMeasurer(0, extractor=seg)
    t = meas.measure_batch(grown, distance=2)
    assert meas._pre is None                                             # the segmenter's handle did the work
    h_grown = grown.cpu().numpy()
    assert len(t) == int(n_labels.sum()) == 10
    got = meas.measure_dense(grown, 2)
    same(got, NR.measure(h_grown, 4), "one handle")
    d = NR.derive(*got)
    assert all(np.array_equal(getattr(t, k), v, equal_nan=True) for k, v in d.items()) and np.array_equal(t.pairs, got[3])
    assert (t.first_closest_label > 0).all() and (t.second_closest_label > 0).all() and np.isfinite(t.angle_between_neighbors).all()
    timing = meas.last_timing()
    assert all(np.isfinite(v) and v >= 0.0 for v in timing.values())
    seg.close()
