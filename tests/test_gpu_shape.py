"""The per-object shape records on the device (cs_label_shape through cellscreen.shape) against the CPU restatement of
tests/shape_reference.py, which tests/test_shape_cpu.py holds to its slow form, to SciPy and to closed forms.

Every record is an integer: np.array_equal on the dense tables, the rows of absent objects included.

A lane of the moments pass owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows; SHAPES crosses the 16 rows, the 64 rows
and the 256 columns one short, equal and one past, and has the single row, the single column and the single pixel.  Widths that are
no multiple of 4 take the scalar path.  A tile's table in LDS has 256 slots: an image where every pixel is its own label overflows
it.  The outline pass walks a box in strips through a bitmap of 64-bit words with a halo of 2 rows and 3 columns: the boxes here are
1 to 4096 wide, so that a row of the bitmap has 1 to 65 words and a box one or many strips, and touch all four sides of the image.
Boxes above 256 rows go through the second launch."""
import functools

import numpy as np
import pytest

import shape_reference as SR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import segment as S
from cellscreen import shape as SH

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1)]
NAMES = ("moments", "box", "quads", "perim", "hull")
DTYPES = (np.int64, np.int32, np.int32, np.int32, np.int64)


@pytest.fixture(scope="module")
def measurer():
    m = SH.ShapeMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def batch_of(shape, seed):
    """(name, labels int32 [2,H,W], the restatement's records with the hull) per kind of content, the two images different."""
    out = []
    for (name, a), (_, b) in zip(SR.contents(shape, seed), SR.contents(shape, seed + 1)):
        lab = np.stack([a, b[::-1, ::-1] if name == "two pieces" else b])
        if name == "two pieces":
            lab[1][lab[1] > 0] = 2
            lab[1, shape[0] // 2, shape[1] // 2] = 5
        lab.flags.writeable = False
        out.append((name, lab, SR.measure(lab)))
    return out


def same(got, want, what=""):
    """device records against reference records; a reference with the hull serves a device call without it"""
    assert len(got) == len(want) == 5, what
    for k in range(5):
        g, w = got[k], want[k]
        if g is None:
            assert k == 4, what
            continue
        assert w is not None and g.dtype == w.dtype == DTYPES[k] and g.shape == w.shape, (what, NAMES[k])
        assert np.array_equal(g, w), (what, NAMES[k])


def check(measurer, lab, exclude=None, max_label=None, hull=True, what=""):
    """measure_dense against the restatement; returns the device's records"""
    got = measurer.measure_dense(lab, exclude, max_label, hull)
    same(got, SR.measure(lab, exclude, max_label, hull), what)
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_records_equal_the_restatement_across_the_tiles(measurer, shape):
    seed = 7 * shape[0] + shape[1]
    for name, lab, want in batch_of(shape, seed):
        for hull in (True, False):
            got = measurer.measure_dense(lab, hull=hull)
            assert (got[4] is None) == (not hull)
            same(got, want, f"{shape} {name} hull={hull}")
    t = measurer.measure_batch(lab)
    d = SR.derive(*want)
    assert len(t) == len(d["label"]) and all(np.array_equal(getattr(t, k), v, equal_nan=True) for k, v in d.items())
    t = measurer.measure_batch(lab, hull=False)
    assert t.convex_area is None and t.hull is None and np.array_equal(t.perimeter, d["perimeter"])


def test_halos(measurer):
    # one object fills the image: its quads sit at -1 and at H and W, its border pixels on all four sides
    for shape in ((20, 30), (1, 70), (70, 1), (64, 256), (67, 130), (300, 5)):
        H, W = shape
        m, bx, q, p, h = check(measurer, np.ones((1,) + shape, np.int32), what=f"full {shape}")
        if H >= 3 and W >= 3:
            want = SR.rectangle_records(0, 0, H, W)
            assert [m[0, 0].tolist(), bx[0, 0].tolist(), q[0, 0].tolist(), p[0, 0].tolist(), h[0, 0].tolist()] == [list(x) for x in want]
    # two objects that touch along a straight edge: each is background to the other, so each is a rectangle on its own
    lab = np.ones((1, 24, 40), np.int32)
    lab[0, :, 20:] = 2
    m, bx, q, p, h = check(measurer, lab, what="touching")
    for k, c0 in ((0, 0), (1, 20)):
        want = SR.rectangle_records(0, c0, 24, 20)
        assert [m[0, k].tolist(), bx[0, k].tolist(), q[0, k].tolist(), p[0, k].tolist(), h[0, k].tolist()] == [list(x) for x in want]
    lab = np.ones((1, 30, 24), np.int32)                                 # the same along a row
    lab[0, 13:] = 7
    check(measurer, lab, what="touching rows")
    ring = np.zeros((2, 40, 300), np.int32)                              # a one-pixel-wide ring, at the border and inside
    ring[0, 0, :] = ring[0, -1, :] = ring[0, :, 0] = ring[0, :, -1] = 1
    ring[1, 5:30, 7:290] = 2
    ring[1, 6:29, 8:289] = 0
    m, bx, q, p, h = check(measurer, ring, what="ring")
    t = SH.shape_table(m, bx, q, p, h)
    assert t.euler_number.tolist() == [0, 0] and t.perimeter.tolist() == [2 * (40 + 300) - 4, 2 * (25 + 283) - 4]
    board = (np.add.outer(np.arange(67), np.arange(131)) % 2 == 0).astype(np.int32)[None] * 3      # most border pixels, diagonal quads
    m, bx, q, p, h = check(measurer, board, what="checkerboard")
    n = int(board.sum()) // 3
    assert q[0, 2, 6] + q[0, 2, 9] == 66 * 130 and q[0, 2, 15] == 0 and q[0, 2, 7] == 0 and m[0, 2, 0] == n
    t = SH.shape_table(m, bx, q, p, h)
    holes = int((board[0, 1:-1, 1:-1] == 0).sum())                       # one 8-connected piece; every inner zero is a 4-connected hole
    assert t.euler_number_4[0] == n and t.euler_number[0] == 1 - holes and holes == 4192


def test_more_labels_in_a_tile_than_the_table_has_slots(measurer):
    shape = (64, 256)                                                    # every pixel its own label
    lab = np.arange(1, 64 * 256 + 1, dtype=np.int32).reshape((1,) + shape)
    m, bx, q, p, h = measurer.measure_dense(lab)
    r, c = (x.ravel().astype(np.int64) for x in np.indices(shape))
    want = np.stack([np.ones_like(r), r, c, r * r, r * c, c * c, r ** 3, r * r * c, r * c * c, c ** 3], axis=1)
    assert np.array_equal(m[0], want) and np.array_equal(bx[0], np.stack([r, c, r + 1, c + 1], axis=1))
    single = SR.rectangle_records(0, 0, 1, 1)
    assert (q[0] == np.array(single[2])).all() and not p.any() and (h[0] == np.array(single[4])).all() and single[4] == [1, 4, 2, 2]
    t = SH.shape_table(m, bx, q, p, h)
    assert len(t) == 64 * 256 and (t.euler_number == 1).all() and (t.perimeter == 0).all() and np.isnan(t.form_factor).all()


def test_one_label_over_a_4096_plane(measurer):
    side = 4096
    lab = np.ones((1, side, side), np.int32)
    m, bx, q, p, h = measurer.measure_dense(lab)
    want = SR.rectangle_records(0, 0, side, side)                        # closed forms: power sums, an octagon of 8 vertices
    assert m[0, 0].tolist() == want[0] and max(want[0]) < 2 ** 59 and want[0][6] == (side * (side - 1) // 2) ** 2 * side
    assert bx[0, 0].tolist() == [0, 0, side, side] and q[0, 0].tolist() == want[2] and q[0, 0, 15] == (side - 1) ** 2
    assert p[0, 0].tolist() == [4 * side - 4, 0, 0]
    assert h[0, 0].tolist() == want[4] and want[4] == [side * side, 4 * side * side + (2 * side - 2) ** 2, 2 * side * (2 * side - 2), (2 * side - 2) ** 2]
    t = SH.shape_table(m, bx, q, p, h)
    assert t.feret_diameter_min[0] == side and t.solidity[0] == 1.0 and t.euler_number[0] == 1 and t.orientation[0] == 0.0
    got = measurer.measure_dense(lab, hull=False)
    assert got[4] is None and all(np.array_equal(x, y) for x, y in zip(got[:4], (m, bx, q, p)))


def test_tall_and_wide_boxes_through_the_second_launch(measurer):
    # boxes of 257 to 700 rows beside small ones in one image: both launches serve it; diagonal bands make long hull chains
    H, W = 700, 520
    rr, cc = np.indices((H, W))
    lab = np.zeros((1, H, W), np.int32)
    lab[0][np.abs(rr - cc) < 9] = 1                                      # a diagonal band, 520 rows
    lab[0][(rr - 350) ** 2 * 4 + (cc - 400) ** 2 * 49 < 340 ** 2 * 4] = 2        # a tall ellipse, about 680 rows
    lab[0][(rr - 600) ** 2 + (cc - 60) ** 2 < 40 ** 2] = 3              # a disk of 79 rows
    lab[0, 257:514, 500:503] = 4                                         # 257 rows: the first of the second launch
    lab[0, 0:256, 510:512] = 5                                           # 256 rows: the last of the first
    ex = ((rr + cc) % 11 == 0).astype(np.int32)[None]
    check(measurer, lab, what="tall boxes")
    check(measurer, lab, exclude=ex, what="tall boxes, excluded diagonals")


def test_scalar_path_for_odd_widths_and_unaligned_tensor_views(measurer):
    import torch
    for shape in ((33, 258), (20, 7), (9, 301)):                         # widths that are no multiple of 4
        lab = batch_of(shape, 3)[0][1]
        check(measurer, lab, exclude=(lab % 2).astype(np.int32), what=f"{shape}")
    shape = (40, 264)                                                    # a multiple of 4: only the pointers decide
    lab = batch_of(shape, 4)[0][1]
    ex = (lab % 3 == 1).astype(np.int32)
    dev = torch.device("cuda", 0)

    def shifted(a, by):
        """a on the device at `by` elements past an allocation's start"""
        flat = torch.empty(a.size + by, dtype=torch.int32, device=dev)
        view = flat[by:].view(a.shape)
        view.copy_(as_tensor(a))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view

    want, plain = SR.measure(lab, ex), batch_of(shape, 4)[0][2]
    same(measurer.measure_dense(as_tensor(lab), as_tensor(ex)), want, "aligned")
    same(measurer.measure_dense(shifted(lab, 1), as_tensor(ex)), want, "labels shifted")
    same(measurer.measure_dense(as_tensor(lab), shifted(ex, 3)), want, "exclude shifted")
    same(measurer.measure_dense(shifted(lab, 2), shifted(ex, 1)), want, "both shifted")
    same(measurer.measure_dense(shifted(lab, 3)), plain, "labels shifted, no exclude")


def test_exclude(measurer):
    shape = (70, 300)
    nuclei = np.stack([SR.disks(shape, 30, 1, radii=(2, 4)), SR.disks(shape, 30, 2, radii=(2, 4))])
    cells = np.stack([SR.disks(shape, 30, 1, radii=(5, 9)), SR.disks(shape, 30, 3, radii=(5, 9))])
    ring = check(measurer, cells, exclude=nuclei, what="rings")          # cells with their nuclei excluded
    whole = check(measurer, cells, what="whole cells")
    assert not np.array_equal(ring[0], whole[0]) and (ring[0][..., 0] <= whole[0][..., 0]).all()
    big = np.where(nuclei % 2 == 1, -nuclei, nuclei * 1000003).astype(np.int32)       # any non-zero value excludes, negative ones too
    assert (big < 0).any() and (big > 0).any()
    same(measurer.measure_dense(cells, exclude=big), ring, "any non-zero value")
    same(measurer.measure_dense(cells, exclude=np.zeros_like(cells)), whole, "an all-zero exclude")
    got = measurer.measure_dense(cells, exclude=cells)                   # swallowed whole: all zero, absent from the table
    assert all(not x.any() for x in got) and got[0].shape == whole[0].shape
    t = measurer.measure_batch(cells, exclude=cells)
    assert len(t) == 0 and t.hu.shape == (0, 7) and t.hull.shape == (0, 4)
    half = cells.copy()
    half[cells == 3] = 0
    t = measurer.measure_batch(cells, exclude=(cells == 3).astype(np.int32) * -2, max_label=int(cells.max()))
    assert 3 not in t.label.tolist() and len(t) == len(measurer.measure_batch(half))
    lab = np.ones((1, 5, 5), np.int32)                                   # one excluded pixel inside a 5 x 5 object: a hole
    ex = np.zeros((1, 5, 5), np.int32)
    ex[0, 2, 2] = -1
    m, bx, q, p, h = check(measurer, lab, exclude=ex, what="one excluded pixel")
    t = SH.shape_table(m, bx, q, p, h)
    assert t.area.tolist() == [24] and t.euler_number.tolist() == [0] and t.euler_number_4.tolist() == [0] and t.convex_area.tolist() == [25]


def test_input_kinds_repeatability_and_batch_independence(measurer):
    shape = (70, 300)
    lab = np.stack([SR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([SR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    a = check(measurer, lab, exclude=ex, what="numpy in")
    b = measurer.measure_dense(lab, exclude=ex)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))               # bit-identical run to run
    t = measurer.last_timing()
    assert set(t) == {"shape_moments_ms", "shape_outline_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())
    dev = measurer.measure_dense(as_tensor(lab), exclude=as_tensor(ex))
    assert all(np.array_equal(x, y) for x, y in zip(a, dev))             # CUDA tensors in equal numpy in
    check(measurer, lab, what="no exclude")
    m = int(lab.max())
    for k in range(3):                                                   # an image alone equals its rows in the batch
        got = measurer.measure_dense(lab[k:k + 1].copy(), exclude=ex[k:k + 1].copy(), max_label=m)
        assert all(np.array_equal(g[0], x[k]) for g, x in zip(got, a))
    got = measurer.measure_dense(lab, exclude=ex, max_label=m + 100)     # a larger table: zeros behind the rows
    assert all(np.array_equal(g[:, :m], w) and not g[:, m:].any() for g, w in zip(got, a))
    with pytest.raises(TypeError):
        measurer.measure_dense(lab, exclude=as_tensor(ex))
    with pytest.raises(ValueError):
        measurer.measure_dense(as_tensor(lab)[:, :, ::2])


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    name, lab, want = batch_of(shape, 5)[0]
    m = int(lab.max())
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 9, 255), m + 1), ((1, 3, 100), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                                               # range-checked on the device: never an index
        for arg, ones in ((bad, np.ones_like(lab)), (as_tensor(bad), as_tensor(np.ones_like(lab)))):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_dense(arg, max_label=m)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            with pytest.raises(L.CellScreenError) as ei:                 # whatever exclude holds there
                measurer.measure_dense(arg, exclude=ones, max_label=m, hull=False)
            assert ei.value.status == -1
            same(measurer.measure_dense(lab, max_label=m), want, "the next good call")
    neg = np.zeros_like(lab)
    neg[0, 2, 2] = -3
    with pytest.raises(L.CellScreenError):
        measurer.measure_batch(neg)                                      # max_label=None on a batch without objects


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


def test_segment_expand_shape_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = torch.from_numpy(imgs.view(np.int16)).to(torch.device("cuda", 0))
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev)                         # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)
    meas = SH.ShapeMeasurer(0, extractor=seg)
    ring = meas.measure_batch(grown, exclude=labels)
    nuc = meas.measure_batch(labels)
    assert meas._pre is None                                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(nuc) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (nuc, (h_lab, None))):
        got = meas.measure_dense(as_tensor(lab), exclude=None if ex is None else as_tensor(ex))
        same(got, SR.measure(lab, ex), "one handle")
        d = SR.derive(*got)
        assert all(np.array_equal(getattr(t, k), v, equal_nan=True) for k, v in d.items())
    assert np.array_equal(ring.label, nuc.label) and np.array_equal(ring.image, nuc.image)
    assert (nuc.euler_number == 1).all() and (ring.euler_number == 0).all()
    assert (ring.solidity < nuc.solidity).all()
    t = meas.last_timing()
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
