"""The per-object radial distribution and edge intensities on the device (cs_label_radial through cellscreen.radial) against the
CPU restatement of tests/radial_reference.py, which tests/test_radial_cpu.py holds to its slow form and to SciPy.

The records are integers, so every comparison is np.array_equal on the dense tables and on the depth plane: no tolerances, and the
rows of absent objects are compared too.

The column pass takes 16 rows per step and 256 columns per workgroup; the row pass a strip of 256 pixels with a halo of 127; a
lane of the bin pass owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows.  SHAPES crosses the 16 rows, the 64 rows
and the 256 columns one short, equal and one past, and has the single row, the single column and the single pixel.  Widths that
are no multiple of 4 take the scalar loads.  The tables in LDS have 1024 ring slots and 256 / 128 label slots: an image where every
pixel is its own label fills them and sends the rest to the global tables."""
import ctypes as C
import functools

import numpy as np
import pytest

import intensity_reference as IR
import radial_reference as RR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import intensity as IN
from cellscreen import neighbors as NB
from cellscreen import radial as RA
from cellscreen import segment as S
from cellscreen import shape as SH

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1)]
NAMES = ("geom", "center", "ring", "edge", "d2")


@pytest.fixture(scope="module")
def measurer():
    m = RA.RadialMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    a = a if a.flags.writeable else a.copy()             # batch_of's labels are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def batch_of(shape, seed):
    """(name, labels int32 [2,H,W]) per kind of content, the two images different."""
    out = []
    for (name, a), (_, b) in zip(IR.contents(shape, seed), IR.contents(shape, seed + 1)):
        lab = np.stack([a, b[::-1, ::-1] if name == "two pieces" else b])
        if name == "two pieces":
            lab[1][lab[1] > 0] = 2
            lab[1, shape[0] // 2, shape[1] // 2] = 5
        lab.flags.writeable = False
        out.append((name, lab))
    return out


def same(got, want, what=""):
    assert len(got) in (4, 5) and len(want) == 5
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype == {"center": np.int32, "d2": np.uint16}.get(name, np.int64) and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w), (name, what)


def some_centers(B, max_label, H, W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, H, (B, max_label)), rng.integers(0, W, (B, max_label))], axis=-1).astype(np.int32)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement_across_the_tiles(measurer, shape, dtype):
    seed = 7 * shape[0] + shape[1]
    H, W = shape
    for nc, bins in ((1, 4), (2, 1), (3, 16), (4, 4)):
        image = IR.noise((2,) + shape, nc, dtype, seed + nc)
        if nc == 1:
            image = image[..., 0]                        # [B,H,W] is one channel
        for name, lab in batch_of(shape, seed):
            want = RR.measure(image, lab, bins=bins)
            same(measurer.measure_dense(image, lab, bins=bins, want_d2=True), want, (name, nc))
            ex = ((lab + np.arange(W)[None, None, :] + np.arange(H)[None, :, None]) % 5 == 0).astype(np.int32) * 9
            same(measurer.measure_dense(image, lab, exclude=ex, bins=bins, want_d2=True), RR.measure(image, lab, ex, bins=bins), (name, nc, "exclude"))
            ctr = some_centers(2, int(want[0].shape[1]), H, W, seed)     # most of them outside their objects
            same(measurer.measure_dense(image, lab, bins=bins, centers=ctr), RR.measure(image, lab, bins=bins, centers=ctr), (name, nc, "centers"))
            t = measurer.measure_batch(image, lab, bins=bins)
            d = RR.derive(*want[:4])
            assert len(t) == len(d["label"]), name
            assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items()), name


def test_exclude_rings(measurer):
    shape = (70, 300)
    nuclei = np.stack([IR.disks(shape, 30, 1, radii=(2, 4)), IR.disks(shape, 30, 2, radii=(2, 4))])
    cells = np.stack([IR.disks(shape, 30, 1, radii=(5, 9)), IR.disks(shape, 30, 3, radii=(5, 9))])
    for nc, dtype in ((1, np.uint8), (3, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, 5 + nc)
        want = RR.measure(image, cells, nuclei)
        got = measurer.measure_dense(image, cells, exclude=nuclei, want_d2=True)
        same(got, want)
        assert not np.array_equal(got[0], RR.measure(image, cells)[0])    # the exclusion took pixels away
        big = (nuclei * 1000003).astype(np.int32) - (nuclei % 2) * 7      # any non-zero value counts, negative ones too
        same(measurer.measure_dense(image, cells, exclude=big), want)
        same(measurer.measure_dense(image, cells, exclude=np.zeros_like(cells)), RR.measure(image, cells))
        g, c, r, e, d2 = measurer.measure_dense(image, cells, exclude=cells, want_d2=True)     # swallowed whole: all zero
        assert not g.any() and not c.any() and not r.any() and not e.any() and not d2.any()
        t = measurer.measure_batch(image, cells, exclude=cells)
        assert len(t) == 0 and t.frac_at_d.shape == (0, 4, nc) and t.edge.shape == (0, nc, 4)
    # the centres of the nuclei for the cells: CellProfiler's use
    nuc = measurer.measure_dense(image, nuclei, max_label=int(cells.max()))[1]
    ctr = np.ascontiguousarray(nuc[:, :, :2])
    same(measurer.measure_dense(image, cells, centers=ctr, bins=6), RR.measure(image, cells, centers=ctr, bins=6))


def test_the_row_pass_reaches_through_the_halo_and_beyond_the_image(measurer):
    # the nearest foreign pixel lies in the neighbouring strip of 256 columns, on either side
    lab = np.zeros((1, 100, 600), np.int32)
    lab[0, 2:98, 150:420] = 1
    lab[0, 30, 262] = 0                                  # a hole in the second strip, 12 from (30, 250) in the first
    lab[0, 70, 250] = 2                                  # a foreign label in the first strip, 10 from (70, 260) in the second
    image = IR.noise((1, 100, 600), 2, np.uint16, 1)
    want = RR.measure(image, lab)
    assert want[4][0, 30, 250] == 144 and want[4][0, 70, 260] == 100
    same(measurer.measure_dense(image, lab, want_d2=True), want)
    # beyond each of the four image edges: an object that fills its image, and objects flush with one edge each
    for shape in ((9, 9), (40, 300), (100, 7)):
        full = np.ones((1,) + shape, np.int32)
        img = IR.noise((1,) + shape, 1, np.uint8, 2)
        want = RR.measure(img, full)
        H, W = shape
        assert want[4][0, H // 2, W // 2] == (min(H, W) // 2 + 1) ** 2 if min(H, W) % 2 else True
        same(measurer.measure_dense(img, full, want_d2=True), want, shape)
    lab = np.zeros((1, 80, 300), np.int32)
    lab[0, :30, 100:160] = 1                             # top
    lab[0, 50:, 20:90] = 2                               # bottom
    lab[0, 20:60, :25] = 3                               # left
    lab[0, 35:70, 270:] = 4                              # right
    img = IR.noise((1, 80, 300), 3, np.uint8, 3)
    same(measurer.measure_dense(img, lab, want_d2=True), RR.measure(img, lab))
    # labels that touch with no background between them, side by side and one above the other
    lab = np.zeros((1, 70, 300), np.int32)
    lab[0, 5:65, 10:140] = 1
    lab[0, 5:65, 140:290] = 2
    lab[0, 35:65, 60:200] = 3
    same(measurer.measure_dense(img[:, :70], lab, want_d2=True, bins=8), RR.measure(img[:, :70], lab, bins=8))
    assert measurer.measure_dense(img[:, :70], lab, want_d2=True)[4].min() >= 0 and (measurer.measure_dense(img[:, :70], lab, want_d2=True)[4][0, 5:65, 10:290] > 0).all()


def test_the_depth_limit(measurer):
    side = 253                                           # the centre is 127 from the first position outside: exactly the limit
    lab = np.ones((1, side, side), np.int32)
    image = IR.noise((1, side, side), 1, np.uint8, 4)
    want = RR.measure(image, lab)
    assert want[1][0, 0].tolist() == [126, 126, RA.MAX_D2, 4 * side - 4] and RA.RadialMeasurer.MAX_D2 == 127 * 127
    same(measurer.measure_dense(image, lab, want_d2=True), want)
    side = 254                                           # four equally deep pixels, still at the limit
    lab = np.ones((1, side, side), np.int32)
    image = IR.noise((1, side, side), 1, np.uint8, 4)
    r, c = np.mgrid[0:side, 0:side]
    got = measurer.measure_dense(image, lab, want_d2=True)
    assert got[1][0, 0].tolist() == [126, 126, RA.MAX_D2, 4 * side - 4]
    assert np.array_equal(got[4][0], (np.minimum(np.minimum(r, c), np.minimum(side - 1 - r, side - 1 - c)) + 1) ** 2)
    side = 255                                           # one deeper
    lab = np.ones((1, side, side), np.int32)
    image = IR.noise((1, side, side), 1, np.uint8, 4)
    for args in ((image, lab), (as_tensor(image), as_tensor(lab))):
        with pytest.raises(L.CellScreenError) as ei:
            measurer.measure_dense(*args)
        assert ei.value.status == -6 and "deeper than 127 px" in str(ei.value)
    with pytest.raises(RR.TooDeep):
        RR.measure(image, lab)
    lab[0, 127, 127] = 0                                 # the next call on the same handle succeeds
    same(measurer.measure_dense(image, lab, want_d2=True), RR.measure(image, lab))


@pytest.mark.parametrize("nc", [1, 4])
@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_every_pixel_its_own_label_overflows_the_tables_in_lds(measurer, shape, nc):
    H, W = shape
    n = H * W
    lab = np.stack([np.arange(1, n + 1, dtype=np.int32).reshape(shape), np.arange(n, 0, -1, dtype=np.int32).reshape(shape)])
    rr, cc = (x.reshape(-1) for x in np.mgrid[0:H, 0:W])
    for dtype, bins in ((np.uint16, 4), (np.uint8, 16)):
        image = IR.noise((2,) + shape, nc, dtype, H + nc)
        g, c, r, e, d2 = measurer.measure_dense(image, lab, bins=bins, want_d2=True)
        v = image.reshape(2, n, nc).astype(np.int64)
        v[1] = v[1, ::-1]                                # row m of the second image is pixel n - 1 - m
        assert (d2 == 1).all() and (g[:, :, 0] == 1).all() and np.array_equal(g[0, :, 1], rr) and np.array_equal(g[1, :, 2], cc[::-1])
        assert np.array_equal(c[0], np.stack([rr, cc, np.ones(n, np.int64), np.ones(n, np.int64)], axis=-1))
        assert (r[:, :, 0, 0, 0] == 1).all() and np.array_equal(r[:, :, 0, 0, 1:], v) and r.sum() == n * 2 + v.sum()   # n = 1, ring 0, wedge 0
        assert np.array_equal(e[..., 0], v) and np.array_equal(e[..., 1], v * v) and np.array_equal(e[..., 2], v) and np.array_equal(e[..., 3], v)
    ex = (lab % 3 == 0).astype(np.int32)
    got = measurer.measure_dense(image, lab, exclude=ex, bins=bins)
    keep = (ex.reshape(2, n) == 0)
    keep[1] = keep[1, ::-1]
    assert np.array_equal(got[0][:, :, 0], keep.astype(np.int64)) and np.array_equal(got[3][..., 0], v * keep[..., None])


def test_a_tie_for_the_deepest_pixel_goes_to_the_smaller_raster_index(measurer):
    lab = np.zeros((1, 40, 600), np.int32)
    lab[0, 3:7, 100:500] = 1                             # deepest: rows 4 and 5, columns 101..498, across two strip borders
    lab[0, 20:24, 300:304] = 2                           # two pieces equally deep: the later rows first in the columns
    lab[0, 12:16, 500:504] = 2
    lab[0, 30:33, 252:259] = 3                           # deepest in row 31 on both sides of column 256
    image = IR.noise((1, 40, 600), 1, np.uint8, 6)
    want = RR.measure(image, lab)
    got = measurer.measure_dense(image, lab, want_d2=True)
    same(got, want)
    assert got[1][0, :, :3].tolist() == [[4, 101, 4], [13, 501, 4], [31, 253, 4]]
    same(measurer.measure_dense(as_tensor(image), as_tensor(lab), want_d2=True), want)


def test_geometry_and_edge_counts_agree_with_the_other_label_tools(measurer):
    shape = (70, 300)
    lab = np.stack([IR.disks(shape, 30, k) for k in (1, 2)])
    image = IR.noise((2,) + shape, 2, np.uint16, 8)
    ex = np.stack([IR.disks(shape, 30, k, radii=(1, 2)) for k in (5, 3)])
    m = int(lab.max())
    for e in (None, ex):
        g, c, r, ed = measurer.measure_dense(image, lab, exclude=e, max_label=m)
        geom = IN.IntensityMeasurer(0, extractor=measurer).measure_dense(image, lab, exclude=e, max_label=m)[0]
        assert np.array_equal(geom, g)                   # cs_label_intensity's geom, bit for bit
        assert np.array_equal(r[..., 0].sum(axis=(2, 3)), g[..., 0])
    objects = NB.NeighborMeasurer(0, extractor=measurer).measure_dense(lab, 1, max_label=m)[1]
    assert np.array_equal(objects[..., 0], measurer.measure_dense(image, lab, max_label=m)[1][..., 3])   # cs_label_neighbors' border pixels
    # cs_label_shape's perimeter classes hold every border pixel of a rectangle with sides >= 3
    rect = np.zeros((1, 70, 300), np.int32)
    for k, (r0, c0, h, w) in enumerate(((0, 0, 3, 3), (10, 250, 20, 40), (40, 5, 30, 200), (5, 100, 3, 120), (34, 296, 30, 4)), 1):
        rect[0, r0:r0 + h, c0:c0 + w] = k
    for e in (None, (rect == 3).astype(np.int32) * (np.arange(300)[None, None, :] == 77)):
        perim = SH.ShapeMeasurer(0, extractor=measurer).measure_dense(rect, exclude=e, hull=False)[3]
        if e is None:
            assert np.array_equal(perim.sum(axis=-1), measurer.measure_dense(image[:1], rect)[1][..., 3])
        want = RR.measure(image[:1], rect, e)
        same(measurer.measure_dense(image[:1], rect, exclude=e), want)
        assert want[1][0, :, 3].tolist()[:2] == [8, 2 * 20 + 2 * 40 - 4]


def test_repeatability_batches_and_input_kinds(measurer):
    import torch
    shape = (70, 300)
    lab = np.stack([IR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([IR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    m = int(lab.max())
    for nc, dtype in ((3, np.uint16), (4, np.uint8), (1, np.uint16)):
        image = IR.noise((3,) + shape, nc, dtype, 12)
        a = measurer.measure_dense(image, lab, exclude=ex, want_d2=True)
        b = measurer.measure_dense(image, lab, exclude=ex, want_d2=True)
        same(a, RR.measure(image, lab, ex))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))      # bit-identical run to run
        t = measurer.last_timing()
        assert set(t) == {"radial_columns_ms", "radial_rows_ms", "radial_bins_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        for k in range(3):                               # an image alone equals its rows in the batch
            one = measurer.measure_dense(image[k:k + 1].copy(), lab[k:k + 1].copy(), exclude=ex[k:k + 1].copy(), max_label=m, want_d2=True)
            assert all(np.array_equal(x[0], y[k]) for x, y in zip(one, a))
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex), want_d2=True), a)      # CUDA tensors in
        if dtype == np.uint16:                           # uint16 as int16 views, and as uint16 tensors
            assert as_tensor(image).dtype == torch.int16
            same(measurer.measure_dense(as_tensor(image).view(torch.uint16), as_tensor(lab)), RR.measure(image, lab))
    g, c, r, e = measurer.measure_dense(image, lab, max_label=m + 100)    # a larger table: the same rows, zeros behind them
    assert np.array_equal(r[:, :m], measurer.measure_dense(image, lab)[2]) and not g[:, m:].any() and not c[:, m:].any() and not r[:, m:].any() and not e[:, m:].any()
    with pytest.raises(TypeError):
        measurer.measure_dense(image, as_tensor(lab))


def test_tables_left_on_the_device_equal_the_host_tables(measurer):
    import torch
    shape = (40, 264)
    lab = batch_of(shape, 6)[0][1]
    image = IR.noise((2,) + shape, 3, np.uint16, 11)
    m, bins = int(lab.max()), 5
    want = measurer.measure_dense(image, lab, bins=bins, want_d2=True)
    same(want, RR.measure(image, lab, bins=bins))
    dev = torch.device("cuda", 0)
    outs = [torch.full(w.shape, -5, dtype={np.int64: torch.int64, np.int32: torch.int32, np.uint16: torch.int16}[w.dtype.type], device=dev)
            for w in want]
    t_img, t_lab = as_tensor(image), as_tensor(lab)
    prm = RA.radial_params(bins)
    torch.cuda.synchronize()
    L.check(measurer._lib.cs_label_radial(measurer._handle, t_img.data_ptr(), 1, 3, t_lab.data_ptr(), None, 2, shape[0], shape[1], L.CS_MEM_DEVICE, m,
                                          C.byref(prm), None, *(o.data_ptr() for o in outs), L.CS_MEM_DEVICE))
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy().view(w.dtype), w)


def test_unaligned_tensor_views_take_the_scalar_loads(measurer):
    import torch
    shape = (40, 264)                                    # a multiple of 4: only the pointers decide
    lab = batch_of(shape, 4)[0][1]
    ex = (lab % 3 == 1).astype(np.int32)
    dev = torch.device("cuda", 0)

    def shifted(a, by):
        """a on the device at `by` elements past an allocation's start"""
        flat = torch.empty(a.size + by, dtype=as_tensor(a[:1]).dtype, device=dev)
        view = flat[by:].view(a.shape)
        view.copy_(as_tensor(a))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view

    for nc, dtype in ((3, np.uint8), (2, np.uint8), (4, np.uint16), (1, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, 10)
        want = RR.measure(image, lab, ex)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex)), want)           # all aligned: wide loads
        same(measurer.measure_dense(shifted(image, 1), as_tensor(lab), exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), shifted(lab, 1), exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=shifted(ex, 3)), want)


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    lab = batch_of(shape, 5)[0][1]
    image = IR.noise((2,) + shape, 3, np.uint8, 1)
    m = int(lab.max())
    want = RR.measure(image, lab, max_label=m)
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 0, 0), m + 1), ((1, 16, 256), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                               # range-checked on the device: never an index or a key
        for args in ((image, bad), (as_tensor(image), as_tensor(bad))):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_dense(*args, max_label=m)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            with pytest.raises(L.CellScreenError):      # whatever exclude holds there
                measurer.measure_dense(*args, exclude=(np.ones_like(lab) if isinstance(args[1], np.ndarray) else as_tensor(np.ones_like(lab))),
                                       max_label=m)
            same(measurer.measure_dense(image, lab, max_label=m), want)
    neg = np.zeros_like(lab)
    neg[0, 2, 2] = -3
    with pytest.raises(L.CellScreenError):
        measurer.measure_batch(image, neg)               # max_label=None on a batch without objects


def test_bad_arguments_are_refused_before_the_device_is_touched(measurer):
    lib, h = measurer._lib, measurer._handle            # a live handle: the refusals are the arguments' own
    zeros = np.zeros(64, np.int32)
    outs = [np.empty(4096, dt) for dt in (np.int64, np.int32, np.int64, np.int64)]
    prm = RA.radial_params(4)

    def status(channels=1, bins=4, reserved=0, B=1, max_label=1, centers=None):
        prm.bins, prm.reserved = bins, reserved
        for o in outs:
            o[:] = -5
        ctr = None if centers is None else np.asarray(centers, np.int32)
        rc = lib.cs_label_radial(h, zeros.ctypes.data, 0, channels, zeros.ctypes.data, None, B, 2, 2, 0, max_label, C.byref(prm),
                                 None if ctr is None else ctr.ctypes.data, *(o.ctypes.data for o in outs), None, 0)
        assert rc == 0 or all((o == -5).all() for o in outs)             # a refused call wrote nothing
        return rc, lib.cs_last_error().decode()

    assert status()[0] == 0
    assert status(channels=0)[0] == -1 and status(channels=5)[0] == -6 and "at most 4" in status(channels=5)[1]
    assert status(bins=0)[0] == -1 and status(bins=17)[0] == -6 and status(reserved=1)[0] == -1 and status(bins=16)[0] == 0
    assert status(centers=[[1, 1]])[0] == 0
    for bad in ([[2, 0]], [[0, 2]], [[-1, 0]], [[0, -1]]):
        rc, text = status(centers=bad)
        assert rc == -1 and "outside the image" in text
    assert status(max_label=2, centers=[[0, 0], [0, 5]])[0] == -1        # the row of an absent object too
    lab = np.ones((1, 4, 4), np.int32)
    image = IR.noise((1, 4, 4), 2, np.uint8, 1)
    for kw, exc in ((dict(bins=0), ValueError), (dict(bins=17), ValueError), (dict(bins=4.0), TypeError), (dict(bins=True), TypeError),
                    (dict(centers=np.zeros((1, 1, 2), np.int64)), TypeError), (dict(centers=[[[0, 0]]]), TypeError),
                    (dict(centers=np.zeros((1, 2, 2), np.int32)), ValueError), (dict(centers=np.full((1, 1, 2), 4, np.int32)), ValueError),
                    (dict(centers=np.full((1, 1, 2), -1, np.int32)), ValueError)):
        with pytest.raises(exc):
            measurer.measure_dense(image, lab, **kw)
    with pytest.raises(ValueError):
        measurer.measure_dense(np.zeros((1, 4, 4, 5), np.uint8), lab)
    with pytest.raises(ValueError, match="split the batch"):
        measurer.measure_dense(np.zeros((1, 1, 1, 4), np.uint8), np.zeros((1, 1, 1), np.int32), max_label=1 << 18, bins=16)
    same(measurer.measure_dense(image, lab, want_d2=True), RR.measure(image, lab))     # and the measurer works


def nuclei_scene():
    """uint16 [2,96,128,2]: five bright blobs per image on a noisy background in channel 0; channel 1 is brightest at their rims."""
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.empty((2, H, W, 2), np.uint16)
    for b in range(2):
        f = 300.0 + rng.normal(0.0, 10.0, (H, W))
        rim = 200.0 + rng.normal(0.0, 5.0, (H, W))
        for y, x, r in ((24, 25, 9), (30, 80, 12), (70, 40, 10), (70, 100, 7 + 4 * b), (50, 62, 5)):
            d = np.sqrt((yy - y) ** 2 + (xx - x) ** 2)
            f += 4000.0 * np.exp(-((d * d / (2.0 * (r / 1.6) ** 2)) ** 2))
            rim += 3000.0 * np.exp(-((d - (r + 4)) ** 2) / 4.0)
        imgs[b, :, :, 0] = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
        imgs[b, :, :, 1] = np.clip(np.rint(rim), 0, 65535).astype(np.uint16)
    return imgs


def test_segment_expand_measure_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = as_tensor(imgs)
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)                    # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)          # left on the device too: no host copy in between
    meas = RA.RadialMeasurer(0, extractor=seg)
    whole = meas.measure_batch(dev, grown)
    ring = meas.measure_batch(dev, grown, exclude=labels)
    nuc = meas.measure_batch(dev, labels)
    assert meas._pre is None                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(nuc) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (whole, (h_grown, None)), (nuc, (h_lab, None))):
        d = RR.derive(*RR.measure(imgs, lab, ex)[:4])
        assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items())
    assert np.array_equal(ring.label, nuc.label) and np.array_equal(ring.area + nuc.area, whole.area)
    assert (whole.mean_frac[:, 3, 1] > 1.2).all() and (whole.mean_frac[:, 0, 1] < 0.8).all()       # channel 1 sits at the rim
    assert (whole.mean_frac[:, 0, 0] > 1.2).all() and (whole.mean_frac[:, 3, 0] < 0.8).all()       # channel 0 in the middle
    t = meas.last_timing()
    assert len(t) == 3 and all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
