"""The per-object order statistics on the device (cs_label_quantiles through cellscreen.quantile) against the CPU restatement of
tests/quantile_reference.py, which tests/test_quantile_cpu.py holds to numpy and SciPy.

The tables are integers, so every comparison is np.array_equal on the dense tables: no tolerances, and the rows of absent
objects are compared too.

A lane of the two walks owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows; SHAPES crosses the 16 rows, the 64 rows
and the 256 columns one short, equal and one past, and has the single row, the single column and the single pixel.  Widths that
are no multiple of 4 take the scalar path.  A tile's table in LDS has 1024 slots: an image where every pixel is its own label
fills it and sends the rest to the per-pixel reservation.  The selection reads a segment 16 bytes at a time between its unaligned
ends, 2048 values per step of the workgroup: the objects here have 1 to 2^24 pixels."""
import functools

import numpy as np
import pytest

import quantile_reference as QR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import intensity as IN
from cellscreen import quantile as QN
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1)]
Q = QR.QUANTILES                                                         # 1/4, 1/2, 3/4, 1/100, 99/100


@pytest.fixture(scope="module")
def measurer():
    m = QN.QuantileMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def batch_of(shape, seed):
    """(name, labels int32 [2,H,W]) per kind of content, the two images different."""
    out = []
    for (name, a), (_, b) in zip(QR.contents(shape, seed), QR.contents(shape, seed + 1)):
        lab = np.stack([a, b[::-1, ::-1] if name == "two pieces" else b])
        if name == "two pieces":
            lab[1][lab[1] > 0] = 2
            lab[1, shape[0] // 2, shape[1] // 2] = 5
        lab.flags.writeable = False
        out.append((name, lab))
    return out


def same(got, want):
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == w.dtype == np.int32 and g.shape == w.shape
            assert np.array_equal(g, w)


def one_object(values, shape=None):
    """(image [1,H,W], labels): one label over the whole plane of `values`"""
    v = np.asarray(values)
    v = v.reshape((1,) + (shape or (1, v.size)))
    return np.ascontiguousarray(v), np.ones(v.shape, np.int32)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement_across_the_tiles(measurer, shape, dtype):
    seed = 7 * shape[0] + shape[1]
    for nc in (1, 3, 4):
        image = QR.noise((2,) + shape, nc, dtype, seed + nc)
        for name, lab in batch_of(shape, seed):
            want = QR.measure(image, lab, Q, True)
            same(measurer.measure_dense(image, lab, Q, mad=True), want)
    t = measurer.measure_batch(image, lab, Q, mad=True)
    d = QR.derive(*want, Q)
    assert len(t) == len(d["label"]) and all(np.array_equal(getattr(t, k), v) for k, v in d.items())
    one = QR.noise((2,) + shape, 1, dtype, seed)[..., 0]                 # [B,H,W]: one channel, and no MAD
    got = measurer.measure_dense(one, batch_of(shape, seed)[0][1], Q)
    assert got[2] is None
    same(got, QR.measure(one, batch_of(shape, seed)[0][1], Q))


@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_every_pixel_its_own_label_overflows_the_table_in_lds(measurer, shape):
    H, W = shape
    lab = np.stack([np.arange(1, H * W + 1, dtype=np.int32).reshape(shape), np.arange(H * W, 0, -1, dtype=np.int32).reshape(shape)])
    for nc, dtype in ((1, np.uint16), (3, np.uint8), (4, np.uint16)):
        image = QR.noise((2,) + shape, nc, dtype, H + nc)
        c, o, m = measurer.measure_dense(image, lab, Q, mad=True)
        same((c, o, m), QR.measure(image, lab, Q, True))
        v = image[0].reshape(H * W, nc)                                  # n = 1: every order statistic is the pixel, every deviation 0
        assert (c == 1).all() and (o[0] == v[:, :, None, None]).all() and (m[0, :, :, :2] == v[:, :, None]).all() and not m[:, :, :, 2:].any()
    ex = (lab % 3 == 0).astype(np.int32)
    same(measurer.measure_dense(image, lab, Q, mad=True, exclude=ex), QR.measure(image, lab, Q, True, ex))


def test_one_object_the_selection_loops_over(measurer):
    image = QR.noise((1, 600, 700), 1, np.uint16, 3)[..., 0]
    lab = np.ones((1, 600, 700), np.int32)
    c, o, m = measurer.measure_dense(image, lab, Q, mad=True)
    same((c, o, m), QR.measure(image, lab, Q, True))
    s = np.sort(image.reshape(-1))
    n = s.size
    assert c.tolist() == [[n]] and o[0, 0, 0, 1].tolist() == [int(s[(n - 1) // 2]), int(s[n // 2])]
    lab[0, 300:, :] = 2                                                  # two of them, neither segment aligned
    lab[0, 0, :3] = 0
    same(measurer.measure_dense(image, lab, Q, mad=True), QR.measure(image, lab, Q, True))


def test_the_largest_object_against_closed_forms(measurer):
    side = 4096
    n = side * side
    image = (np.arange(n, dtype=np.uint32) & 65535).astype(np.uint16).reshape(1, side, side)    # v = (r * 4096 + c) mod 65536
    lab = np.ones((1, side, side), np.int32)
    q = Q + ((0, 1), (1, 1), (1, 3))
    c, o, m = measurer.measure_dense(image, lab, q, mad=True)
    assert c.tolist() == [[n]]
    for k, (num, den) in enumerate(q):                                   # every value occurs 256 times: s[k] = k // 256
        t = num * (n - 1)
        lo = t // den
        hi = lo + (t % den > 0)
        assert o[0, 0, 0, k].tolist() == [lo // 256, hi // 256], (num, den)
    # m_lo + m_hi = 32767 + 32768; d = |2 v - 65535| takes every odd value up to 65535 512 times: d[k] = 2 (k // 512) + 1
    lo, hi = (n - 1) // 2, n // 2
    assert m.tolist() == [[[[32767, 32768, 2 * (lo // 512) + 1, 2 * (hi // 512) + 1]]]]
    t = QN.quantile_table(c, o, m, q)
    assert t.median.tolist() == [[32767.5]] and t.mad.tolist() == [[16384.0]] and t.value[0, 0, 1] == 32767.5


def test_radix_edges(measurer):
    rng = np.random.default_rng(11)
    shape = (70, 300)
    lab = np.stack([QR.disks(shape, 30, 1), QR.disks(shape, 30, 2)])
    flat = QR.noise((2,) + shape, 2, np.uint16, 4, base=60000, spread=600)                       # the high byte hardly varies
    flat[..., 1] = 40000                                                                         # a constant channel: all ties
    same(measurer.measure_dense(flat, lab, Q, mad=True), QR.measure(flat, lab, Q, True))
    for dtype in (np.uint8, np.uint16):
        const = np.full((2,) + shape, 255, dtype)
        same(measurer.measure_dense(const, lab, Q, mad=True), QR.measure(const, lab, Q, True))
    edge = (255 + rng.integers(0, 2, (2,) + shape + (3,))).astype(np.uint16)                     # 255 and 256: a step of the high byte
    same(measurer.measure_dense(edge, lab, Q, mad=True), QR.measure(edge, lab, Q, True))
    # deviations beyond 16 bits: most pixels dark, a fifth of them at the top (d = 131070); then a median in the middle with both
    # ends present (d = 65534, 0 and 65536)
    far = np.where(rng.random(4000) < 0.2, 65535, rng.integers(0, 3, 4000)).astype(np.uint16)
    mid = np.r_[np.zeros(2000), np.full(7, 32767), np.full(2000, 65535)].astype(np.uint16)
    for v in (far, mid, mid[:-1], mid[1:]):
        img, one = one_object(rng.permutation(v))
        got = measurer.measure_dense(img, one, Q, mad=True)
        same(got, QR.measure(img, one, Q, True))
    assert got[2][0, 0, 0, 2] >= 65534
    image = QR.noise((2,) + shape, 3, np.uint16, 6)
    for q in (((1, 2),), ((0, 1),), ((1, 1),), QR.TWELVE[:8], QR.TWELVE[4:], ((1, 2),) * 8, ((65535, 65536), (1, 65536), (1, 3))):
        for mad in (False, True):                                        # n_q = 1 and 8, duplicates, any order, the finest fractions
            same(measurer.measure_dense(image, lab, q, mad=mad), QR.measure(image, lab, q, mad))
    small = QR.noise((1, 1, 40), 1, np.uint8, 8)[..., 0]                 # objects of 1 to 8 pixels in one row
    ids = np.repeat(np.arange(1, 9), np.arange(1, 9)).astype(np.int32)
    lab1 = np.r_[ids, np.zeros(4, np.int32)].reshape(1, 1, 40)
    same(measurer.measure_dense(small, lab1, QR.TWELVE[:8], mad=True), QR.measure(small, lab1, QR.TWELVE[:8], True))


def test_cross_checks_with_the_intensity_measurer(measurer):
    shape = (70, 300)
    lab = np.stack([QR.disks(shape, 30, 3), QR.disks(shape, 30, 4)])
    ex = np.stack([QR.disks(shape, 30, 3, radii=(1, 2)), np.zeros(shape, np.int32)])
    inten = IN.IntensityMeasurer(0)
    for nc, dtype in ((3, np.uint16), (4, np.uint8)):
        image = QR.noise((2,) + shape, nc, dtype, 13)
        c, o, _ = measurer.measure_dense(image, lab, ((0, 1), (1, 1)), exclude=ex)
        g, s = inten.measure_dense(image, lab, exclude=ex)
        assert np.array_equal(c, g[:, :, 0]) and np.array_equal(o[:, :, :, 0, 0], s[:, :, :, 4]) and np.array_equal(o[:, :, :, 1, 0], s[:, :, :, 5])
        assert np.array_equal(o[..., 0], o[..., 1])                      # at q = 0 and q = 1 the two ranks are one
    inten.close()


def test_exclude(measurer):
    shape = (70, 300)
    nuclei = np.stack([QR.disks(shape, 30, 1, radii=(2, 4)), QR.disks(shape, 30, 2, radii=(2, 4))])
    cells = np.stack([QR.disks(shape, 30, 1, radii=(5, 9)), QR.disks(shape, 30, 3, radii=(5, 9))])
    for nc, dtype in ((1, np.uint8), (3, np.uint16)):
        image = QR.noise((2,) + shape, nc, dtype, 5 + nc)
        want = QR.measure(image, cells, Q, True, nuclei)
        got = measurer.measure_dense(image, cells, Q, mad=True, exclude=nuclei)
        same(got, want)
        assert not np.array_equal(got[0], QR.measure(image, cells, Q, True)[0])   # the exclusion took pixels away
        big = (nuclei * 1000003).astype(np.int32) - (nuclei % 2) * 7      # any non-zero value counts, negative ones too
        same(measurer.measure_dense(image, cells, Q, mad=True, exclude=big), want)
        same(measurer.measure_dense(image, cells, Q, mad=True, exclude=np.zeros_like(cells)), measurer.measure_dense(image, cells, Q, mad=True))
        same(measurer.measure_dense(image, cells, Q, mad=True), QR.measure(image, cells, Q, True))
        c, o, m = measurer.measure_dense(image, cells, Q, mad=True, exclude=cells)      # swallowed whole: all zero
        assert not c.any() and not o.any() and not m.any() and o.shape == want[1].shape
        t = measurer.measure_batch(image, cells, mad=True, exclude=cells)
        assert len(t) == 0 and t.value.shape == (0, nc, 3) and t.mad.shape == (0, nc) and t.mad_raw.shape == (0, nc, 4)


def test_scalar_path_for_odd_widths_and_unaligned_tensor_views(measurer):
    import torch
    for shape in ((33, 258), (20, 7), (9, 301)):                         # widths that are no multiple of 4
        lab = batch_of(shape, 3)[0][1]
        for nc, dtype in ((3, np.uint8), (2, np.uint16)):
            image = QR.noise((2,) + shape, nc, dtype, 9)
            same(measurer.measure_dense(image, lab, Q, mad=True, exclude=(lab % 2).astype(np.int32)), QR.measure(image, lab, Q, True, lab % 2))
    shape = (40, 264)                                                    # a multiple of 4: only the pointers decide
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

    for nc, dtype in ((3, np.uint8), (1, np.uint8), (4, np.uint16), (3, np.uint16)):
        image = QR.noise((2,) + shape, nc, dtype, 10)
        want = QR.measure(image, lab, Q, True, ex)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), Q, mad=True, exclude=as_tensor(ex)), want)      # all aligned: wide loads
        same(measurer.measure_dense(shifted(image, 1), as_tensor(lab), Q, mad=True, exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), shifted(lab, 1), Q, mad=True, exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), Q, mad=True, exclude=shifted(ex, 3)), want)
        same(measurer.measure_dense(shifted(image, 1), shifted(lab, 2), Q, mad=True), QR.measure(image, lab, Q, True))


def test_input_kinds_repeatability_and_batch_independence(measurer):
    shape = (70, 300)
    lab = np.stack([QR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([QR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    for nc, dtype in ((3, np.uint16), (4, np.uint8)):
        image = QR.noise((3,) + shape, nc, dtype, 12)
        a = measurer.measure_dense(image, lab, Q, mad=True, exclude=ex)
        b = measurer.measure_dense(image, lab, Q, mad=True, exclude=ex)
        same(a, QR.measure(image, lab, Q, True, ex))
        same(b, a)                                                       # bit-identical run to run
        t = measurer.last_timing()
        assert set(t) == {"quantiles_count_ms", "quantiles_scatter_ms", "quantiles_select_ms"}
        assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), Q, mad=True, exclude=as_tensor(ex)), a)     # CUDA tensors in equal numpy in
        if dtype == np.uint16:
            import torch
            same(measurer.measure_dense(as_tensor(image).view(torch.uint16), as_tensor(lab), Q, mad=True), QR.measure(image, lab, Q, True))
        m = int(lab.max())
        for k in range(3):                                               # an image alone equals its rows in the batch
            got = measurer.measure_dense(image[k:k + 1].copy(), lab[k:k + 1].copy(), Q, mad=True, exclude=ex[k:k + 1].copy(), max_label=m)
            assert all(np.array_equal(g[0], x[k]) for g, x in zip(got, a))
        got = measurer.measure_dense(image, lab, Q, mad=True, max_label=m + 100)    # a larger table: the same rows, zeros behind them
        want = QR.measure(image, lab, Q, True)
        assert all(np.array_equal(g[:, :m], w) and not g[:, m:].any() for g, w in zip(got, want))
    fl = measurer.measure_batch(image, lab, (0.25, 0.5, 0.75, 0.01, 0.99), mad=True)              # floats are the same fractions
    d = QR.derive(*want, Q)
    assert fl.fractions == tuple(QN.as_fraction(q) for q in Q) and all(np.array_equal(getattr(fl, k), v) for k, v in d.items())
    with pytest.raises(TypeError):
        measurer.measure_dense(image, as_tensor(lab))
    with pytest.raises(ValueError):
        measurer.measure_dense(as_tensor(image)[:, :, ::2], as_tensor(lab)[:, :, ::2])


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    lab = batch_of(shape, 5)[0][1]
    image = QR.noise((2,) + shape, 3, np.uint8, 1)
    m = int(lab.max())
    want = QR.measure(image, lab, Q, True, max_label=m)
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 9, 255), m + 1), ((1, 3, 100), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                                               # range-checked on the device: never an index
        for args in ((image, bad), (as_tensor(image), as_tensor(bad))):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_dense(*args, Q, mad=True, max_label=m)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            with pytest.raises(L.CellScreenError):                      # whatever exclude holds there
                measurer.measure_dense(*args, Q, exclude=(np.ones_like(lab) if isinstance(args[1], np.ndarray) else as_tensor(np.ones_like(lab))),
                                       max_label=m)
            same(measurer.measure_dense(image, lab, Q, mad=True, max_label=m), want)
    neg = np.zeros_like(lab)
    neg[0, 2, 2] = -3
    with pytest.raises(L.CellScreenError):
        measurer.measure_batch(image, neg)                               # max_label=None on a batch without objects


def nuclei_scene():
    """uint16 [2,96,128,2]: five bright blobs per image on a noisy background in channel 0, noise in channel 1."""
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.empty((2, H, W, 2), np.uint16)
    for b in range(2):
        f = 300.0 + rng.normal(0.0, 10.0, (H, W))
        for y, x, r in ((24, 25, 9), (30, 80, 12), (70, 40, 10), (70, 100, 7 + 4 * b), (50, 62, 5)):
            f += 4000.0 * np.exp(-(((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (r / 1.6) ** 2)) ** 2)
        imgs[b, :, :, 0] = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
        imgs[b, :, :, 1] = rng.integers(0, 65536, (H, W))
    return imgs


def test_segment_expand_quantiles_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = as_tensor(imgs)
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)                    # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)
    meas = QN.QuantileMeasurer(0, extractor=seg)
    ring = meas.measure_batch(dev, grown, Q, mad=True, exclude=labels)
    whole = meas.measure_batch(dev, grown, Q, mad=True)
    nuc = meas.measure_batch(dev, labels, Q, mad=True)
    assert meas._pre is None                                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(nuc) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (whole, (h_grown, None)), (nuc, (h_lab, None))):
        d = QR.derive(*QR.measure(imgs, lab, Q, True, ex), Q)
        assert all(np.array_equal(getattr(t, k), v) for k, v in d.items())
    assert np.array_equal(ring.label, nuc.label) and np.array_equal(ring.count + nuc.count, whole.count)
    assert (nuc.median[:, 0] > 2.0 * ring.median[:, 0]).all()            # bright nuclei in channel 0, dim rings around them
    t = meas.last_timing()
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
