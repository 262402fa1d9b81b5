"""The per-object intensities on the device (cs_label_intensity through cellscreen.intensity) against the CPU restatement of
tests/intensity_reference.py, which tests/test_intensity_cpu.py holds to scipy.ndimage.

The tables are integers, so every comparison is np.array_equal on the dense tables: no tolerances, and the rows of absent
objects are compared too.

A lane of the pass owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows; SHAPES crosses the 16 rows, the 64 rows and
the 256 columns one short, equal and one past, and has the single row, the single column and the single pixel.  Widths that are
no multiple of 4 take the scalar path.  The table in LDS has 512 slots at one channel and 256 above: an image where every pixel
is its own label fills it and sends the rest to the global tables."""
import functools

import numpy as np
import pytest

import intensity_reference as IR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import intensity as IN
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1)]


@pytest.fixture(scope="module")
def measurer():
    m = IN.IntensityMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
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


def same(got, want):
    (g, s), (wg, ws) = got, want
    assert g.dtype == s.dtype == np.int64 and g.shape == wg.shape and s.shape == ws.shape
    assert np.array_equal(g, wg) and np.array_equal(s, ws)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement_across_the_tiles(measurer, shape, dtype):
    seed = 7 * shape[0] + shape[1]
    for nc in (1, 3, 4):
        image = IR.noise((2,) + shape, nc, dtype, seed + nc)
        for name, lab in batch_of(shape, seed):
            want = IR.measure(image, lab)
            same(measurer.measure_dense(image, lab), want)
            t = measurer.measure_batch(image, lab)
            d = IR.derive(*want)
            assert len(t) == len(d["label"]) and all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items()), name
    one = IR.noise((2,) + shape, 1, dtype, seed)[..., 0]                 # [B,H,W]: one channel
    same(measurer.measure_dense(one, batch_of(shape, seed)[0][1]), IR.measure(one, batch_of(shape, seed)[0][1]))


@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_every_pixel_its_own_label_overflows_the_table_in_lds(measurer, shape):
    H, W = shape
    lab = np.stack([np.arange(1, H * W + 1, dtype=np.int32).reshape(shape), np.arange(H * W, 0, -1, dtype=np.int32).reshape(shape)])
    for nc, dtype in ((1, np.uint16), (3, np.uint8), (4, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, H + nc)
        g, s = measurer.measure_dense(image, lab)
        same((g, s), IR.measure(image, lab))
        assert (g[:, :, 0] == 1).all() and np.array_equal(s[0, :, :, 4], image[0].reshape(H * W, nc))
    ex = (lab % 3 == 0).astype(np.int32)
    same(measurer.measure_dense(image, lab, exclude=ex), IR.measure(image, lab, ex))


def test_the_largest_sums_against_closed_forms(measurer):
    side, v = 4096, 65535
    image = np.full((1, side, side), v, np.uint16)
    lab = np.ones((1, side, side), np.int32)
    g, s = measurer.measure_dense(image, lab)
    n = side * side
    sr = side * (side * (side - 1) // 2)                                 # sum of r over the plane, and of c
    assert g.tolist() == [[[n, sr, sr]]]
    assert s.tolist() == [[[[n * v, n * v * v, v * sr, v * sr, v, v]]]]
    t = IN.object_table(g, s)
    assert t.mean[0, 0] == v and t.std[0, 0] == 0.0 and t.centroid.tolist() == [[2047.5, 2047.5]] and t.weighted_centroid.tolist() == [[[2047.5, 2047.5]]]
    lab[:] = 0
    lab[0, side - 1, side - 1] = 1
    g, s = measurer.measure_dense(image, lab)
    assert g.tolist() == [[[1, side - 1, side - 1]]]
    assert s.tolist() == [[[[v, v * v, v * (side - 1), v * (side - 1), v, v]]]]


def test_exclude(measurer):
    shape = (70, 300)
    nuclei = np.stack([IR.disks(shape, 30, 1, radii=(2, 4)), IR.disks(shape, 30, 2, radii=(2, 4))])
    cells = np.stack([IR.disks(shape, 30, 1, radii=(5, 9)), IR.disks(shape, 30, 3, radii=(5, 9))])
    for nc, dtype in ((1, np.uint8), (3, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, 5 + nc)
        want = IR.measure(image, cells, nuclei)
        got = measurer.measure_dense(image, cells, exclude=nuclei)
        same(got, want)
        assert not np.array_equal(got[0], IR.measure(image, cells)[0])    # the exclusion took pixels away
        big = (nuclei * 1000003).astype(np.int32) - (nuclei % 2) * 7      # any non-zero value counts, negative ones too
        same(measurer.measure_dense(image, cells, exclude=big), want)
        same(measurer.measure_dense(image, cells, exclude=np.zeros_like(cells)), measurer.measure_dense(image, cells))
        same(measurer.measure_dense(image, cells), IR.measure(image, cells))
        g, s = measurer.measure_dense(image, cells, exclude=cells)       # swallowed whole: all zero, the minimum included
        assert not g.any() and not s.any() and g.shape == want[0].shape
        t = measurer.measure_batch(image, cells, exclude=cells)
        assert len(t) == 0 and t.mean.shape == (0, nc) and t.weighted_centroid.shape == (0, nc, 2)


def test_scalar_path_for_odd_widths_and_unaligned_tensor_views(measurer):
    import torch
    for shape in ((33, 258), (20, 7), (9, 301)):                         # widths that are no multiple of 4
        lab = batch_of(shape, 3)[0][1]
        for nc, dtype in ((3, np.uint8), (2, np.uint16)):
            image = IR.noise((2,) + shape, nc, dtype, 9)
            same(measurer.measure_dense(image, lab, exclude=(lab % 2).astype(np.int32)), IR.measure(image, lab, lab % 2))
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
        image = IR.noise((2,) + shape, nc, dtype, 10)
        want = IR.measure(image, lab, ex)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex)), want)           # all aligned: wide loads
        same(measurer.measure_dense(shifted(image, 1), as_tensor(lab), exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), shifted(lab, 1), exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=shifted(ex, 3)), want)
        same(measurer.measure_dense(shifted(image, 1), shifted(lab, 2)), IR.measure(image, lab))


def test_input_kinds_repeatability_and_batch_independence(measurer):
    shape = (70, 300)
    lab = np.stack([IR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([IR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    for nc, dtype in ((3, np.uint16), (4, np.uint8)):
        image = IR.noise((3,) + shape, nc, dtype, 12)
        a = measurer.measure_dense(image, lab, exclude=ex)
        b = measurer.measure_dense(image, lab, exclude=ex)
        same(a, IR.measure(image, lab, ex))
        same(b, a)                                                       # bit-identical run to run
        t = measurer.last_timing()
        assert set(t) == {"intensity_clear_ms", "intensity_pass_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex)), a)     # CUDA tensors in equal numpy in
        if dtype == np.uint16:
            import torch
            same(measurer.measure_dense(as_tensor(image).view(torch.uint16), as_tensor(lab)), IR.measure(image, lab))
        m = int(lab.max())
        for k in range(3):                                               # an image alone equals its rows in the batch
            g, s = measurer.measure_dense(image[k:k + 1].copy(), lab[k:k + 1].copy(), exclude=ex[k:k + 1].copy(), max_label=m)
            assert np.array_equal(g[0], a[0][k]) and np.array_equal(s[0], a[1][k])
        g, s = measurer.measure_dense(image, lab, max_label=m + 100)     # a larger table: the same rows, zeros behind them
        assert np.array_equal(g[:, :m], IR.measure(image, lab)[0]) and not g[:, m:].any() and not s[:, m:].any()
    with pytest.raises(TypeError):
        measurer.measure_dense(image, as_tensor(lab))
    with pytest.raises(ValueError):
        measurer.measure_dense(as_tensor(image)[:, :, ::2], as_tensor(lab)[:, :, ::2])


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    lab = batch_of(shape, 5)[0][1]
    image = IR.noise((2,) + shape, 3, np.uint8, 1)
    m = int(lab.max())
    want = IR.measure(image, lab, max_label=m)
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 9, 255), m + 1), ((1, 3, 100), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                                               # range-checked on the device: never an index
        for args in ((image, bad), (as_tensor(image), as_tensor(bad))):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_dense(*args, max_label=m)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            with pytest.raises(L.CellScreenError):                      # whatever exclude holds there
                measurer.measure_dense(*args, exclude=(np.ones_like(lab) if isinstance(args[1], np.ndarray) else as_tensor(np.ones_like(lab))),
                                       max_label=m)
            same(measurer.measure_dense(image, lab, max_label=m), want)
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


def test_segment_expand_measure_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = as_tensor(imgs)
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)                    # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)
    meas = IN.IntensityMeasurer(0, extractor=seg)
    ring = meas.measure_batch(dev, grown, exclude=labels)
    whole = meas.measure_batch(dev, grown)
    nuc = meas.measure_batch(dev, labels)
    assert meas._pre is None                                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(nuc) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (whole, (h_grown, None)), (nuc, (h_lab, None))):
        d = IR.derive(*IR.measure(imgs, lab, ex))
        assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items())
    assert np.array_equal(ring.label, nuc.label) and np.array_equal(ring.area + nuc.area, whole.area)
    assert np.array_equal(ring.integrated + nuc.integrated, whole.integrated)
    assert (nuc.mean[:, 0] > 2.0 * ring.mean[:, 0]).all()                # bright nuclei in channel 0, dim rings around them
    t = meas.last_timing()
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
