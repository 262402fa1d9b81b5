"""The per-object colocalization on the device (cs_label_colocalize through cellscreen.colocalize) against the CPU restatement of
tests/colocalize_reference.py, which tests/test_colocalize_cpu.py holds to its slow form and to SciPy.

The records are integers, so every comparison is np.array_equal on the dense tables: no tolerances, and the rows of absent objects
are compared too.

A lane of either walk owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows; SHAPES crosses the 16 rows, the 64 rows and
the 256 columns one short, equal and one past, and has the single row, the single column and the single pixel.  Widths that are no
multiple of 4 take the scalar loads.  The tables in LDS have 512 / 256 / 256 slots (moments) and 512 / 256 / 128 slots (thresholded)
at 2 / 3 / 4 channels: an image where every pixel is its own label fills them and sends the rest to the global tables."""
import ctypes as C
import functools

import numpy as np
import pytest

import colocalize_reference as CR
import intensity_reference as IR
from cellscreen import _lib as L
from cellscreen import colocalize as CO
from cellscreen import expand as EX
from cellscreen import intensity as IN
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1)]


@pytest.fixture(scope="module")
def measurer():
    m = CO.ColocalizationMeasurer(0)
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
    assert len(got) == len(want) == 4
    for g, w, name in zip(got, want, ("geom", "chan", "pair", "levels")):
        assert g.dtype == w.dtype == (np.int32 if name == "levels" else np.int64) and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w), (name, what)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement_across_the_tiles(measurer, shape, dtype):
    seed = 7 * shape[0] + shape[1]
    top = int(np.iinfo(dtype).max)
    for nc, rule in ((2, dict()), (3, dict(absolute=[top // 4, top // 2, 0])), (4, dict(threshold=(1, 2)))):
        image = IR.noise((2,) + shape, nc, dtype, seed + nc)
        for name, lab in batch_of(shape, seed):
            want = CR.measure(image, lab, **rule)
            same(measurer.measure_dense(image, lab, **rule), want, (name, nc))
            t = measurer.measure_batch(image, lab, **rule)
            d = CR.derive(*want)
            assert len(t) == len(d["label"]) and t.pairs == CR.pairs_of(nc), name
            assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items()), name
    few = IR.noise((2,) + shape, 3, dtype, seed, spread=7)               # few values: equal ranks, ties at the maximum
    lab = batch_of(shape, seed)[0][1]
    same(measurer.measure_dense(few, lab, threshold=(1, 1)), CR.measure(few, lab, threshold=(1, 1)))


@pytest.mark.parametrize("nc", [2, 4])
@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_every_pixel_its_own_label_overflows_the_tables_in_lds(measurer, shape, nc):
    H, W = shape
    lab = np.stack([np.arange(1, H * W + 1, dtype=np.int32).reshape(shape), np.arange(H * W, 0, -1, dtype=np.int32).reshape(shape)])
    for dtype in (np.uint16, np.uint8):
        image = IR.noise((2,) + shape, nc, dtype, H + nc)
        g, c, p, lv = got = measurer.measure_dense(image, lab)
        same(got, CR.measure(image, lab))
        assert (g[:, :, 0] == 1).all() and np.array_equal(c[0, :, :, 2], image[0].reshape(H * W, nc)) and (c[:, :, :, 3] == 1).all()
        assert np.array_equal(p[0, :, 0, 0], image[0, :, :, 0].reshape(-1).astype(np.int64) * image[0, :, :, 1].reshape(-1))
    ex = (lab % 3 == 0).astype(np.int32)
    same(measurer.measure_dense(image, lab, exclude=ex), CR.measure(image, lab, ex))
    same(measurer.measure_dense(image, lab, exclude=ex, absolute=[128] * nc, rwc=False), CR.measure(image, lab, ex, absolute=[128] * nc, rwc=False))


def ramp_records(v0, v1, mult, num, den):
    """chan [2][5] and pair [9] of one object whose pixels are (v0[k], v1[k]), each `mult` times, every value of 0..65535 present in
    both channels: closed forms from the 65536 values, in Python ints."""
    v0, v1 = v0.astype(np.int64), v1.astype(np.int64)
    up0, up1 = v0 * den >= num * int(v0.max()), v1 * den >= num * int(v1.max())
    both = up0 & up1
    w = 65536 - np.abs(v0 - v1)                                          # every value occurs: rank = value, R = 65536
    tot = lambda x: mult * int(x.sum())
    chan = [[tot(v), tot(v * v), int(v.max()), tot(up), tot(v * up)] for v, up in ((v0, up0), (v1, up1))]
    pair = [tot(v0 * v1), tot(both), tot(v0 * both), tot(v1 * both), tot(v0 * v0 * both), tot(v1 * v1 * both), tot(v0 * v1 * both),
            tot(v0 * w * both), tot(v1 * w * both)]
    return chan, pair


def test_the_largest_sums_against_closed_forms(measurer):
    side, v = 4096, 65535
    n = side * side
    sr = side * (side * (side - 1) // 2)                                 # sum of r over the plane, and of c
    lab = np.ones((1, side, side), np.int32)
    image = np.full((1, side, side, 2), v, np.uint16)
    g, c, p, lv = measurer.measure_dense(image, lab)
    assert g.tolist() == [[[n, sr, sr]]] and lv.tolist() == [[1, 1]]
    assert c.tolist() == [[[[n * v, n * v * v, v, n, n * v]] * 2]]
    assert p.tolist() == [[[[n * v * v, n, n * v, n * v, n * v * v, n * v * v, n * v * v, n * v, n * v]]]]      # R = 1, w = 1
    t = CO.colocalization_table(g, c, p, lv)
    assert np.isnan(t.pearson[0, 0]) and np.isnan(t.slope[0, 0]) and t.overlap[0, 0] == t.k1[0, 0] == t.manders1[0, 0] == t.rwc1[0, 0] == t.rwc2[0, 0] == 1.0
    # opposite ramps over all 65536 values: R = 65536 and |rank_i - rank_j| = |2 v - 65535| spans 1..65535
    vals = np.arange(65536, dtype=np.int64)
    ramp = (np.arange(n, dtype=np.int64) % 65536).astype(np.uint16).reshape(side, side)
    image[0, :, :, 0] = ramp
    image[0, :, :, 1] = 65535 - ramp
    for num, den in ((0, 1), (15, 100)):
        g, c, p, lv = measurer.measure_dense(image, lab, threshold=(num, den))
        chan, pair = ramp_records(vals, 65535 - vals, n // 65536, num, den)
        assert g.tolist() == [[[n, sr, sr]]] and lv.tolist() == [[65536, 65536]]
        assert c.tolist() == [[chan]] and p.tolist() == [[[pair]]]
    t = CO.colocalization_table(g, c, p, lv)
    assert abs(t.pearson[0, 0] + 1.0) <= 4 * 2.0 ** -53 and t.slope[0, 0] == -1.0


def test_threshold_ties_count_as_above(measurer):
    lab = np.ones((1, 3, 8), np.int32)
    lab[0, 2] = 2
    image = np.zeros((1, 3, 8, 2), np.uint16)
    image[0, 0, :, 0] = [100, 15, 14, 16, 0, 99, 15, 14]                 # maximum 100: 15 is the tie of 15 / 100
    image[0, 1, :, 0] = [15, 14, 100, 0, 0, 0, 0, 15]
    image[0, :2, :, 1] = 40000
    image[0, 1, 7, 1] = 6000                                             # 6000 * 100 == 15 * 40000: a tie; 5999 is below
    image[0, 1, 6, 1] = 5999
    image[0, 2, :, 0] = [65535, 65534, 65535, 0, 1, 65535, 65534, 65535]  # label 2, for 1 / 1
    image[0, 2, :, 1] = [7, 7, 6, 7, 0, 7, 7, 6]
    for rule, above in ((dict(threshold=(15, 100)), {1: [8, 15], 2: [6, 7]}), (dict(threshold=(1, 1)), {1: [2, 14], 2: [4, 5]}),
                        (dict(threshold=(0, 1)), {1: [16, 16], 2: [8, 8]}), (dict(threshold=(65536, 65536)), {1: [2, 14], 2: [4, 5]}),
                        (dict(absolute=[0, 0]), {1: [16, 16], 2: [8, 8]}), (dict(absolute=[65536, 65536]), {1: [0, 0], 2: [0, 0]}),
                        (dict(absolute=[15, 6000]), {1: [8, 15], 2: [6, 0]}), (dict(absolute=[16, 6001]), {1: [4, 14], 2: [6, 0]})):
        got = measurer.measure_dense(image, lab, **rule)
        same(got, CR.measure(image, lab, **rule), rule)
        assert got[1][0, :, :, 3].tolist() == [above[1], above[2]], rule
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):             # v den and num max at their extremes
        im = np.full((1, 2, 2, 2), top, dtype)
        im[0, 0, 0] = top - 1, top
        got = measurer.measure_dense(im, np.ones((1, 2, 2), np.int32), threshold=(65536, 65536))
        same(got, CR.measure(im, np.ones((1, 2, 2), np.int32), threshold=(65536, 65536)))
        assert got[1][0, 0, :, 3].tolist() == [3, 4] and got[2][0, 0, 0, 1] == 3


def test_exclude(measurer):
    shape = (70, 300)
    nuclei = np.stack([IR.disks(shape, 30, 1, radii=(2, 4)), IR.disks(shape, 30, 2, radii=(2, 4))])
    cells = np.stack([IR.disks(shape, 30, 1, radii=(5, 9)), IR.disks(shape, 30, 3, radii=(5, 9))])
    for nc, dtype in ((2, np.uint8), (3, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, 5 + nc)
        want = CR.measure(image, cells, nuclei)
        got = measurer.measure_dense(image, cells, exclude=nuclei)
        same(got, want)
        assert not np.array_equal(got[0], CR.measure(image, cells)[0])    # the exclusion took pixels away
        big = (nuclei * 1000003).astype(np.int32) - (nuclei % 2) * 7      # any non-zero value counts, negative ones too
        same(measurer.measure_dense(image, cells, exclude=big), want)
        same(measurer.measure_dense(image, cells, exclude=np.zeros_like(cells)), measurer.measure_dense(image, cells))
        same(measurer.measure_dense(image, cells), CR.measure(image, cells))
        g, c, p, lv = measurer.measure_dense(image, cells, exclude=cells)  # swallowed whole: all zero, the levels too
        assert not g.any() and not c.any() and not p.any() and not lv.any() and p.shape == want[2].shape
        t = measurer.measure_batch(image, cells, exclude=cells)
        assert len(t) == 0 and t.pearson.shape == (0, nc * (nc - 1) // 2) and t.chan.shape == (0, nc, 5)
    # a value that occurs only on excluded or background pixels gets no rank
    lab = np.zeros((1, 20, 40), np.int32)
    lab[0, 2:18, 4:36] = 1
    image = IR.noise((1, 20, 40), 2, np.uint8, 3, spread=50)
    ex = np.zeros_like(lab)
    ex[0, 5:9, 10:20] = 9
    image[0, 5:9, 10:20, 0] = 200                                        # only under `exclude`
    image[0, 0, :, 1] = 250                                              # only on the background
    got = measurer.measure_dense(image, lab, exclude=ex)
    same(got, CR.measure(image, lab, ex))
    on = (lab[0] > 0) & (ex[0] == 0)
    assert got[3].tolist() == [[len(np.unique(image[0, :, :, c][on])) for c in range(2)]] and max(got[3][0]) <= 50
    assert measurer.measure_dense(image, lab)[3][0, 0] == got[3][0, 0] + 1          # without the plane 200 is ranked


def test_ranks_are_per_image(measurer):
    shape = (40, 264)
    lab = np.stack([IR.disks(shape, 12, k) for k in (1, 2, 3)])
    image = np.stack([IR.noise(shape, 3, np.uint16, 1, spread=300), IR.noise(shape, 3, np.uint16, 2, base=1000, spread=5000),
                      IR.noise(shape, 3, np.uint16, 3, base=60000, spread=17)])
    whole = measurer.measure_dense(image, lab)
    same(whole, CR.measure(image, lab))
    assert len({tuple(x) for x in whole[3].tolist()}) == 3               # the value sets differ
    m = int(lab.max())
    for k in range(3):                                                   # an image alone equals its rows in the batch, ranks included
        one = measurer.measure_dense(image[k:k + 1].copy(), lab[k:k + 1].copy(), max_label=m)
        assert all(np.array_equal(x[0], y[k]) for x, y in zip(one, whole))
    g, c, p, lv = measurer.measure_dense(image, lab, max_label=m + 100)  # a larger table: the same rows, zeros behind them
    assert np.array_equal(p[:, :m], whole[2]) and not g[:, m:].any() and not c[:, m:].any() and not p[:, m:].any() and np.array_equal(lv, whole[3])


def test_without_rwc_the_rank_fields_and_levels_are_zero(measurer):
    shape = (33, 258)
    lab = batch_of(shape, 3)[0][1]
    for nc, dtype in ((2, np.uint16), (3, np.uint8), (4, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, 9)
        with_rwc = measurer.measure_dense(image, lab)
        g, c, p, lv = without = measurer.measure_dense(image, lab, rwc=False)
        same(without, CR.measure(image, lab, rwc=False))
        assert not lv.any() and not p[..., 7:].any() and with_rwc[2][..., 7:].any() and with_rwc[3].all()
        assert np.array_equal(g, with_rwc[0]) and np.array_equal(c, with_rwc[1]) and np.array_equal(p[..., :7], with_rwc[2][..., :7])
        assert measurer.last_timing()["colocalize_ranks_ms"] == 0.0
        t = measurer.measure_batch(image, lab, rwc=False)
        assert np.isnan(t.rwc1).all() and np.isnan(t.rwc2).all() and not np.isnan(t.pearson).any()


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    lab = batch_of(shape, 5)[0][1]
    image = IR.noise((2,) + shape, 3, np.uint8, 1)
    m = int(lab.max())
    want = CR.measure(image, lab, max_label=m)
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 0, 0), m + 1), ((1, 16, 256), 2 ** 31 - 1)):
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


def test_channel_counts_and_the_scratch_cap_are_refused_before_the_device_is_touched(measurer):
    lib, h = measurer._lib, measurer._handle                            # a live handle: the refusals are the arguments' own
    many = 2731                                                          # 2731 x 2 x 192 KB is just above 1 GiB
    zeros = np.zeros(4 * many, np.int32)                                 # image and labels: no objects
    outs = [np.empty(many * k, dt) for k, dt in ((3, np.int64), (4 * 5, np.int64), (6 * 9, np.int64), (4, np.int32))]
    prm = CO.colocalize_params(2)

    def status(channels, B=1, rwc=1):
        prm.rwc = rwc
        for o in outs:
            o[:] = -5
        rc = lib.cs_label_colocalize(h, zeros.ctypes.data, 0, channels, zeros.ctypes.data, None, B, 1, 1, 0, 1, C.byref(prm),
                                     *(o.ctypes.data for o in outs), 0)
        assert rc == 0 or all((o == -5).all() for o in outs)             # a refused call wrote nothing
        return rc, lib.cs_last_error().decode()

    assert status(1)[0] == -1 and "needs at least 2" in status(1)[1]
    assert status(5)[0] == -6 and "at most 4" in status(5)[1]
    assert status(2, B=many)[0] == -6 and "split the batch" in status(2, B=many)[1]
    assert status(2, B=many, rwc=0)[0] == 0                              # no rank tables, no cap
    lab = np.ones((1, 4, 4), np.int32)
    for image in (np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4, 1), np.uint8), np.zeros((1, 4, 4, 5), np.uint8)):
        with pytest.raises(ValueError):
            measurer.measure_dense(image, lab)
    with pytest.raises(ValueError, match="split the batch"):
        measurer.measure_dense(np.zeros((2731, 1, 1, 2), np.uint8), np.zeros((2731, 1, 1), np.int32), max_label=1)
    image = IR.noise((1, 4, 4), 2, np.uint8, 1)
    same(measurer.measure_dense(image, lab), CR.measure(image, lab))     # and the measurer works


def test_input_kinds_and_repeatability(measurer):
    import torch
    shape = (70, 300)
    lab = np.stack([IR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([IR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    for nc, dtype in ((3, np.uint16), (4, np.uint8), (2, np.uint16)):
        image = IR.noise((3,) + shape, nc, dtype, 12)
        a = measurer.measure_dense(image, lab, exclude=ex)
        b = measurer.measure_dense(image, lab, exclude=ex)
        same(a, CR.measure(image, lab, ex))
        same(b, a)                                                       # bit-identical run to run
        t = measurer.last_timing()
        assert set(t) == {"colocalize_clear_ms", "colocalize_moments_ms", "colocalize_ranks_ms", "colocalize_thresholded_ms"}
        assert len(t) == 4 and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex)), a)     # CUDA tensors in equal numpy in
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex)), a)
        if dtype == np.uint16:                                           # uint16 as int16 views, and as uint16 tensors
            assert as_tensor(image).dtype == torch.int16
            same(measurer.measure_dense(as_tensor(image).view(torch.uint16), as_tensor(lab)), CR.measure(image, lab))
    geom = IN.IntensityMeasurer(0, extractor=measurer).measure_dense(image, lab, exclude=ex)[0]
    assert np.array_equal(geom, a[0])                                    # cs_label_intensity's geom, bit for bit
    with pytest.raises(TypeError):
        measurer.measure_dense(image, as_tensor(lab))
    with pytest.raises(ValueError):
        measurer.measure_dense(as_tensor(image)[:, :, ::2], as_tensor(lab)[:, :, ::2])


def test_unaligned_tensor_views_take_the_scalar_loads(measurer):
    import torch
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

    for nc, dtype in ((3, np.uint8), (2, np.uint8), (4, np.uint16), (3, np.uint16)):
        image = IR.noise((2,) + shape, nc, dtype, 10)
        want = CR.measure(image, lab, ex)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex)), want)           # all aligned: wide loads
        same(measurer.measure_dense(shifted(image, 1), as_tensor(lab), exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), shifted(lab, 1), exclude=as_tensor(ex)), want)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=shifted(ex, 3)), want)


def nuclei_scene():
    """uint16 [2,96,128,2]: five bright blobs per image on a noisy background in channel 0; channel 1 follows channel 0 with noise."""
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.empty((2, H, W, 2), np.uint16)
    for b in range(2):
        f = 300.0 + rng.normal(0.0, 10.0, (H, W))
        for y, x, r in ((24, 25, 9), (30, 80, 12), (70, 40, 10), (70, 100, 7 + 4 * b), (50, 62, 5)):
            f += 4000.0 * np.exp(-(((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (r / 1.6) ** 2)) ** 2)
        imgs[b, :, :, 0] = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
        imgs[b, :, :, 1] = np.clip(np.rint(0.5 * f + rng.normal(0.0, 60.0, (H, W))), 0, 65535).astype(np.uint16)
    return imgs


def test_segment_expand_measure_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = as_tensor(imgs)
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)                    # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)
    meas = CO.ColocalizationMeasurer(0, extractor=seg)
    ring = meas.measure_batch(dev, grown, exclude=labels)
    whole = meas.measure_batch(dev, grown)
    nuc = meas.measure_batch(dev, labels)
    assert meas._pre is None                                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(nuc) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (whole, (h_grown, None)), (nuc, (h_lab, None))):
        tables = CR.measure(imgs, lab, ex)
        d = CR.derive(*tables)
        assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items()) and np.array_equal(t.levels, tables[3])
    assert np.array_equal(ring.label, nuc.label) and np.array_equal(ring.area + nuc.area, whole.area)
    assert np.array_equal(ring.pair[..., 0] + nuc.pair[..., 0], whole.pair[..., 0])
    assert (whole.pearson[:, 0] > 0.9).all() and (whole.slope[:, 0] > 0.4).all() and (whole.slope[:, 0] < 0.6).all()      # channel 1 is half of channel 0
    t = meas.last_timing()
    assert len(t) == 4 and all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
