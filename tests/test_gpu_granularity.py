"""The per-object granularity spectrum on the device (cs_label_granularity through cellscreen.granularity) against the CPU
restatement of tests/granularity_reference.py, which tests/test_granularity_cpu.py holds to its slow form and to SciPy.

The records are integers, so every comparison is np.array_equal on the dense tables and on the planes R_0..R_steps: no tolerances,
and the rows of absent objects are compared too.

The prepare pass gives a thread max(4, s) columns of the s rows of a block row; the erosion four pixels of a row; the reconstruction
relaxes tiles of 64 x 32 pixels of the working plane with a one-pixel halo; a lane of the sums pass owns 4 columns x 16 rows, a wave
256 columns, a workgroup 64 rows.  SHAPES crosses the 16, 32 and 64 rows and the 64 and 256 columns one short, equal and one past,
and has the single row, the single column and the single pixel.  Widths that are no multiple of 4 take the scalar loads; subsample 8, the one
block size at which a prepare thread loads two quads of a row, runs on all of them too, none a multiple of 8 but (16, 256),
(32, 64) and (64, 256).  The table
in LDS has 256 label slots: an image where every pixel is its own label fills it and sends the rest to the global table."""
import ctypes as C
import functools

import numpy as np
import pytest

import granularity_reference as GR
import intensity_reference as IR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import granularity as GA
from cellscreen import intensity as IN
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (1, 1), (15, 255), (16, 256), (17, 257), (31, 63), (32, 64), (33, 65), (63, 255), (64, 256), (65, 257)]
NAMES = ("geom", "sums", "image_sums", "planes")
TILE_W, TILE_H = 64, 32                                  # the reconstruction's


@pytest.fixture(scope="module")
def measurer():
    m = GA.GranularityMeasurer(0)
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
    assert len(got) in (3, 4) and len(want) == 4
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype == (np.uint16 if name == "planes" else np.int64) and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w), (name, what)


def speckled(shape, nc, dtype, seed):
    """[2,H,W,nc]: low noise with bright squares of side 1, 3 and 5 and a few blobs: structure at several steps of the spectrum"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    H, W = shape
    a = rng.integers(0, top // 8 + 1, (2, H, W, nc)).astype(np.int64)
    for _ in range(max(2, H * W // 150)):
        b, r, c, ch, h = int(rng.integers(2)), int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(nc)), int(rng.integers(3))
        a[b, max(0, r - h):r + h + 1, max(0, c - h):c + h + 1, ch] += top // 2
    return np.clip(a, 0, top).astype(dtype)


# ---- tables across the tiles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_and_planes_equal_the_restatement_across_the_tiles(measurer, shape, dtype):
    seed = 7 * shape[0] + shape[1]
    H, W = shape
    for nc, s, masked, steps in ((1, 1, False, 3), (2, 2, True, 2), (3, 4, False, 6), (4, 1, True, 2), (2, 8, False, 2), (3, 8, True, 3)):
        image = (IR.noise if nc % 2 else speckled)((2,) + shape if nc % 2 else shape, nc, dtype, seed + nc)
        if nc == 1:
            image = image[..., 0]                        # [B,H,W] is one channel
        kw = dict(steps=steps, subsample=s, masked=masked)
        for name, lab in batch_of(shape, seed):
            want = GR.measure(image, lab, **kw)
            same(measurer.measure_dense(image, lab, want_planes=True, **kw), want, (name, nc))
            ex = ((lab + np.arange(W)[None, None, :] + np.arange(H)[None, :, None]) % 5 == 0).astype(np.int32) * 9
            same(measurer.measure_dense(image, lab, exclude=ex, want_planes=True, **kw), GR.measure(image, lab, ex, **kw), (name, nc, "exclude"))
            t = measurer.measure_batch(image, lab, **kw)
            d = GR.derive(*want[:3])
            assert len(t) == len(d["label"]), name
            assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items()), name


# ---- the reconstruction must travel -------------------------------------------------------------------------------------------------------
def serpentine(shape, passes, level, blob_level):
    """A corridor 3 px wide at `level` on zero that runs the whole width in rows y..y+2 for y in `passes`, joined at alternating ends,
    with a 7 x 7 blob at `blob_level` at its start."""
    H, W = shape
    p = np.zeros(shape, np.uint16)
    for i, y in enumerate(passes):
        p[y:y + 3, 2:W - 2] = level
        if i + 1 < len(passes):
            x = W - 5 if i % 2 == 0 else 2
            p[y:passes[i + 1] + 3, x:x + 3] = level
    y = passes[0]
    p[y - 2:y + 5, 2:9] = blob_level
    return p


def test_the_reconstruction_travels_the_whole_corridor_and_one_image_does_not_cut_short_the_other(measurer):
    shape = (70, 600)
    passes = (3, 19, 35, 51, 65)                         # two in each of the first two rows of tiles, one in the third
    image = np.stack([serpentine(shape, passes, 1000, 3000), IR.noise(shape, 1, np.uint16, 4)[..., 0]])
    tiles_x = -(-shape[1] // TILE_W)
    for y in passes:                                     # the corridor crosses every tile of the plane
        assert all((image[0, y:y + 3, x * TILE_W:(x + 1) * TILE_W] > 0).any() for x in range(tiles_x))
    assert {y // TILE_H for y in passes} == set(range(-(-shape[0] // TILE_H)))
    lab = np.stack([np.ones(shape, np.int32), IR.disks(shape, 40, 3)])
    want = GR.measure(image, lab, steps=4)
    got = measurer.measure_dense(image, lab, steps=4, want_planes=True)
    rounds, reads = measurer.last_rounds()
    same(got, want)
    sums = got[1][0, 0, :, 0]
    # step 1 leaves the corridor's middle line, steps 2 and 3 nothing of it but the blob's core: all of it is refilled from there
    assert sums[0] == int(image[0].sum()) and sums[1] == sums[2] == sums[3] == sums[0] and sums[4] == 0
    assert np.array_equal(got[3][0, 2, 0], image[0]) and not got[3][0, 4, 0].any()
    along = tiles_x * -(-shape[0] // TILE_H)             # the tiles along the corridor, all of the plane: a quiet first tile must not end the loop
    assert rounds > along and 1 <= reads <= rounds
    alone = measurer.measure_dense(image[1:].copy(), lab[1:].copy(), steps=4, max_label=int(lab.max()), want_planes=True)
    assert measurer.last_rounds()[0] < rounds            # the noise alone settles sooner: in the batch the corridor kept the rounds going
    assert all(np.array_equal(a[0], g[1]) for a, g in zip(alone, got))


# ---- more fixed-point cases ---------------------------------------------------------------------------------------------------------------
def test_plateaus_ramps_and_the_ends_of_the_value_range(measurer):
    shape = (70, 300)
    rng = np.random.default_rng(8)
    lab = np.stack([IR.disks(shape, 30, 1), IR.disks(shape, 30, 2)])
    plateaus = np.kron(rng.integers(0, 6, (2, 7, 10)) * 11000, np.ones((1, 10, 30), np.int64)).astype(np.uint16)      # across the tile borders
    ramp = np.broadcast_to((np.arange(300) * 218)[None, None, :], (2,) + shape).astype(np.uint16).copy()            # rises across the whole width
    ramp[1] = ramp[1, :, ::-1] + (np.arange(70) % 3)[:, None]
    ends = (rng.integers(0, 2, (2,) + shape) * 65535).astype(np.uint16)
    ends[1, 20:50, 100:250] = 65535
    ends[1, 30:33, 120:125] = 0
    for name, image, steps in (("plateaus", plateaus, 6), ("ramp", ramp, 5), ("ends", ends, 4)):
        for s in (1, 2):
            want = GR.measure(image, lab, steps=steps, subsample=s)
            same(measurer.measure_dense(image, lab, steps=steps, subsample=s, want_planes=True), want, (name, s))
    assert want[3].max() == 65535 and want[3].min() == 0
    stack = np.stack([plateaus, ramp, ends], axis=-1)     # the three as channels of one call
    same(measurer.measure_dense(stack, lab, steps=4, want_planes=True), GR.measure(stack, lab, steps=4))


# ---- table limits, input kinds and agreement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 4])
@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_every_pixel_its_own_label_overflows_the_table_in_lds(measurer, shape, nc):
    H, W = shape
    n = H * W
    lab = np.stack([np.arange(1, n + 1, dtype=np.int32).reshape(shape), np.arange(n, 0, -1, dtype=np.int32).reshape(shape)])
    rr, cc = (x.reshape(-1) for x in np.mgrid[0:H, 0:W])
    for dtype, steps in ((np.uint16, 3), (np.uint8, 2)):
        image = speckled(shape, nc, dtype, H + nc)
        g, s, i, planes = measurer.measure_dense(image, lab, steps=steps, want_planes=True)
        assert np.array_equal(planes, GR.measure(image, lab, steps=steps)[3])
        v = planes.transpose(0, 3, 4, 1, 2).reshape(2, n, steps + 1, nc).astype(np.int64)      # row m of the first image is pixel m
        v[1] = v[1, ::-1]                                # row m of the second image is pixel n - 1 - m
        assert np.array_equal(s, v) and np.array_equal(s[:, :, 0], np.stack([image.reshape(2, n, nc)[0], image.reshape(2, n, nc)[1, ::-1]]))
        assert (g[:, :, 0] == 1).all() and np.array_equal(g[0, :, 1], rr) and np.array_equal(g[1, :, 2], cc[::-1])
        assert np.array_equal(i, planes.astype(np.int64).sum(axis=(3, 4)))
    ex = (lab % 3 == 0).astype(np.int32)
    got = measurer.measure_dense(image, lab, exclude=ex, steps=steps)
    keep = (ex.reshape(2, n) == 0)
    keep[1] = keep[1, ::-1]
    assert np.array_equal(got[0][:, :, 0], keep.astype(np.int64)) and np.array_equal(got[1], v * keep[..., None, None]) and np.array_equal(got[2], i)


def test_geometry_and_start_sums_agree_with_cs_label_intensity(measurer):
    shape = (70, 300)
    lab = np.stack([IR.disks(shape, 30, k) for k in (1, 2)])
    image = IR.noise((2,) + shape, 3, np.uint16, 8)
    ex = np.stack([IR.disks(shape, 30, k, radii=(1, 2)) for k in (5, 3)])
    m = int(lab.max())
    inten = IN.IntensityMeasurer(0, extractor=measurer)
    for e in (None, ex):
        for s, masked in ((1, False), (2, False), (1, True)):
            g, su, _ = measurer.measure_dense(image, lab, exclude=e, max_label=m, steps=2, subsample=s, masked=masked)
            geom, stats = inten.measure_dense(image, lab, exclude=e, max_label=m)
            assert np.array_equal(geom, g)               # cs_label_intensity's geom, bit for bit
            if s == 1:                                   # on the objects' own pixels the mask changes nothing
                assert np.array_equal(su[:, :, 0, :], stats[..., 0])


def test_repeatability_batches_and_input_kinds(measurer):
    import torch
    shape = (70, 300)
    lab = np.stack([IR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([IR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    m = int(lab.max())
    for nc, dtype, kw in ((3, np.uint16, dict(steps=4)), (4, np.uint8, dict(steps=3, subsample=2, masked=True)), (1, np.uint16, dict(steps=5, subsample=4))):
        image = np.concatenate([speckled(shape, nc, dtype, 12), IR.noise((1,) + shape, nc, dtype, 13)])
        a = measurer.measure_dense(image, lab, exclude=ex, want_planes=True, **kw)
        b = measurer.measure_dense(image, lab, exclude=ex, want_planes=True, **kw)
        same(a, GR.measure(image, lab, ex, **kw))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))      # bit-identical run to run
        t = measurer.last_timing()
        assert set(t) == {"granularity_prepare_ms", "granularity_steps_ms", "granularity_sums_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        rounds, reads = measurer.last_rounds()
        assert rounds >= kw["steps"] and kw["steps"] <= reads <= rounds
        for k in range(3):                               # an image alone equals its rows in the batch
            one = measurer.measure_dense(image[k:k + 1].copy(), lab[k:k + 1].copy(), exclude=ex[k:k + 1].copy(), max_label=m, want_planes=True, **kw)
            assert all(np.array_equal(x[0], y[k]) for x, y in zip(one, a))
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex), want_planes=True, **kw), a)      # CUDA tensors in
        if dtype == np.uint16:                           # uint16 as int16 views, and as uint16 tensors
            assert as_tensor(image).dtype == torch.int16
            same(measurer.measure_dense(as_tensor(image).view(torch.uint16), as_tensor(lab), **kw), GR.measure(image, lab, **kw))
    g, s, i = measurer.measure_dense(image, lab, max_label=m + 100, **kw)     # a larger table: the same rows, zeros behind them
    assert np.array_equal(s[:, :m], measurer.measure_dense(image, lab, **kw)[1]) and not g[:, m:].any() and not s[:, m:].any()
    with pytest.raises(TypeError):
        measurer.measure_dense(image, as_tensor(lab))


def test_tables_left_on_the_device_equal_the_host_tables(measurer):
    import torch
    shape = (40, 264)
    lab = batch_of(shape, 6)[0][1]
    image = speckled(shape, 3, np.uint16, 11)
    m, steps = int(lab.max()), 3
    want = measurer.measure_dense(image, lab, steps=steps, subsample=2, want_planes=True)
    same(want, GR.measure(image, lab, steps=steps, subsample=2))
    dev = torch.device("cuda", 0)
    outs = [torch.full(w.shape, -5, dtype={np.int64: torch.int64, np.uint16: torch.int16}[w.dtype.type], device=dev) for w in want]
    t_img, t_lab = as_tensor(image), as_tensor(lab)
    prm = GA.granularity_params(steps, 2)
    torch.cuda.synchronize()
    L.check(measurer._lib.cs_label_granularity(measurer._handle, t_img.data_ptr(), 1, 3, t_lab.data_ptr(), None, 2, shape[0], shape[1], L.CS_MEM_DEVICE, m,
                                               C.byref(prm), *(o.data_ptr() for o in outs), L.CS_MEM_DEVICE))
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

    for nc, dtype, kw in ((3, np.uint8, dict(steps=2, masked=True)), (2, np.uint8, dict(steps=2, subsample=4)), (4, np.uint16, dict(steps=2, subsample=2, masked=True)),
                          (1, np.uint16, dict(steps=3)), (3, np.uint16, dict(steps=2, subsample=8, masked=True))):
        image = speckled(shape, nc, dtype, 10)
        want = GR.measure(image, lab, ex, **kw)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=as_tensor(ex), **kw), want)           # all aligned: wide loads
        same(measurer.measure_dense(shifted(image, 1), as_tensor(lab), exclude=as_tensor(ex), **kw), want)
        same(measurer.measure_dense(as_tensor(image), shifted(lab, 1), exclude=as_tensor(ex), **kw), want)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), exclude=shifted(ex, 3), **kw), want)


# ---- error statuses ----------------------------------------------------------------------------------------------------------------------
def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    lab = batch_of(shape, 5)[0][1]
    image = IR.noise((2,) + shape, 3, np.uint8, 1)
    m = int(lab.max())
    want = GR.measure(image, lab, steps=2, max_label=m)
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 0, 256), m + 1), ((1, 16, 0), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                               # range-checked on the device: never an index or a key
        for args in ((image, bad), (as_tensor(image), as_tensor(bad))):
            for kw in (dict(), dict(subsample=4, masked=True)):
                with pytest.raises(L.CellScreenError) as ei:
                    measurer.measure_dense(*args, steps=2, max_label=m, **kw)
                assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            with pytest.raises(L.CellScreenError):      # whatever exclude holds there
                measurer.measure_dense(*args, exclude=(np.ones_like(lab) if isinstance(args[1], np.ndarray) else as_tensor(np.ones_like(lab))),
                                       steps=2, max_label=m)
            same(measurer.measure_dense(image, lab, steps=2, max_label=m), want)
    neg = np.zeros_like(lab)
    neg[0, 2, 2] = -3
    with pytest.raises(L.CellScreenError):
        measurer.measure_batch(image, neg)               # max_label=None on a batch without objects


def test_bad_arguments_are_refused_before_the_device_is_touched(measurer):
    lib, h = measurer._lib, measurer._handle            # a live handle: the refusals are the arguments' own
    zeros = np.zeros(64, np.int32)
    outs = [np.empty(4096, dt) for dt in (np.int64, np.int64, np.int64)]
    prm = L.CSGranularityParams()

    def status(channels=1, steps=4, subsample=1, masked=0, reserved=0, B=1, max_label=1):
        prm.steps, prm.subsample, prm.masked, prm.reserved = steps, subsample, masked, reserved
        for o in outs:
            o[:] = -5
        rc = lib.cs_label_granularity(h, zeros.ctypes.data, 0, channels, zeros.ctypes.data, None, B, 2, 2, 0, max_label, C.byref(prm),
                                      *(o.ctypes.data for o in outs), None, 0)
        assert rc == 0 or all((o == -5).all() for o in outs)             # a refused call wrote nothing
        return rc, lib.cs_last_error().decode()

    assert status()[0] == 0 and status(steps=64, channels=4, subsample=8, masked=1)[0] == 0
    assert status(channels=0)[0] == -1 and status(channels=5)[0] == -6 and "at most 4" in status(channels=5)[1]
    assert status(steps=0)[0] == -1 and status(steps=65)[0] == -6 and "at most 64 steps" in status(steps=65)[1]
    assert status(subsample=3)[0] == -1 and status(subsample=0)[0] == -1 and status(reserved=1)[0] == -1 and status(masked=2)[0] == -1
    rc, text = status(channels=4, steps=64, max_label=1 << 20)           # 2^20 x 65 x 4 x 8 bytes
    assert rc == -6 and "split the batch" in text
    lab = np.ones((1, 4, 4), np.int32)
    image = IR.noise((1, 4, 4), 2, np.uint8, 1)
    for kw, exc in ((dict(steps=0), ValueError), (dict(steps=65), ValueError), (dict(steps=4.0), TypeError), (dict(steps=True), TypeError),
                    (dict(subsample=3), ValueError), (dict(subsample=2.0), TypeError), (dict(masked=1), TypeError)):
        with pytest.raises(exc):
            measurer.measure_dense(image, lab, **kw)
    with pytest.raises(ValueError):
        measurer.measure_dense(np.zeros((1, 4, 4, 5), np.uint8), lab)
    with pytest.raises(ValueError, match="split the batch"):
        measurer.measure_dense(np.zeros((1, 1, 1, 4), np.uint8), np.zeros((1, 1, 1), np.int32), max_label=1 << 20, steps=64)
    same(measurer.measure_dense(image, lab, steps=3, want_planes=True), GR.measure(image, lab, steps=3))     # and the measurer works


# ---- on one handle ------------------------------------------------------------------------------------------------------------------------
def speckle_scene():
    """uint16 [2,96,128,2]: five smooth bright blobs per image on a noisy background in channel 0; channel 1 is 3 x 3 speckles on zero,
    one every 6 pixels either way, clear of the border."""
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.zeros((2, H, W, 2), np.uint16)
    for b in range(2):
        f = 300.0 + rng.normal(0.0, 10.0, (H, W))
        for y, x, r in ((24, 25, 9), (30, 80, 12), (70, 40, 10), (70, 100, 7 + 4 * b), (50, 62, 5)):
            d = np.sqrt((yy - y) ** 2 + (xx - x) ** 2)
            f += 4000.0 * np.exp(-((d * d / (2.0 * (r / 1.6) ** 2)) ** 2))
        imgs[b, :, :, 0] = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
        spots = (yy % 6 >= 2) & (yy % 6 < 5) & (xx % 6 >= 2) & (xx % 6 < 5)  # none at the image's border, where a corner holds out longer
        imgs[b, :, :, 1] = spots * rng.integers(500, 3000, (H // 6 + 1, W // 6 + 1))[yy // 6, xx // 6]
    return imgs


def test_segment_expand_measure_on_one_handle():
    import torch
    imgs = speckle_scene()
    dev = as_tensor(imgs)
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)                    # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)          # left on the device too: no host copy in between
    meas = GA.GranularityMeasurer(0, extractor=seg)
    whole = meas.measure_batch(dev, grown, steps=8)
    ring = meas.measure_batch(dev, grown, exclude=labels, steps=8)
    assert meas._pre is None                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(whole) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (whole, (h_grown, None))):
        d = GR.derive(*GR.measure(imgs, lab, ex, steps=8)[:3])
        assert all(np.array_equal(getattr(t, k), v, equal_nan=v.dtype.kind == "f") for k, v in d.items())
    # the 3 x 3 speckles go at step 2, all of them; the smooth blobs lose little before step 3
    assert (whole.spectrum[:, 1, 1] == 100.0).all() and (np.delete(whole.spectrum[:, :, 1], 1, axis=1) == 0.0).all()
    assert (whole.image_spectrum[:, 1, 1] == 100.0).all()
    assert (whole.spectrum[:, 2:, 0].sum(axis=1) > 4.0 * whole.spectrum[:, :2, 0].sum(axis=1)).all()
    t = meas.last_timing()
    assert len(t) == 3 and all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
