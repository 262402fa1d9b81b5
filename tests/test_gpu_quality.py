"""The image and per-object focus and saturation records on the device (cs_image_quality and cs_object_focus through
cellscreen.quality) against the CPU restatement of tests/quality_reference.py, which tests/test_quality_cpu.py holds to SciPy.

Every table is integers, so every comparison is np.array_equal: no tolerances, the rows of absent objects and the tiles of the
mesh included.

A lane of either pass owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows, and the stencil's side neighbours come
from the next lanes: SHAPES has the sides without an interior, the smallest with one, and 64 x 256 one short, equal, one and two
past in both axes, so that the stencil crosses lanes, waves and workgroup tiles.  Widths that are no multiple of 4 take the
narrow loads.  Mesh tiles of 16, 17, 64 and 256 on 130 x 515 put the mesh's borders off the workgroup tile's (and, at 16, more
mesh tiles under a workgroup than its table in LDS holds).  With every pixel an object of its own, 64 x 256 and 70 x 300 put more
objects under a workgroup than lf_pass's table in LDS has slots, at one, three and four channels."""
import functools

import numpy as np
import pytest

import intensity_reference as IR
import quality_reference as QR
from cellscreen import _lib as L
from cellscreen import intensity as IN
from cellscreen import quality as Q
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 5), (3, 3), (3, 4), (5, 7), (64, 256), (65, 257), (66, 260), (130, 515)]
FOCUS_OF_RECORD = [8, 9, 10, 11, 12]


@pytest.fixture(scope="module")
def measurer():
    m = Q.ImageQualityMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    a = a if a.flags.writeable else a.copy()                             # the cached inputs are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def image_of(shape, nc, dtype, seed, batch=2):
    a = QR.noise((batch,) + shape, nc, dtype, seed)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def want_image(shape, nc, dtype, seed, tile=0, sat=None):
    return QR.measure_image(image_of(shape, nc, dtype, seed), tile, sat)


def same_image(got, want):
    (r, m), (wr, wm) = got, want
    assert r.dtype == np.int64 and r.shape == wr.shape and np.array_equal(r, wr)
    assert (m is None and wm is None) or (m.dtype == np.int64 and m.shape == wm.shape and np.array_equal(m, wm))


def same_objects(got, want):
    (g, f), (wg, wf) = got, want
    assert g.dtype == f.dtype == np.int64 and g.shape == wg.shape and f.shape == wf.shape
    assert np.array_equal(g, wg) and np.array_equal(f, wf)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_image_records_equal_the_restatement(measurer, shape, dtype):
    for nc in (1, 2, 3, 4):
        seed = 11 * shape[0] + shape[1] + nc
        got = measurer.measure_batch_dense(image_of(shape, nc, dtype, seed))
        same_image(got, want_image(shape, nc, dtype, seed))
        if shape[0] < 3 or shape[1] < 3:
            assert not got[0][:, :, 8:].any()
    one = image_of(shape, 1, dtype, 5)[..., 0]                            # [B,H,W]: one channel
    same_image(measurer.measure_batch_dense(one), QR.measure_image(one))


@pytest.mark.parametrize("tile", [16, 17, 64, 256])
def test_mesh_equals_the_restatement_and_sums_to_the_image(measurer, tile):
    shape = (130, 515)
    for nc, dtype in ((1, np.uint16), (3, np.uint8), (4, np.uint16)):
        rec, mesh = measurer.measure_batch_dense(image_of(shape, nc, dtype, 77 + nc), tile=tile)
        same_image((rec, mesh), want_image(shape, nc, dtype, 77 + nc, tile))
        assert mesh.shape == (2, nc) + QR.mesh_dims(*shape, tile) + (8,)
        assert np.array_equal(mesh.sum(axis=(2, 3)), rec[:, :, [0, 1, 2, 8, 9, 10, 11, 12]])
    shape = (66, 260)                                                    # a width that takes the wide loads, with a mesh
    same_image(measurer.measure_batch_dense(image_of(shape, 2, np.uint16, 9), tile=tile), want_image(shape, 2, np.uint16, 9, tile))
    t = measurer.measure_batch(image_of(shape, 2, np.uint16, 9), tile=tile)
    w = Q.image_quality_table(*want_image(shape, 2, np.uint16, 9, tile), tile)
    for k in ("mean", "std", "focus_score", "laplacian_variance", "tenengrad", "brenner", "percent_minimal", "percent_maximal",
              "percent_saturated", "tile_focus_score", "tile_laplacian_variance", "local_focus_score"):
        assert np.array_equal(getattr(t, k), getattr(w, k), equal_nan=True), k


def test_saturation_levels_and_a_constant_image(measurer):
    shape = (65, 257)
    for nc, dtype, sat in ((3, np.uint16, (65535, 30000, 0)), (4, np.uint8, (256, 255, 128, 1)), (1, np.uint16, (65536,))):
        image = image_of(shape, nc, dtype, 21)
        rec, _ = measurer.measure_batch_dense(image, sat_level=list(sat))
        same_image((rec, None), want_image(shape, nc, dtype, 21, 0, sat))
        for c, s in enumerate(sat):
            assert (rec[:, c, 7] == (image[..., c] >= s).sum(axis=(1, 2))).all()
    rec, _ = measurer.measure_batch_dense(image_of(shape, 2, np.uint8, 22), sat_level=200)          # one level for every channel
    same_image((rec, None), want_image(shape, 2, np.uint8, 22, 0, (200, 200)))
    n, n_int = shape[0] * shape[1], (shape[0] - 2) * (shape[1] - 2)
    for dtype, v in ((np.uint8, 0), (np.uint8, 255), (np.uint16, 65535), (np.uint16, 1234)):
        rec, mesh = measurer.measure_batch_dense(np.full((1,) + shape + (2,), v, dtype), tile=16)
        sat = n if v == QR.top_of(dtype) else 0
        assert rec.tolist() == [[[n, n * v, n * v * v, v, v, n, n, sat, n_int, 0, 0, 0, 0]] * 2]
        assert not mesh[..., 4:].any() and mesh[..., 0].sum() == 2 * n


def object_scene():
    """(labels [2,130,515] int32, exclude, max_label): an object across the workgroup-tile corner at (64, 256), objects to the
    image's borders and corners, one of two far pieces, one with the label max_label, excluded pixels; labels 4..8 are absent."""
    lab = np.zeros((2, 130, 515), np.int32)
    lab[0, 58:71, 249:263] = 1                                           # across the corner of four workgroup tiles
    lab[0, 0:6, 0:9] = 2                                                 # the top left corner
    lab[0, 10:15, 300:306] = 3                                           # two far pieces
    lab[0, 120:126, 20:27] = 3
    lab[0, 125:130, 507:515] = 9                                         # the bottom right corner, the label max_label
    lab[1] = np.roll(lab[0], (3, 5), axis=(0, 1))
    lab[1, :, 0] = 2                                                     # the whole left border
    lab[1, 129, :] = 1                                                   # the whole bottom border
    ex = np.zeros_like(lab)
    ex[0, 60:64, 255:258] = 7                                            # a hole at the tile corner
    ex[0, 0, :] = -1                                                     # the top row of every object that has one
    ex[1, 100:, 3:9] = 1
    return lab, ex, 9


def test_object_focus_equals_the_restatement_and_geom_equals_intensity(measurer):
    lab, ex, m = object_scene()
    im = IN.IntensityMeasurer(0, extractor=None)
    for nc, dtype in ((1, np.uint16), (2, np.uint8), (3, np.uint16), (4, np.uint8), (4, np.uint16)):
        image = image_of(lab.shape[1:], nc, dtype, 60 + nc)
        for e in (None, ex):
            got = measurer.measure_objects_dense(image, lab, exclude=e, max_label=m)
            same_objects(got, QR.measure_objects(image, lab, e, m))
            assert np.array_equal(got[0], im.measure_dense(image, lab, exclude=e, max_label=m)[0])     # geom, bit for bit
            assert not got[0][:, 3:8].any() and not got[1][:, 3:8].any() and got[0][:, 8, 0].all()   # absent rows, the last label
        t = measurer.measure_objects(image, lab, exclude=ex, max_label=m)
        w = Q.object_focus_table(*QR.measure_objects(image, lab, ex, m))
        assert len(t) == len(w) == 8 and all(np.array_equal(getattr(t, k), getattr(w, k), equal_nan=True)
                                              for k in ("image", "label", "area", "n_interior", "laplacian_variance", "tenengrad", "brenner"))
    im.close()
    for shape in ((1, 1), (2, 5), (3, 4), (5, 7), (64, 256), (65, 257)):  # every pixel an object of its own row: the small sides
        image = image_of(shape, 2, np.uint16, 3)
        rows = np.broadcast_to(np.arange(1, shape[0] + 1, dtype=np.int32)[None, :, None], (2,) + shape).copy()
        same_objects(measurer.measure_objects_dense(image, rows), QR.measure_objects(image, rows))
    whole = np.ones((2, 66, 260), np.int32)                              # one object over the image: the image's own focus sums
    image = image_of((66, 260), 3, np.uint8, 4)
    _, f = measurer.measure_objects_dense(image, whole)
    assert np.array_equal(f[:, 0], want_image((66, 260), 3, np.uint8, 4)[0][:, :, FOCUS_OF_RECORD])


@pytest.mark.parametrize("shape", [(64, 256), (70, 300)])
def test_every_pixel_its_own_label_overflows_the_table_in_lds(measurer, shape):
    """lf_pass keeps the objects of a 64 x 256 tile in a table in LDS, 512 slots at one channel and 256 above; what finds no slot
    within 16 probes goes straight to the dense tables (lf_insert -> lf_global).  With every pixel an object of its own a full
    tile holds 16384: most of them take the direct way."""
    H, W = shape
    n = H * W
    lab = np.stack([np.arange(1, n + 1, dtype=np.int32).reshape(shape), np.arange(n, 0, -1, dtype=np.int32).reshape(shape)])
    ex = (lab % 3 == 0).astype(np.int32)
    assert min(H, 64) * min(W, 256) > 512
    for nc in (1, 3, 4):
        image = image_of(shape, nc, np.uint16, 40 + nc)
        for e in (None, ex):
            got = measurer.measure_objects_dense(image, lab, exclude=e, max_label=n)
            same_objects(got, QR.measure_objects(image, lab, e, n))
            assert got[0][:, :, 0].max() == 1 and (e is None) == bool((got[0][:, :, 0] == 1).all())
        interior = np.zeros(shape, bool)
        interior[1:-1, 1:-1] = True                                      # n_int of a one-pixel object: whether the pixel is interior
        assert np.array_equal(got[1][0, :, 0, 0].reshape(shape) == 1, interior & (ex[0] == 0))


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    lab, ex, m = object_scene()
    image = image_of(lab.shape[1:], 2, np.uint16, 8)
    want = QR.measure_objects(image, lab, ex, m)
    for where, value in (((0, 0, 0), -1), ((1, 129, 514), -7), ((0, 64, 256), m + 1), ((1, 3, 100), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                                               # range-checked on the device: never an index
        for args in ((image, bad, ex), (as_tensor(image), as_tensor(bad), as_tensor(ex))):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_objects_dense(args[0], args[1], exclude=args[2], max_label=m)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            same_objects(measurer.measure_objects_dense(image, lab, exclude=ex, max_label=m), want)


def test_the_largest_sums_against_closed_forms(measurer):
    side, top = 4096, 65535
    n, inner = side * side, side - 2
    n_int = inner * inner
    rec, mesh = measurer.measure_batch_dense(QR.checkerboard((side, side), np.uint16)[None], tile=1024)
    # L = +-4 top at every interior pixel, as many of either sign; G = Br = 0: sum L^2 at its proved maximum (4 top)^2 n_int
    assert rec.tolist() == [[[n, n // 2 * top, n // 2 * top * top, 0, top, n // 2, n // 2, n // 2, n_int, 0, 16 * top * top * n_int, 0, 0]]]
    assert mesh.shape == (1, 1, 4, 4, 8) and np.array_equal(mesh.sum(axis=(2, 3))[0, 0], rec[0, 0, [0, 1, 2, 8, 9, 10, 11, 12]])
    assert (mesh[0, 0, :, :, 0] == 1024 * 1024).all() and mesh[0, 0, 1, 1].tolist()[3:] == [1 << 20, 0, 16 * top * top << 20, 0, 0]
    t = Q.image_quality_table(rec, mesh, 1024)
    assert t.laplacian_variance[0, 0] == float(16 * top * top) and t.tenengrad[0, 0] == 0.0 and t.percent_maximal[0, 0] == 50.0
    stripes = QR.stripes4((side, side), np.uint16)[None]
    rec, _ = measurer.measure_batch_dense(stripes, sat_level=[1])
    cols = np.arange(1, side - 1) % 4                                    # columns 0, 0, top, top: L = +top on the dark, -top on the lit
    sl = inner * top * int(((cols < 2).sum() - (cols >= 2).sum()))
    assert rec.tolist() == [[[n, n // 2 * top, n // 2 * top * top, 0, top, n // 2, n // 2, n // 2, n_int, sl, top * top * n_int,
                              16 * top * top * n_int, top * top * n_int]]]
    _, f = measurer.measure_objects_dense(stripes, np.ones((1, side, side), np.int32))          # one object over the cap plane
    assert f.tolist() == [[[rec[0, 0, FOCUS_OF_RECORD].tolist()]]]


def test_repeatability_batch_independence_and_input_kinds(measurer):
    import torch
    shape = (66, 260)
    image = image_of(shape, 3, np.uint16, 31, batch=3).copy()
    lab = np.stack([IR.disks(shape, 20, k) for k in (1, 2, 3)])
    a = measurer.measure_batch_dense(image, tile=17, sat_level=[9, 99, 999])
    b = measurer.measure_batch_dense(image, tile=17, sat_level=[9, 99, 999])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()                    # the same call twice
    oa = measurer.measure_objects_dense(image, lab)
    ob = measurer.measure_objects_dense(image, lab)
    assert oa[0].tobytes() == ob[0].tobytes() and oa[1].tobytes() == ob[1].tobytes()
    t = measurer.last_timing()
    assert set(t) == {"quality_clear_ms", "quality_pass_ms", "focus_clear_ms", "focus_pass_ms"}
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
    same_image(measurer.measure_batch_dense(as_tensor(image), tile=17, sat_level=[9, 99, 999]), a)      # CUDA tensors in
    same_image(measurer.measure_batch_dense(as_tensor(image).view(torch.uint16), tile=17, sat_level=[9, 99, 999]), a)
    same_objects(measurer.measure_objects_dense(as_tensor(image), as_tensor(lab)), oa)
    other = image.copy()                                                 # image 1 alone differs: images 0 and 2 keep their records
    other[1] = other[1][::-1, ::-1] // 2
    c = measurer.measure_batch_dense(other, tile=17, sat_level=[9, 99, 999])
    oc = measurer.measure_objects_dense(other, lab)
    for k in (0, 2):
        assert np.array_equal(c[0][k], a[0][k]) and np.array_equal(c[1][k], a[1][k])
        assert np.array_equal(oc[0][k], oa[0][k]) and np.array_equal(oc[1][k], oa[1][k])
    assert not np.array_equal(c[0][1], a[0][1]) and not np.array_equal(oc[1][1], oa[1][1])
    same_image(c, QR.measure_image(other, 17, [9, 99, 999]))
    for k in range(3):                                                   # an image alone equals its rows in the batch
        r, m = measurer.measure_batch_dense(image[k:k + 1].copy(), tile=17, sat_level=[9, 99, 999])
        assert np.array_equal(r[0], a[0][k]) and np.array_equal(m[0], a[1][k])
    with pytest.raises(TypeError):
        measurer.measure_objects_dense(image, as_tensor(lab))
    with pytest.raises(ValueError):
        measurer.measure_batch_dense(as_tensor(image)[:, :, ::2])


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


def test_segment_quality_intensity_on_one_handle(measurer):
    import torch
    imgs = nuclei_scene()
    dev = as_tensor(imgs)
    alone_seg = S.ThresholdSegmenter(0)
    alone_labels = alone_seg.segment_batch(dev, channel=0)[0].cpu().numpy()
    alone_seg.close()
    alone_quality = measurer.measure_batch_dense(imgs, tile=32)
    alone_focus = measurer.measure_objects_dense(imgs, alone_labels)
    alone_in = IN.IntensityMeasurer(0)
    alone_tables = alone_in.measure_dense(imgs, alone_labels)
    alone_in.close()

    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)              # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    shared = Q.ImageQualityMeasurer(0, extractor=seg)
    quality = shared.measure_batch_dense(dev, tile=32)
    focus = shared.measure_objects_dense(dev, labels)
    host_quality = shared.measure_batch_dense(imgs, tile=32)             # host planes go through the shared uploads
    meas = IN.IntensityMeasurer(0, extractor=seg)
    tables = meas.measure_dense(dev, labels)
    assert shared._pre is None and meas._pre is None                     # the segmenter's handle did the work
    assert np.array_equal(labels.cpu().numpy(), alone_labels) and int(n_labels.sum()) == 10
    same_image(quality, alone_quality)
    same_image(host_quality, alone_quality)
    same_image(quality, QR.measure_image(imgs, 32))
    same_objects(focus, alone_focus)
    same_objects(focus, QR.measure_objects(imgs, alone_labels))
    assert np.array_equal(tables[0], alone_tables[0]) and np.array_equal(tables[1], alone_tables[1])
    assert np.array_equal(focus[0], tables[0])                           # geom, bit for bit
    labels2 = seg.segment_batch(dev, channel=0)[0]                       # the segmenter after the measurers: the same labels
    assert np.array_equal(labels2.cpu().numpy(), alone_labels)
    q = Q.image_quality_table(*quality, 32)
    assert (q.tenengrad[:, 1] > q.tenengrad[:, 0]).all()                 # noise is sharper than blobs
    seg.close()
