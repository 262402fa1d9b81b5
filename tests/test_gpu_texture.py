"""The per-object texture records on the device (cs_label_texture through cellscreen.texture) against the CPU restatement of
tests/texture_reference.py, which tests/test_texture_cpu.py holds to its slow form and to Haralick's double sums.

count, marg, sumsq and glcm are integers: np.array_equal on the dense tables, the rows of absent objects included.  clogc, the
one float, is held to |dev - ref| <= 2^-40 * ref with ref the math.fsum of the float64 terms G * log2(G).  The bound is derived,
not measured: every term is non-negative, there are at most 4096 of them, log2 is within 3 ulp (OpenCL's bound), the device takes
one product per term and up to 4095 additions, the reference rounds each term twice; together under 4104 * 2^-53, half of 2^-40.

A lane of the box pass owns 4 columns x 16 rows, a wave 256 columns, a workgroup 64 rows; SHAPES crosses the 16 rows, the 64 rows
and the 256 columns one short, equal and one past, and has the single row, the single column and the single pixel.  Widths that
are no multiple of 4 take the scalar path.  A tile's table in LDS has 1024 slots: an image where every pixel is its own label
fills it.  The matrix pass gives a workgroup 256 pixels per step, a row of a wide box or several rows of a narrow one: the boxes
here are 1 to 4096 wide."""
import functools
import math

import numpy as np
import pytest

import texture_reference as TR
from cellscreen import _lib as L
from cellscreen import expand as EX
from cellscreen import segment as S
from cellscreen import texture as TX

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 255), (16, 256), (17, 257), (63, 255), (65, 257), (1, 1)]
DL = [(1, 8), (3, 32), (5, 64)]                                          # (distance, levels)
CLOGC_REL = 2.0 ** -40


@pytest.fixture(scope="module")
def measurer():
    m = TX.TextureMeasurer(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def batch_of(shape, seed):
    """(name, labels int32 [2,H,W]) per kind of content, the two images different."""
    out = []
    for (name, a), (_, b) in zip(TR.contents(shape, seed), TR.contents(shape, seed + 1)):
        lab = np.stack([a, b[::-1, ::-1] if name == "two pieces" else b])
        if name == "two pieces":
            lab[1][lab[1] > 0] = 2
            lab[1, shape[0] // 2, shape[1] // 2] = 5
        lab.flags.writeable = False
        out.append((name, lab))
    return out


def ranges_of(image, value_range):
    nc = image.shape[3] if image.ndim == 4 else 1
    if value_range is None:
        return TR.full_range(image.dtype, nc)
    return [tuple(value_range)] * nc if isinstance(value_range[0], int) else [tuple(r) for r in value_range]


def same(got, want, what=""):
    """device records against reference records: integers equal, clogc within its derived bound"""
    assert len(got) == len(want) == 5, what
    for k, dt in ((0, np.int32), (1, np.int32), (2, np.int64), (4, np.int32)):
        g, w = got[k], want[k]
        assert (g is None) == (w is None), what
        if g is not None:
            assert g.dtype == w.dtype == dt and g.shape == w.shape, (what, k)
            assert np.array_equal(g, w), (what, k)
    g, w = got[3], want[3]
    assert g.dtype == w.dtype == np.float64 and g.shape == w.shape, what
    err = np.abs(g - w)
    print(f"clogc {what}: largest |dev - ref| / ref = {float(np.max(err[w > 0] / w[w > 0], initial=0.0)):.3e}")
    assert (err <= CLOGC_REL * w).all(), what


def check(measurer, image, lab, d, levels, value_range=None, exclude=None, max_label=None, glcm=True, what=""):
    """measure_dense against the restatement; returns the device's records"""
    got = measurer.measure_dense(image, lab, d, levels, value_range, exclude, max_label, glcm)
    same(got, TR.measure(image, lab, d, levels, ranges_of(image, value_range), exclude, max_label, glcm), what)
    return got


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_records_equal_the_restatement_across_the_tiles(measurer, shape, dtype):
    seed = 7 * shape[0] + shape[1]
    for k, nc in enumerate((1, 3, 4)):
        d, levels = DL[(k + (dtype == np.uint16)) % 3]                   # every (d, L) meets every channel count over the two dtypes but one
        image = TR.noise((2,) + shape, nc, dtype, seed + nc)
        for name, lab in batch_of(shape, seed):
            got = check(measurer, image, lab, d, levels, what=f"{shape} {name} C{nc} d{d} L{levels}")
    t = measurer.measure_batch(image, lab, d, levels)
    want = TR.derive(*got[:4], levels)
    assert len(t) == len(want["label"]) and t.levels == levels and t.features.shape == (len(t), nc, 4, 13)
    assert all(np.array_equal(getattr(t, k), v, equal_nan=True) for k, v in want.items())
    one = TR.noise((2,) + shape, 1, dtype, seed)[..., 0]                 # [B,H,W]: one channel, and no matrices
    got = measurer.measure_dense(one, batch_of(shape, seed)[0][1], 1, 8)
    assert got[4] is None
    same(got, TR.measure(one, batch_of(shape, seed)[0][1], 1, 8, TR.full_range(dtype, 1)), "one channel")


def test_borders_and_directions(measurer):
    # one object fills the image: every direction meets every border, (d, -d) at column 0 included
    for shape, dist in (((20, 30), (1, 3, 19)), ((20, 30), (25,)), ((30, 20), (25,)), ((20, 30), (40,)), ((7, 5), (4, 6))):
        H, W = shape
        image = TR.noise((1,) + shape, 2, np.uint8, H + W)
        lab = np.ones((1,) + shape, np.int32)
        for d in dist:
            c, m, s, cl, g = check(measurer, image, lab, d, 16, what=f"{shape} d{d}")
            n = m[0, 0, :, :, :16].sum(axis=-1)                          # [C,4]: N per direction
            want = [2 * max(0, H - dr * d) * max(0, W - abs(dc) * d) for dr, dc in TR.STEPS]
            assert n.tolist() == [want, want], (shape, d)
            for k in range(4):
                if want[k] == 0:                                         # d past the height, the width or both: all-zero records
                    assert not m[0, 0, :, k].any() and not s[0, 0, :, k].any() and not cl[0, 0, :, k].any() and not g[0, 0, :, k].any()
    image = TR.noise((1, 128, 130), 1, np.uint16, 9)
    c, m, s, cl, g = check(measurer, image, np.ones((1, 128, 130), np.int32), 127, 32, what="d = 127")
    assert m[0, 0, 0, :, :32].sum(axis=-1).tolist() == [2 * 128 * 3, 2 * 1 * 3, 2 * 1 * 130, 2 * 1 * 3]


def test_neighbours(measurer):
    H, W = 24, 40
    image = TR.noise((1, H, W), 1, np.uint8, 4)
    lab = np.ones((1, H, W), np.int32)
    lab[0, :, 20:] = 2                                                   # two objects that touch along a straight edge
    for d in (1, 2):
        c, m, s, cl, g = check(measurer, image, lab, d, 8, what=f"touching d{d}")
        n = m[0, :, 0, :, :8].sum(axis=-1)                               # [2,4]
        want = [2 * (H - dr * d) * (20 - abs(dc) * d) for dr, dc in TR.STEPS]   # each half on its own: no pair crosses the edge
        assert n.tolist() == [want, want]
    for d in (3, 9):                                                     # a disconnected object: two columns d apart pair with each other
        lab = np.zeros((1, H, W), np.int32)
        lab[0, :, 5] = 1
        lab[0, :, 5 + d] = 1
        c, m, s, cl, g = check(measurer, image, lab, d, 8, what=f"two pieces d{d}")
        assert m[0, 0, 0, :, :8].sum(axis=-1).tolist() == [2 * H, 2 * (H - d), 4 * (H - d), 2 * (H - d)]
    shape = (64, 256)                                                    # every pixel its own label: no pairs, the boxes single pixels
    lab = np.arange(1, 64 * 256 + 1, dtype=np.int32).reshape((1,) + shape)
    image = TR.noise((1,) + shape, 2, np.uint16, 5)
    c, m, s, cl, g = measurer.measure_dense(image, lab, 1, 8, glcm=True)
    assert (c == 1).all() and not m.any() and not s.any() and not cl.any() and not g.any()
    assert m.shape == (1, 64 * 256, 2, 4, 32) and g.shape == (1, 64 * 256, 2, 4, 8, 8)
    t = TX.texture_table(c, m, s, cl, 8)
    assert len(t) == 64 * 256 and np.isnan(t.features).all() and np.isnan(t.mean).all() and not t.pairs.any()


def test_exclude(measurer):
    shape = (70, 300)
    nuclei = np.stack([TR.disks(shape, 30, 1, radii=(2, 4)), TR.disks(shape, 30, 2, radii=(2, 4))])
    cells = np.stack([TR.disks(shape, 30, 1, radii=(5, 9)), TR.disks(shape, 30, 3, radii=(5, 9))])
    for nc, dtype, d, levels in ((1, np.uint8, 1, 8), (3, np.uint16, 2, 32)):
        image = TR.noise((2,) + shape, nc, dtype, 5 + nc)
        ring = check(measurer, image, cells, d, levels, exclude=nuclei, what="rings")     # cells with their nuclei excluded
        whole = check(measurer, image, cells, d, levels, what="whole cells")
        assert not np.array_equal(ring[0], whole[0]) and (ring[1][..., :levels].sum(axis=-1) <= whole[1][..., :levels].sum(axis=-1)).all()
        big = (nuclei * 1000003).astype(np.int32) - (nuclei % 2) * 7      # any non-zero value excludes, negative ones too
        same(measurer.measure_dense(image, cells, d, levels, exclude=big, glcm=True), ring, "any non-zero value")
        same(measurer.measure_dense(image, cells, d, levels, exclude=np.zeros_like(cells), glcm=True), whole, "an all-zero exclude")
        got = measurer.measure_dense(image, cells, d, levels, exclude=cells, glcm=True)   # swallowed whole: all zero
        assert all(not x.any() for x in got) and got[1].shape == whole[1].shape
        t = measurer.measure_batch(image, cells, d, levels, exclude=cells)
        assert len(t) == 0 and t.features.shape == (0, nc, 4, 13) and t.mean.shape == (0, nc, 13) and t.pairs.shape == (0, nc, 4)
    # a pair with an excluded endpoint is gone: one excluded pixel inside a 5 x 5 object takes 2 pairs out of every direction
    image = TR.noise((1, 5, 5), 1, np.uint8, 2)
    lab = np.ones((1, 5, 5), np.int32)
    ex = np.zeros((1, 5, 5), np.int32)
    ex[0, 2, 2] = -1
    c, m, s, cl, g = check(measurer, image, lab, 1, 4, exclude=ex, what="one excluded pixel")
    assert c.tolist() == [[24]] and m[0, 0, 0, :, :4].sum(axis=-1).tolist() == [2 * (20 - 2), 2 * (16 - 2), 2 * (20 - 2), 2 * (16 - 2)]


def test_quantisation_on_the_device(measurer):
    rng = np.random.default_rng(3)
    image = rng.permutation(65536).astype(np.uint16).reshape(1, 256, 256)          # every uint16 value once
    lab = np.ones((1, 256, 256), np.int32)
    for levels in (64, 7):
        for span in ((0, 65535), (0, 4095), (1000, 50000)):              # the last two clip at the top, the last at the bottom too
            c, m, s, cl, g = check(measurer, image, lab, 1, levels, value_range=span, what=f"L{levels} {span}")
            # direction (0, 1) drops one column of ends: px counts every level about twice; all of them occur
            assert (m[0, 0, 0, 0, :levels] > 0).all()
    two = np.stack([image, image[:, ::-1]], axis=-1)                     # a range per channel
    check(measurer, two, lab, 2, 64, value_range=[(0, 65535), (1000, 50000)], what="two ranges")


def flat_closed_form(side, levels, level, steps=TR.STEPS):
    n = [2 * (side - abs(dr)) * (side - abs(dc)) for dr, dc in steps]
    marg = np.zeros((4, 4 * levels), np.int32)
    marg[:, level] = n
    marg[:, levels + 2 * level] = n
    marg[:, 3 * levels] = n
    return n, marg


def test_contention_one_label_over_a_flat_4096_plane(measurer):
    side, levels = 4096, 64
    image = np.full((1, side, side), 40000, np.uint16)                   # level 40000 * 64 // 65536 = 39
    lab = np.ones((1, side, side), np.int32)
    c, m, s, cl, g = measurer.measure_dense(image, lab, 1, levels, glcm=True)
    n, marg = flat_closed_form(side, levels, 39)                         # N = 2 (4096 - |dr|) (4096 - |dc|), all of it in one cell
    assert c.tolist() == [[side * side]] and np.array_equal(m[0, 0, 0], marg)
    assert s[0, 0, 0].tolist() == [x * x for x in n]
    want = np.zeros((4, levels, levels), np.int32)
    want[:, 39, 39] = n
    assert np.array_equal(g[0, 0, 0], want)
    for k in range(4):                                                   # one term: N log2 N
        ref = n[k] * math.log2(n[k])
        assert abs(cl[0, 0, 0, k] - ref) <= CLOGC_REL * ref
    t = TX.texture_table(c, m, s, cl, levels)
    f = t.features[0, 0]                                                 # flat: ASM 1, contrast 0, correlation 1, entropy 0, both info measures 0
    assert (f[:, 0] == 1).all() and (f[:, 1] == 0).all() and (f[:, 2] == 1).all() and (f[:, 8] == 0).all() and (f[:, 11:] == 0).all()


def test_largest_counts_on_a_plane_of_columns_modulo_64(measurer):
    side, levels = 4096, 64
    image = np.ascontiguousarray(np.broadcast_to((np.arange(side) % 64).astype(np.uint16), (1, side, side)))
    lab = np.ones((1, side, side), np.int32)
    c, m, s, cl, g = measurer.measure_dense(image, lab, 1, levels, value_range=(0, 63), glcm=True)   # the level is the value
    # (0, 1): a row pairs column c with c + 1 for c = 0 .. 4094, levels j = c mod 64 and j + 1 mod 64: 64 such c for j <= 62 and 63
    # for j = 63 (c = 4095 has no partner).  So G[j][j + 1] = G[j + 1][j] = 64 * rows for j = 0 .. 62, G[63][0] = G[0][63] = 63 * rows,
    # rows = 4096; (1, 1) and (1, -1) pair the same columns over 4095 rows.  (1, 0) pairs a column with itself: G[j][j] = 2 * 64 * 4095.
    want = np.zeros((4, levels, levels), np.int64)
    j = np.arange(63)
    for k, rows in ((0, side), (1, side - 1), (3, side - 1)):
        want[k, j, j + 1] = want[k, j + 1, j] = 64 * rows
        want[k, 63, 0] = want[k, 0, 63] = 63 * rows
    want[2, np.arange(64), np.arange(64)] = 2 * 64 * (side - 1)
    assert c.tolist() == [[side * side]] and np.array_equal(g[0, 0, 0], want)
    marg, sumsq, clogc = TR.records(want)
    assert np.array_equal(m[0, 0, 0], marg) and np.array_equal(s[0, 0, 0], sumsq)
    assert (np.abs(cl[0, 0, 0] - clogc) <= CLOGC_REL * clogc).all()
    assert m[0, 0, 0, :, :levels].sum(axis=-1).tolist() == [2 * side * (side - 1), 2 * (side - 1) ** 2, 2 * side * (side - 1), 2 * (side - 1) ** 2]


def test_scalar_path_for_odd_widths_and_unaligned_tensor_views(measurer):
    import torch
    for shape in ((33, 258), (20, 7), (9, 301)):                         # widths that are no multiple of 4
        lab = batch_of(shape, 3)[0][1]
        for nc, dtype in ((3, np.uint8), (2, np.uint16)):
            image = TR.noise((2,) + shape, nc, dtype, 9)
            check(measurer, image, lab, 2, 16, exclude=(lab % 2).astype(np.int32), what=f"{shape} C{nc}")
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
        image = TR.noise((2,) + shape, nc, dtype, 10)
        want = TR.measure(image, lab, 1, 16, TR.full_range(dtype, nc), ex, glcm=True)
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), 1, 16, exclude=as_tensor(ex), glcm=True), want, "aligned")
        same(measurer.measure_dense(shifted(image, 1), as_tensor(lab), 1, 16, exclude=as_tensor(ex), glcm=True), want, "image shifted")
        same(measurer.measure_dense(as_tensor(image), shifted(lab, 1), 1, 16, exclude=as_tensor(ex), glcm=True), want, "labels shifted")
        same(measurer.measure_dense(as_tensor(image), as_tensor(lab), 1, 16, exclude=shifted(ex, 3), glcm=True), want, "exclude shifted")
        same(measurer.measure_dense(shifted(image, 1), shifted(lab, 2), 1, 16, glcm=True),
             TR.measure(image, lab, 1, 16, TR.full_range(dtype, nc), glcm=True), "both shifted")


def test_input_kinds_repeatability_and_batch_independence(measurer):
    shape = (70, 300)
    lab = np.stack([TR.disks(shape, 30, k) for k in (1, 2, 3)])
    ex = np.stack([TR.disks(shape, 30, k, radii=(1, 2)) for k in (1, 5, 3)])
    for nc, dtype, d, levels in ((3, np.uint16, 1, 32), (4, np.uint8, 3, 8)):
        image = TR.noise((3,) + shape, nc, dtype, 12)
        a = check(measurer, image, lab, d, levels, exclude=ex, what="numpy in")
        b = measurer.measure_dense(image, lab, d, levels, exclude=ex, glcm=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))           # bit-identical run to run, clogc included
        t = measurer.last_timing()
        assert set(t) == {"texture_boxes_ms", "texture_matrices_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        dev = measurer.measure_dense(as_tensor(image), as_tensor(lab), d, levels, exclude=as_tensor(ex), glcm=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, dev))         # CUDA tensors in equal numpy in
        if dtype == np.uint16:
            import torch
            check(measurer, image, lab, d, levels, what="no exclude")
            got = measurer.measure_dense(as_tensor(image).view(torch.uint16), as_tensor(lab), d, levels, glcm=True)
            assert all(np.array_equal(x, y) for x, y in zip(got, measurer.measure_dense(image, lab, d, levels, glcm=True)))
        m = int(lab.max())
        for k in range(3):                                               # an image alone equals its rows in the batch
            got = measurer.measure_dense(image[k:k + 1].copy(), lab[k:k + 1].copy(), d, levels, exclude=ex[k:k + 1].copy(), max_label=m, glcm=True)
            assert all(np.array_equal(g[0], x[k]) for g, x in zip(got, a))
        got = measurer.measure_dense(image, lab, d, levels, exclude=ex, max_label=m + 100, glcm=True)   # a larger table: zeros behind the rows
        assert all(np.array_equal(g[:, :m], w) and not g[:, m:].any() for g, w in zip(got, a))
    with pytest.raises(TypeError):
        measurer.measure_dense(image, as_tensor(lab))
    with pytest.raises(ValueError):
        measurer.measure_dense(as_tensor(image)[:, :, ::2], as_tensor(lab)[:, :, ::2])


def test_a_bad_label_is_an_error_status_and_the_handle_stays_usable(measurer):
    shape = (17, 257)
    lab = batch_of(shape, 5)[0][1]
    image = TR.noise((2,) + shape, 3, np.uint8, 1)
    m = int(lab.max())
    want = TR.measure(image, lab, 1, 8, TR.full_range(np.uint8, 3), max_label=m, glcm=True)
    for where, value in (((0, 0, 0), -1), ((1, 16, 256), -7), ((0, 9, 255), m + 1), ((1, 3, 100), 2 ** 31 - 1)):
        bad = lab.copy()
        bad[where] = value                                               # range-checked on the device: never an index
        for args in ((image, bad), (as_tensor(image), as_tensor(bad))):
            with pytest.raises(L.CellScreenError) as ei:
                measurer.measure_dense(*args, 1, 8, max_label=m, glcm=True)
            assert ei.value.status == -1 and "negative or exceeds max_label" in str(ei.value)
            with pytest.raises(L.CellScreenError):                      # whatever exclude holds there
                measurer.measure_dense(*args, 1, 8, exclude=(np.ones_like(lab) if isinstance(args[1], np.ndarray) else as_tensor(np.ones_like(lab))),
                                       max_label=m)
            same(measurer.measure_dense(image, lab, 1, 8, max_label=m, glcm=True), want, "the next good call")
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


def test_segment_expand_texture_on_one_handle():
    import torch
    imgs = nuclei_scene()
    dev = as_tensor(imgs)
    seg = S.ThresholdSegmenter(0)
    labels, n_labels, _ = seg.segment_batch(dev, channel=0)                    # left on the device
    assert isinstance(labels, torch.Tensor) and labels.is_cuda
    grown = EX.LabelExpander(0, extractor=seg).expand_batch(labels, 6)
    meas = TX.TextureMeasurer(0, extractor=seg)
    rng = [(0, 4500), (0, 65535)]                                        # channel 0 holds 300 .. 4300: its levels span the blobs
    ring = meas.measure_batch(dev, grown, 1, 32, rng, exclude=labels)
    nuc = meas.measure_batch(dev, labels, 1, 32, rng)
    assert meas._pre is None                                             # the segmenter's handle did the work
    h_lab, h_grown = labels.cpu().numpy(), grown.cpu().numpy()
    assert len(nuc) == int(n_labels.sum()) == 10 and (h_grown > 0).sum() > (h_lab > 0).sum()
    for t, (lab, ex) in ((ring, (h_grown, h_lab)), (nuc, (h_lab, None))):
        got = meas.measure_dense(dev, as_tensor(lab), 1, 32, rng, exclude=None if ex is None else as_tensor(ex), glcm=True)
        want = TR.measure(imgs, lab, 1, 32, rng, ex, glcm=True)
        same(got, want, "one handle")
        d = TR.derive(*got[:4], 32)                                      # from the device's records: its clogc differs in the last bits
        assert all(np.array_equal(getattr(t, k), v, equal_nan=True) for k, v in d.items())
    assert np.array_equal(ring.label, nuc.label)
    # Channel 1 is independent uniform noise: two neighbours' levels differ by a variance of 2 (32^2 - 1) / 12 = 170 whatever the
    # object.  Channel 0 inside a blob is smooth: a blob of radius r >= 5 falls 4000 counts, 28 levels, over no less than 2 px, and
    # most of its pixels lie on the flat top, so its contrast stays far below.  That direction is certain; how a blob's contrast
    # compares with its ring's depends on where the threshold cuts the slope, and is not asserted.
    c = TX.FEATURE_NAMES.index("contrast")
    assert (nuc.mean[:, 1, c] > 100.0).all() and (nuc.mean[:, 1, c] > 2.0 * nuc.mean[:, 0, c]).all()
    t = meas.last_timing()
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values())
    seg.close()
