"""The flat-field correction on the device (cs_illum_tile_stats, cs_illum_reduce and cs_illum_apply through
cellscreen.illumination) against the CPU restatement of tests/illumination_reference.py, which tests/test_illumination_cpu.py
holds to a slow form in exact rationals.

Everything is integers, so every comparison is np.array_equal: no tolerances.

il_stats keeps a tile of at most 4096 pixels in registers and reads a larger one again in every pass; a regular tile has T x T
pixels, the last one of an axis up to 2T - 1: the shapes put sides one short of, on and one past every multiple of T = 16 up to
three tiles, single tiles on both sides of 4096 pixels, and at T = 256 the widest last tile (767 = 256 + 511).  Its radix
selection takes the high byte first: the values straddle a byte border.  il_across loops over any n; il_apply's quotient is
settled in integers: ties, negative numerators, both clamps and the function at its floor are all here.

The mean across the plate cannot sum above 2^32 inside the caps (16384 meshes of values up to 65535 stay below 2^30): the stack
at both caps stands for that case."""
import functools

import numpy as np
import pytest

import illumination_reference as IR
import intensity_reference as IRI
import segment_reference as R
import smooth_reference as SR
from cellscreen import illumination as IL
from cellscreen import intensity as IN
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

QUANTILES = [(0, 1), (1, 4), (1, 2), (1, 1), (65535, 65536)]
SIDES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49]


@pytest.fixture(scope="module")
def ic():
    c = IL.IlluminationCorrector(0)
    yield c
    c.close()


def as_tensor(a):
    import torch
    a = np.array(a)                                                      # the cached inputs are read-only
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(torch.device("cuda", 0))


def to_host(ic, t, dtype):
    ic.last_timing()                                                     # waits for what was left on the device
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


@functools.lru_cache(maxsize=None)
def noise(shape, dtype, seed):
    top = int(np.iinfo(dtype).max)
    a = np.random.default_rng(seed).integers(0, top + 1, shape).astype(dtype)
    a.flags.writeable = False
    return a


def function_of(F8, shape, T, dtype, G8, offset=0, floor=1):
    F8 = np.ascontiguousarray(F8, np.int32)
    Cn = F8.shape[0]
    return IL.IlluminationFunction(tile=T, shape=shape, channels=Cn, dtype=dtype, F8=F8, G8=list(G8),
                                   offset=[offset] * Cn if np.isscalar(offset) else list(offset), floor=floor)


def want_apply(images, fn, pedestal=None):
    return IR.apply(images, fn.F8, fn.G8, fn.tile, fn.offset, pedestal, fn.floor)


# ---- tile statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_tile_stats_at_t16_on_sides_around_its_multiples(ic, dtype):
    for k, h in enumerate(SIDES):
        w = SIDES[(k + 3) % len(SIDES)]                                  # non-square pairs
        nc = (1, 3, 4)[k % 3]
        image = noise((3, h, w, nc) if nc > 1 else (3, h, w), dtype, 100 + k)
        for q in (QUANTILES if k % 4 == 1 else [QUANTILES[k % 5], (1, 2)]):
            got = ic.tile_stats_batch(image, 16, q)
            want = IR.tile_stats(image, 16, q)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (h, w, nc, q)
    image = noise((3, 33, 49, 3), dtype, 7)
    assert np.array_equal(ic.tile_stats_batch(as_tensor(image), 16, (1, 4)), IR.tile_stats(image, 16, (1, 4)))    # a tensor


@pytest.mark.parametrize("shape", [(511, 300), (512, 512), (767, 256), (256, 767)], ids=str)
def test_tile_stats_at_t256(ic, shape):
    for dtype, nc in ((np.uint16, 1), (np.uint8, 3)):
        image = noise((2,) + shape + ((nc,) if nc > 1 else ()), dtype, 3 * shape[0] + nc)
        for q in ((1, 2), (65535, 65536)):
            assert np.array_equal(ic.tile_stats_batch(image, 256, q), IR.tile_stats(image, 256, q)), (dtype, q)


def test_single_tiles_on_both_sides_of_the_register_limit(ic):
    for shape in ((64, 64), (65, 63), (64, 65), (127, 33)):              # 4096, 4095, 4160, 4191 pixels in one tile of T = 64
        image = noise((3,) + shape + (3,), np.uint16, shape[0] * shape[1])
        assert max(1, shape[0] // 64) * max(1, shape[1] // 64) == 1
        for q in QUANTILES:
            assert np.array_equal(ic.tile_stats_batch(image, 64, q), IR.tile_stats(image, 64, q)), (shape, q)


def test_values_at_a_byte_border_two_valued_and_saturated_tiles(ic):
    rng = np.random.default_rng(21)
    shape = (3, 49, 130)                                                 # T = 16: 3 x 8 tiles, the last ones 17 and 18 wide; T = 64: one, above 4096
    sets = [np.array(s) for s in ([255, 256, 257], [0xFEFF, 0xFF00, 0xFFFF], [0, 65535], [256, 511], [1000, 1001])]
    for k, values in enumerate(sets):
        image = values[rng.integers(0, len(values), shape)].astype(np.uint16)
        image[1] = values[(rng.random(shape[1:]) < 0.3).astype(int) * (len(values) - 1)]      # another mix in the second image
        for T in (16, 64):
            for q in QUANTILES:
                assert np.array_equal(ic.tile_stats_batch(image, T, q), IR.tile_stats(image, T, q)), (k, T, q)
    for dtype in (np.uint8, np.uint16):                                  # more than half of every tile at the top
        top = int(np.iinfo(dtype).max)
        image = noise(shape, dtype, 22).copy()
        image[rng.random(shape) < 0.75] = top
        for q in QUANTILES:
            got = ic.tile_stats_batch(image, 16, q)
            assert np.array_equal(got, IR.tile_stats(image, 16, q)), (dtype, q)
        assert (ic.tile_stats_batch(image, 16, (1, 2)) == top).all()


# ---- across the plate ---------------------------------------------------------------------------------------------------------
def test_reduce_over_every_n_where_the_loop_turns(ic):
    rng = np.random.default_rng(31)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000):
        stack = rng.integers(0, 65536, (n, 2, 3, 2)).astype(np.int32)
        for rule, rp in (((1, 2), IL.reduce_params(2)), ((0, 1), IL.reduce_params(2, (0, 1))), ((1, 1), IL.reduce_params(2, (1, 1))),
                         ((1, 3), IL.reduce_params(2, (1, 3), [5, 60000], 7)), ("mean", IL.reduce_params(2, "mean", 100, 2))):
            off, fl = [int(rp.offset[0]), int(rp.offset[1])], int(rp.floor)
            got = ic.reduce_stack(stack, rp)
            assert got.dtype == np.int32 and np.array_equal(got, IR.reduce(stack, rule, off, fl)), (n, rule)
        assert np.array_equal(ic.reduce_stack(as_tensor(stack), IL.reduce_params(2)), IR.reduce(stack))            # a device stack
    stack = rng.integers(0, 65536, (40, 3, 16, 16)).astype(np.int32)
    assert np.array_equal(ic.reduce_stack(stack, IL.reduce_params(3)), IR.reduce(stack))
    assert np.array_equal(ic.reduce_stack(stack, IL.reduce_params(3, "mean")), IR.reduce(stack, "mean"))
    same = np.full((64, 1, 3, 2), 4321, np.int32)                        # all equal, an even n
    for rule in ((1, 2), (0, 1), (1, 1), "mean"):
        assert (ic.reduce_stack(same, IL.reduce_params(1, rule)) == 256 * 4321).all()
    big = np.full((16384, 1, 3, 2), 65535, np.int32)                     # both caps: the largest sum the mean can meet
    big[::2, 0, 0, 0] = 65534
    assert np.array_equal(ic.reduce_stack(big, IL.reduce_params(1, "mean")), IR.reduce(big, "mean"))
    assert np.array_equal(ic.reduce_stack(big, IL.reduce_params(1)), IR.reduce(big))


def test_reduce_offset_floor_and_the_mesh_filters(ic):
    rng = np.random.default_rng(32)
    stack = rng.integers(200, 3000, (5, 2, 3, 7)).astype(np.int32)
    got = ic.reduce_stack(stack, IL.reduce_params(2, (1, 2), [5000, 0], 9))       # an offset above every value: the floor holds
    assert (got[0] == 256 * 9).all() and np.array_equal(got, IR.reduce(stack, (1, 2), [5000, 0], 9))
    for shape in ((5, 2, 3, 7), (3, 1, 1, 1), (4, 1, 1, 9), (3, 4, 16, 16)):
        stack = rng.integers(0, 65536, shape).astype(np.int32)
        for median, sigma in ((True, 0), (False, 1.0), (True, 1.0), (False, 2.5), (True, 16.0)):     # radii 4, 10 and 64: above the mesh's sides
            w = SR.smooth_weights(sigma) if sigma else None
            got = ic.reduce_stack(stack, IL.reduce_params(shape[1], (1, 2), 3, 2, median, sigma))
            assert np.array_equal(got, IR.reduce(stack, (1, 2), 3, 2, median, w)), (shape, median, sigma)


# ---- apply --------------------------------------------------------------------------------------------------------------------
def test_apply_rounds_an_exact_tie_up_and_floors_below_the_offset(ic):
    f, g = 10, 3
    fn = function_of(np.full((1, 2, 3), 256 * f), (40, 49), 16, np.uint16, [256 * g], offset=0)
    v = np.arange(40 * 49, dtype=np.uint16).reshape(1, 40, 49)           # v g = f / 2 (mod f) wherever 3 v = 5 (mod 10): v = 5, 15, ...
    got = ic.apply_batch(v, fn)
    assert np.array_equal(got, want_apply(v, fn)[0])
    ties = (v.astype(np.int64) * g) % f == f // 2
    assert ties.sum() > 100 and np.array_equal(got[ties].astype(np.int64), (v[ties].astype(np.int64) * g + f // 2) // f)
    assert (got[ties].astype(np.int64) * f > v[ties].astype(np.int64) * g).all()          # up, not down or to even
    fn = function_of(np.full((1, 2, 3), 256 * f), (40, 49), 16, np.uint16, [256 * g], offset=1000)
    for ped in (0, 700):                                                 # v < offset: the quotient is negative and floors
        got, clipped = ic.apply_batch(v, fn, pedestal=ped, return_clipped=True)
        want, want_clipped = want_apply(v, fn, ped)
        assert np.array_equal(got, want) and np.array_equal(clipped, want_clipped)
        assert (clipped[0, 0, 0] > 0) == (ped == 0) and (ped == 0 or (got[0, 0, :20] > 0).all())
    assert got[0].ravel()[995] == 700 + (-5 * g * 2 + f) // (2 * f) == 699        # -1.5 + 0.5 floors to -1


def test_apply_clips_at_both_ends_of_the_scales(ic):
    for dtype in (np.uint8, np.uint16):
        top = int(np.iinfo(dtype).max)
        v = noise((2, 33, 47, 2), dtype, 41)
        for F, G in ((256, (1 << 24) - 1), ((1 << 24) - 1, 1), (256, 256), (256 * 300, 256 * 299)):
            fn = function_of(np.full((2, 2, 2), F), (33, 47), 16, dtype, [G, G], offset=[0, 3])
            got, clipped = ic.apply_batch(v, fn, return_clipped=True)
            want, want_clipped = want_apply(v, fn)
            assert np.array_equal(got, want) and np.array_equal(clipped, want_clipped), (dtype, F, G)
        assert clipped[:, 0, 1].sum() == 0 and got.max() <= top
    fn = function_of(np.full((2, 2, 2), 256), (33, 47), 16, np.uint16, [(1 << 24) - 1] * 2)
    got, clipped = ic.apply_batch(v, fn, return_clipped=True)
    assert (got[v > 0] == 65535).all() and clipped[:, :, 1].sum() == (v > 0).sum()


def test_apply_where_the_extrapolation_goes_negative(ic):
    F8 = np.array([[[256 * 4000, 256 * 10, 256 * 10], [256 * 10, 256 * 4000, 256 * 10]]])
    fn = function_of(F8, (33, 49), 16, np.uint16, [256 * 50], offset=2, floor=3)
    N, D = IR.maps(fn.F8[0], 33, 49, 16, 3)
    assert (N == 256 * 3 * D).any()                                      # pinned at the floor somewhere
    v = noise((2, 33, 49), np.uint16, 42)
    got, clipped = ic.apply_batch(v, fn, return_clipped=True)
    want, want_clipped = want_apply(v, fn)
    assert np.array_equal(got, want) and np.array_equal(clipped, want_clipped)


@pytest.mark.parametrize("shape", [(256, 767), (767, 256), (300, 40)], ids=str)
def test_apply_on_the_widest_last_tile_and_a_single_node_axis(ic, shape):
    T = 256 if max(shape) == 767 else 32
    rng = np.random.default_rng(43)
    my, mx = max(1, shape[0] // T), max(1, shape[1] // T)
    assert min(my, mx) == 1
    F8 = (256 * rng.integers(100, 60000, (3, my, mx))).astype(np.int32)
    fn = function_of(F8, shape, T, np.uint16, IR.scale(F8), offset=[0, 50, 100])
    v = noise((1,) + shape + (3,), np.uint16, 44)
    got, clipped = ic.apply_batch(v, fn, return_clipped=True)
    want, want_clipped = want_apply(v, fn)
    assert np.array_equal(got, want) and np.array_equal(clipped, want_clipped)
    band = T // 2
    assert np.array_equal(got[:, :, :band], want[:, :, :band]) and np.array_equal(got[:, :, -band:], want[:, :, -band:])


def test_apply_in_place_on_tensors_twice_and_image_by_image(ic):
    import torch
    rng = np.random.default_rng(45)
    for dtype, nc in ((np.uint16, 1), (np.uint8, 3), (np.uint16, 4)):
        shape = (3, 70, 131) + ((nc,) if nc > 1 else ())
        v = noise(shape, dtype, 46 + nc)
        F8 = (256 * rng.integers(20, 3000, (nc, 2, 4))).astype(np.int32)
        fn = function_of(F8, (70, 131), 32, dtype, IR.scale(F8, "min"), offset=list(range(nc)))
        want, want_clipped = want_apply(v, fn)
        got = ic.apply_batch(v, fn)
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, want)
        place = v.copy()
        assert ic.apply_batch(place, fn, out=place) is place and np.array_equal(place, want)         # in place, numpy
        dev = as_tensor(v)
        out = ic.apply_batch(dev, fn)                                    # no counts: no host synchronisation
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dev.dtype and out.shape == dev.shape
        assert np.array_equal(to_host(ic, out, dtype), want) and np.array_equal(to_host(ic, dev, dtype), v)
        again, clipped = ic.apply_batch(dev, fn, out=dev, return_clipped=True)                       # in place, tensor, with counts
        assert again is dev and np.array_equal(to_host(ic, dev, dtype), want) and np.array_equal(clipped, want_clipped)
        assert to_host(ic, out, dtype).tobytes() == to_host(ic, dev, dtype).tobytes()               # two runs, equal bytes
        for b in range(3):                                               # the images of a batch do not influence each other
            alone, c1 = ic.apply_batch(np.ascontiguousarray(v[b:b + 1]), fn, return_clipped=True)
            assert np.array_equal(alone[0], want[b]) and np.array_equal(c1[0], want_clipped[b])
    t = ic.last_timing()
    assert t["apply_ms"] > 0.0 and set(t) == {"stats_ms", "reduce_ms", "apply_ms"}


# ---- the status words -----------------------------------------------------------------------------------------------------------
def test_a_bad_device_stack_or_function_is_refused_by_its_status_word(ic):
    """A value out of range in device memory is cut to the range and raises a status word: the call answers if it synchronises,
    else cs_illum_last_timing does, once; the handle stays usable."""
    from cellscreen import _lib as L
    stack = np.full((3, 1, 2, 2), 500, np.int32)
    bad = stack.copy()
    bad[1, 0, 1, 0], bad[2, 0, 0, 1] = 70000, -5
    with pytest.raises(L.CellScreenError) as ei:
        ic.reduce_stack(as_tensor(bad), IL.reduce_params(1))
    assert ei.value.status == -1 and "device stack" in str(ei.value)
    assert np.array_equal(ic.reduce_stack(as_tensor(stack), IL.reduce_params(1)), IR.reduce(stack))       # read and cleared
    fn = function_of(np.full((1, 2, 2), 256 * 100), (40, 40), 16, np.uint16, [256 * 90])
    v = noise((2, 40, 40), np.uint16, 61)
    dev = as_tensor(v)
    assert np.array_equal(to_host(ic, ic.apply_batch(dev, fn), np.uint16), want_apply(v, fn)[0])
    for value, cut in ((255, 256), (1 << 24, (1 << 24) - 1), (-7, 256)):
        fn._dev[0, 1, 1] = value                                         # the device copy alone: the host never sees it
        F8 = fn.F8.copy()
        F8[0, 1, 1] = cut
        want = IR.apply(v, F8, fn.G8, 16, fn.offset, None, fn.floor)[0]
        with pytest.raises(L.CellScreenError) as ei:
            ic.apply_batch(dev, fn, return_clipped=True)                 # synchronises: this call answers
        assert ei.value.status == -1 and "device function" in str(ei.value)
        ic.last_timing()                                                 # nothing is left to report
        out = ic.apply_batch(dev, fn)                                    # does not synchronise: it returns, the values cut
        with pytest.raises(L.CellScreenError) as ei:
            ic.last_timing()
        assert ei.value.status == -1 and "device function" in str(ei.value)
        assert np.array_equal(to_host(ic, out, np.uint16), want)        # reported once: to_host reads the times again
    fn.F8[0, 1, 1] = 256 * 50                                            # a changed F8 is uploaded again
    assert np.array_equal(to_host(ic, ic.apply_batch(dev, fn), np.uint16), want_apply(v, fn)[0])
    assert np.array_equal(ic.apply_batch(v, fn), want_apply(v, fn)[0])


# ---- the chain ----------------------------------------------------------------------------------------------------------------
def test_add_finish_apply_segment_and_measure_on_one_handle():
    import torch
    fields, _ = IR.plate(3, 8, 256, 8, 0.5)
    dev = as_tensor(fields)
    seg = S.ThresholdSegmenter(0, "otsu", 1, True)
    before = [np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a) for a in seg.segment_batch(dev[:4])]
    ic = IL.IlluminationCorrector(0, extractor=seg)
    assert ic.add_batch(dev[:4], tile=32) == 4 and ic.add_batch(fields[4:], tile=32) == 8 and ic.n_images == 8
    with pytest.raises(ValueError):
        ic.add_batch(np.ascontiguousarray(fields[:, :128]), tile=32)     # another shape
    with pytest.raises(ValueError):
        ic.add_batch(fields, tile=64)                                    # another tile
    fn = ic.finish(offset=100)
    stack = IR.tile_stats(fields, 32)
    assert np.array_equal(to_host(ic, ic._stack[:8], np.int32), stack)
    F8 = IR.reduce(stack, (1, 2), 100, 1)
    G8 = IR.scale(F8)
    assert np.array_equal(fn.F8, F8) and fn.G8 == G8 and fn.n_images == 8 and fn.offset == [100] and fn.tile == 32
    flat = ic.apply_batch(dev, fn)
    want_flat, _ = IR.apply(fields, F8, G8, 32, 100)
    labels, n, thr = seg.segment_batch(flat)
    elab, en, ethr = R.segment_batch(want_flat, threshold="otsu", connectivity=1, fill_holes=True)
    assert np.array_equal(to_host(ic, flat, np.uint16), want_flat)
    assert np.array_equal(labels.cpu().numpy(), elab) and np.array_equal(n, en) and np.array_equal(thr, ethr)
    meas = IN.IntensityMeasurer(0, extractor=seg)
    geom, stats = meas.measure_dense(flat, labels)
    wgeom, wstats = IRI.measure(want_flat, elab, None, int(elab.max()))
    assert np.array_equal(geom, wgeom) and np.array_equal(stats, wstats)
    assert ic._pre is None and meas._pre is None                         # the segmenter's handle did the work
    after = [np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a) for a in seg.segment_batch(dev[:4])]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    ic.reset()
    assert ic.n_images == 0 and ic.add_batch(fields[:2], tile=64) == 2   # after reset() another tile is taken
    seg.close()
