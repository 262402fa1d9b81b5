"""The geodesic label growth on the device (cs_label_propagate through cellscreen.propagate) against the CPU restatement of
tests/propagate_reference.py, which tests/test_propagate_cpu.py holds to scipy.sparse.csgraph.dijkstra.

Labels and costs are integers, so every comparison is np.array_equal: no tolerances.

The relaxation works on 64 x 16 tiles with a one-pixel halo; SHAPES crosses the tile one short, equal and one past in both
directions, has several tiles either way, and the single row, column and pixel.  The restatement runs once per content, metric
and guide without a limit; with max_cost the expected planes are its cut (costs only grow along a path: propagate_reference.cut,
which the CPU tests hold to the rule with the limit inside)."""
import functools

import numpy as np
import pytest

import intensity_reference as IR
import pipeline_reference as PL
import propagate_reference as PR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import intensity as IN
from cellscreen import propagate as PG
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300), (300, 1), (15, 63), (16, 64), (17, 65), (33, 129), (70, 300), (1, 1)]
LAM = {"cityblock": 3, "chessboard": 1, "chamfer": 2}


@pytest.fixture(scope="module")
def tool():
    t = PG.LabelPropagator(0)
    yield t
    t.close()


def as_tensor(a):
    import torch
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))     # a copy: the cached contents are read-only


def to_np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


@functools.lru_cache(maxsize=None)
def contents(shape, seed, channels=1, dtype=np.uint16):
    """(seeds int32 [2,H,W], mask uint8 [2,H,W], guide [2,H,W,channels]): two fields of propagate_reference.field."""
    f = [PR.field(shape, seed + k, cells=max(2, shape[0] * shape[1] // 900), channels=channels, dtype=dtype) for k in range(2)]
    out = tuple(np.stack([x[i] for x in f]) for i in range(3))
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def unlimited(shape, seed, metric, with_guide, channels=1, dtype=np.uint16):
    seeds, mask, guide = contents(shape, seed, channels, dtype)
    return PR.propagate(seeds, mask, guide if with_guide else None, channels - 1, metric, LAM[metric])


def check(got, want):
    (g, c), (wg, wc) = got, want
    g, c = to_np(g), to_np(c)
    assert g.dtype == np.int32 and c.dtype == np.int64 and g.shape == wg.shape and c.shape == wc.shape
    assert np.array_equal(c, wc), int((c != wc).sum())
    assert np.array_equal(g, wg), int((g != wg).sum())


@pytest.mark.parametrize("shape", SHAPES)
def test_labels_and_costs_equal_the_restatement(tool, shape):
    seed = 7 * shape[0] + shape[1]
    seeds, mask, guide = contents(shape, seed)
    for metric in PR.METRICS:
        for with_guide in (False, True):
            free = unlimited(shape, seed, metric, with_guide)
            kw = dict(mask=mask, guide=guide if with_guide else None, metric=metric, lam=LAM[metric])
            check(tool.propagate_batch(seeds, return_cost=True, **kw), free)
            reached = free[1][free[1] > 0]
            limit = int(np.median(reached)) if reached.size else 3              # half of what grows lies beyond it
            check(tool.propagate_batch(seeds, return_cost=True, max_cost=limit, **kw), PR.cut(*free, limit))
    only = tool.propagate_batch(seeds, mask=mask)                           # without the cost plane, the defaults
    assert isinstance(only, np.ndarray) and np.array_equal(only, PR.propagate(seeds, mask)[0])


def test_no_mask_grows_everywhere_and_distance_is_a_cost(tool):
    seeds = contents((33, 129), 5)[0]
    for metric in PR.METRICS:
        free = PR.propagate(seeds, metric=metric, lam=LAM[metric])
        check(tool.propagate_batch(seeds, metric=metric, lam=LAM[metric], return_cost=True), free)
        assert (free[0] > 0).all()
        limit = PR.max_cost_of(6.5, metric, LAM[metric])
        check(tool.propagate_batch(seeds, metric=metric, lam=LAM[metric], distance=6.5, return_cost=True), PR.cut(*free, limit))


def test_serpentine_corridor_takes_more_than_one_group_of_rounds(tool):
    seeds, mask = PR.serpentine(48, 192)
    for metric in ("cityblock", "chamfer"):
        want = PR.propagate_one(seeds, mask, None, metric, 1)
        got = tool.propagate_batch(seeds[None], mask=mask[None], metric=metric, return_cost=True)
        rounds = tool.last_timing()["propagate_rounds"]
        check(got, (want[0][None], want[1][None]))
        assert (got[0][0] == mask).all() and rounds > 8, rounds            # the front re-enters every tile: beyond the first group
        print(f"\nserpentine {metric}: {rounds} rounds")
    stop = int(want[1].max()) // 2                                      # and stopped half way down the corridor
    check(tool.propagate_batch(seeds[None], mask=mask[None], metric="chamfer", max_cost=stop, return_cost=True),
          tuple(a[None] for a in PR.cut(*want, stop)))


@pytest.mark.parametrize("dtype,channels", [(np.uint8, 1), (np.uint8, 3), (np.uint16, 3), (np.uint16, 4), (np.uint8, 4)])
def test_guide_dtypes_and_channels(tool, dtype, channels):
    shape, seed = (33, 129), 21
    seeds, mask, guide = contents(shape, seed, channels, dtype)
    want = unlimited(shape, seed, "chamfer", True, channels, dtype)
    kw = dict(mask=mask, guide_channel=channels - 1, metric="chamfer", lam=LAM["chamfer"], return_cost=True)
    check(tool.propagate_batch(seeds, guide=guide, **kw), want)
    check(tool.propagate_batch(as_tensor(seeds), guide=as_tensor(guide), **dict(kw, mask=as_tensor(mask))), want)
    if channels == 1:
        kw["guide_channel"] = 0
        check(tool.propagate_batch(seeds, guide=np.ascontiguousarray(guide[..., 0]), **kw), want)       # [B,H,W]
    else:
        other = PR.propagate(seeds, mask, guide, 0, "chamfer", LAM["chamfer"])
        assert not np.array_equal(other[1], want[1])                    # the channels differ, so the choice shows
        check(tool.propagate_batch(seeds, guide=guide, **dict(kw, guide_channel=0)), other)


def test_max_cost_stops_growth_inside_a_tile(tool):
    seeds = np.zeros((1, 16, 64), np.int32)
    seeds[0, 8, 5] = 3
    for metric, limit in (("cityblock", 20), ("chessboard", 7), ("chamfer", 52)):
        got, cost = tool.propagate_batch(seeds, metric=metric, max_cost=limit, return_cost=True)
        check((got, cost), PR.propagate(seeds, metric=metric, max_cost=limit))
        assert cost.max() <= limit and (got == 0).any() and (got == 3).sum() > 50 and got[0, 8, 63] == 0


def test_seeds_off_the_mask_empty_masks_and_planes_without_seeds(tool):
    shape, seed = (33, 129), 9
    seeds, mask, _ = contents(shape, seed)
    hole = mask.copy()
    hole[seeds == seeds.max()] = 0                                      # a nucleus whose own pixels the mask leaves out
    far = seeds.copy()
    ys, xs = np.nonzero((mask[0] == 0) & (seeds[0] == 0))
    far[0, ys[len(ys) // 2], xs[len(ys) // 2]] = 77                     # and a seed on closed ground
    got = tool.propagate_batch(far, mask=hole, return_cost=True)
    check(got, PR.propagate(far, hole))
    assert np.array_equal(got[0][far > 0], far[far > 0]) and (got[0] == 77).sum() >= 1
    nothing = np.zeros_like(mask)
    got = tool.propagate_batch(seeds, mask=nothing, return_cost=True)
    assert np.array_equal(got[0], seeds) and np.array_equal(got[1], np.where(seeds > 0, 0, -1))
    got = tool.propagate_batch(np.zeros_like(seeds), mask=mask, return_cost=True)
    assert not got[0].any() and (got[1] == -1).all()
    flags = np.ascontiguousarray(mask.astype(bool))                     # a bool mask is a byte mask
    assert np.array_equal(tool.propagate_batch(seeds, mask=flags), PR.propagate(seeds, mask)[0])
    big = (mask * 200).astype(np.uint8)                                 # any non-zero byte opens
    assert np.array_equal(tool.propagate_batch(seeds, mask=big), PR.propagate(seeds, mask)[0])


def test_largest_label_and_ties_to_the_smallest(tool):
    two = np.zeros((1, 9, 9), np.int32)
    two[0, 4, 1], two[0, 4, 7] = PR.MAX_LABEL, 5
    for metric in PR.METRICS:
        got = tool.propagate_batch(two, metric=metric, return_cost=True)
        check(got, PR.propagate(two, metric=metric))
        assert (got[0][0, :, 4] == 5).all() and got[0][0, 4, 3] == PR.MAX_LABEL


def test_in_place_input_kinds_and_repeatability(tool):
    import torch
    shape, seed = (70, 300), 11
    seeds, mask, guide = contents(shape, seed)
    want = unlimited(shape, seed, "chamfer", True)
    kw = dict(guide_channel=0, metric="chamfer", lam=LAM["chamfer"], return_cost=True)
    a = tool.propagate_batch(seeds, mask=mask, guide=guide, **kw)
    b = tool.propagate_batch(seeds, mask=mask, guide=guide, **kw)
    check(a, want)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])    # bit-identical run to run
    t = tool.last_timing()
    assert set(t) == {"propagate_init_ms", "propagate_relax_ms", "propagate_finish_ms", "propagate_rounds"}
    assert all(np.isfinite(v) and v > 0 for v in t.values()) and isinstance(t["propagate_rounds"], int)
    host = seeds.copy()
    r, c = tool.propagate_batch(host, mask=mask, guide=guide, out=host, **kw)          # numpy, in place
    assert r is host
    check((host, c), want)
    ds, dm, dg = as_tensor(seeds), as_tensor(mask), as_tensor(guide)
    r, c = tool.propagate_batch(ds, mask=dm, guide=dg, **kw)             # tensors in: tensors out, the input untouched
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.int32 and c.dtype == torch.int64 and c.is_cuda
    check((r, c), want)
    assert np.array_equal(to_np(ds), seeds)
    r2, c2 = tool.propagate_batch(ds, mask=dm, guide=dg, out=ds, **kw)   # a tensor, in place
    assert r2 is ds
    check((ds, c2), want)
    check(tool.propagate_batch(as_tensor(seeds), mask=dm.bool(), guide=dg, **kw), want)                 # a bool tensor mask
    with pytest.raises(TypeError):
        tool.propagate_batch(seeds, mask=dm)
    with pytest.raises(TypeError):
        tool.propagate_batch(seeds, out=torch.empty_like(ds))


def test_an_image_alone_equals_its_plane_in_a_batch(tool):
    shape = (70, 300)
    f = [PR.field(shape, 40 + k, cells=n) for k, n in enumerate((3, 17, 40))]
    seeds, mask, guide = (np.stack([x[i] for x in f]) for i in range(3))
    whole = tool.propagate_batch(seeds, mask=mask, guide=guide, lam=4, return_cost=True)
    check(whole, PR.propagate(seeds, mask, guide, lam=4))
    for b in range(3):
        one = tool.propagate_batch(seeds[b:b + 1].copy(), mask=mask[b:b + 1].copy(), guide=guide[b:b + 1].copy(), lam=4, return_cost=True)
        assert np.array_equal(one[0][0], whole[0][b]) and np.array_equal(one[1][0], whole[1][b])
    assert len({int((whole[0][b] > 0).sum()) for b in range(3)}) == 3


def test_a_bad_seed_is_an_error_status_and_the_tool_stays_usable(tool):
    shape, seed = (17, 65), 5
    seeds, mask, _ = contents(shape, seed)
    want = unlimited(shape, seed, "chamfer", False)
    for where, value in (((0, 0, 0), -1), ((1, 16, 64), PR.MAX_LABEL + 1), ((0, 9, 63), -(2 ** 31)), ((1, 3, 3), 2 ** 31 - 1)):
        bad = seeds.copy()
        bad[where] = value
        for arg, m in ((bad, mask), (as_tensor(bad), as_tensor(mask))):
            with pytest.raises(L.CellScreenError) as ei:
                tool.propagate_batch(arg, mask=m)
            assert ei.value.status == -1 and "seed" in str(ei.value)
            check(tool.propagate_batch(seeds, mask=mask, lam=LAM["chamfer"], return_cost=True), want)


def body_scene():
    """uint16 [2,96,128,2]: channel 0 the nuclei, five bright blobs per image; channel 1 the cell bodies, wider and dimmer."""
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.empty((2, H, W, 2), np.uint16)
    for b in range(2):
        n = 300.0 + rng.normal(0.0, 10.0, (H, W))
        c = 300.0 + rng.normal(0.0, 10.0, (H, W))
        for y, x, r in ((24, 25, 9), (30, 80, 12), (70, 40, 10), (70, 100, 7 + 4 * b), (50, 62, 5)):
            q = (yy - y) ** 2 + (xx - x) ** 2
            n += 4000.0 * np.exp(-(q / (2.0 * (r / 1.6) ** 2)) ** 2)
            c += 1500.0 * np.exp(-(q / (2.0 * (1.9 * r / 1.6) ** 2)) ** 2)
        imgs[b, ..., 0] = np.clip(np.rint(n), 0, 65535)
        imgs[b, ..., 1] = np.clip(np.rint(c), 0, 65535)
    return imgs


def test_nuclei_to_cells_to_measurements_on_one_handle():
    """segment_batch leaves the nuclei on the device, the same handle cuts the body mask, grows the nuclei inside it along the body
    stain, and measures the grown labels; everything equals the host chain of restatements."""
    imgs = body_scene()
    seg = S.ThresholdSegmenter(0)
    bodies = S.ThresholdSegmenter(0, extractor=seg, open_radius=1)
    grow = PG.LabelPropagator(0, extractor=seg)
    meas = IN.IntensityMeasurer(0, extractor=seg)
    dev = as_tensor(imgs)
    nuclei, n_labels, _ = seg.segment_batch(dev, channel=0)
    mask = bodies.clean_mask_batch(dev, channel=1)
    cells, cost = grow.propagate_batch(nuclei, mask=mask, guide=dev, guide_channel=1, lam=4, return_cost=True)
    max_label = int(n_labels.max())
    geom, stats = meas.measure_dense(dev, cells, max_label=max_label)
    assert grow._handle is seg._handle and grow._pre is None and meas._pre is None and bodies._pre is None

    want_nuclei = R.segment_batch(np.ascontiguousarray(imgs[..., 0]))[0]
    want_mask = PL.segment_batch(imgs, channel=1, open_radius=1)[-1]["clean_mask_batch"]
    assert np.array_equal(to_np(nuclei), want_nuclei) and np.array_equal(to_np(mask), want_mask) and want_mask.any()
    want = PR.propagate(want_nuclei, want_mask, imgs, 1, "chamfer", 4)
    check((cells, cost), want)
    assert (want[0] > 0).sum() > 2 * (want_nuclei > 0).sum()            # the cells are much larger than their nuclei
    wg, ws = IR.measure(imgs, want[0], max_label=max_label)[:2]
    assert np.array_equal(geom, wg) and np.array_equal(stats, ws)
    t = grow.last_timing()
    assert t["propagate_rounds"] >= 2 and all(np.isfinite(v) and v >= 0 for v in t.values())
    seg.close()
