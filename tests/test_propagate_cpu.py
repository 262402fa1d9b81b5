"""CPU tests of the geodesic label growth (cs_label_propagate, cellscreen/propagate.py): the restatement of
tests/propagate_reference.py against scipy.sparse.csgraph.dijkstra as recorded in tests/golden/golden_propagate.npz (labels and costs
equal everywhere, the ties included: the golden takes the smallest label among equal distances by itself), its two forms against
each other, one pixel from the definition, the closed forms of the three metrics, the distance's integer form, and the wrapper's
and the C ABI's refusals before any device work."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import propagate_reference as PR
from cellscreen import _lib as L
from cellscreen import propagate as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_propagate.npz")


def golden_cases():
    g = np.load(GOLDEN)
    for i in range(int(g["n_cases"])):
        yield dict(name=str(g[f"name_{i}"]), seeds=g[f"seeds_{i}"], mask=g[f"mask_{i}"], guide=g[f"guide_{i}"] if f"guide_{i}" in g else None,
                   metric=str(g[f"metric_{i}"]), lam=int(g[f"lam_{i}"]), max_cost=int(g[f"max_cost_{i}"]), cost=g[f"cost_{i}"],
                   labels=g[f"labels_{i}"])


def test_restatement_equals_scipy_everywhere():
    seen = dict(metric=set(), guide=set(), lam=set(), capped=set())
    n = outside = pockets = 0
    for c in golden_cases():
        assert c["seeds"].dtype == np.int32 and c["seeds"].size <= 70 * 300 and c["mask"].dtype == np.uint8
        got, cost = PR.propagate_one(c["seeds"], c["mask"], c["guide"], c["metric"], c["lam"], c["max_cost"] or PR.NO_LIMIT)
        assert got.dtype == np.int32 and cost.dtype == np.int64
        assert np.array_equal(got, c["labels"]) and np.array_equal(cost, c["cost"]), c["name"]
        assert np.array_equal(got[c["seeds"] > 0], c["seeds"][c["seeds"] > 0]) and not cost[c["seeds"] > 0].any()
        assert not got[(c["mask"] == 0) & (c["seeds"] == 0)].any()                      # nothing grows off the mask
        assert ((got > 0) & (c["seeds"] == 0)).sum() > 100
        seen["metric"].add(c["metric"]); seen["guide"].add(c["guide"] is not None); seen["lam"].add(c["lam"]); seen["capped"].add(c["max_cost"] > 0)
        outside += int(((c["seeds"] > 0) & (c["mask"] == 0)).sum())
        pockets += int(((c["mask"] != 0) & (got == 0)).sum() > 0 and c["max_cost"] == 0)
        n += 1
    assert n == 9 and seen == dict(metric=set(PR.METRICS), guide={False, True}, lam={1, 8}, capped={False, True})
    assert outside > 0 and pockets > 0


def test_the_cut_equals_the_rule_with_max_cost():
    for c in golden_cases():
        if c["max_cost"]:
            free = PR.propagate_one(c["seeds"], c["mask"], c["guide"], c["metric"], c["lam"])
            lab, cost = PR.cut(*free, c["max_cost"])
            assert np.array_equal(lab, c["labels"]) and np.array_equal(cost, c["cost"]) and (free[1] > c["max_cost"]).any()


def test_heap_form_and_synchronous_relaxation_reach_the_same_fixed_point():
    for c in golden_cases():
        args = (c["seeds"], c["mask"], c["guide"], c["metric"], c["lam"], c["max_cost"] or PR.NO_LIMIT)
        a, b = PR.propagate_one(*args), PR.relax_sync(*args)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and b[2] > 3, c["name"]
    seeds, mask = PR.serpentine(16, 40)
    for metric in PR.METRICS:
        a, b = PR.propagate_one(seeds, mask, None, metric, 3), PR.relax_sync(seeds, mask, None, metric, 3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert b[2] > 8 * 40 - 30 and (a[0] == mask).all()              # the whole corridor, one sweep per pixel of it
        axial = 3 * PR.WEIGHTS[metric][0]
        assert a[1][14, 39 if metric == "cityblock" else 38] > axial * 7 * 38


def brute_force_pixel(seeds, mask, guide, metric, lam, target):
    """(cost, label) of one pixel by enumerating every simple path from every seed pixel: no code shared with the restatement."""
    H, W = seeds.shape
    moves = {"cityblock": [(0, 1, 1), (1, 0, 1), (0, -1, 1), (-1, 0, 1)],
             "chessboard": [(dy, dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx],
             "chamfer": [(dy, dx, 5 if dy == 0 or dx == 0 else 7) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]}[metric]
    best = [None]

    def walk(y, x, cost, label, seen):
        if (y, x) == target:
            if best[0] is None or (cost, label) < best[0]:
                best[0] = (cost, label)
            return
        for dy, dx, w in moves:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and (yy, xx) not in seen and seeds[yy, xx] == 0 and mask[yy, xx]:
                walk(yy, xx, cost + lam * w + abs(int(guide[yy, xx]) - int(guide[y, x])), label, seen | {(yy, xx)})

    for y, x in zip(*np.nonzero(seeds)):
        walk(int(y), int(x), 0, int(seeds[y, x]), {(int(y), int(x))})
    return best[0]


def test_one_pixel_from_the_definition():
    seeds = np.array([[2, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], np.int32)
    mask = np.array([[0, 1, 1, 0], [1, 1, 0, 1], [1, 1, 1, 1], [1, 0, 1, 1]], np.uint8)
    guide = np.array([[9, 1, 7, 0], [3, 12, 0, 2], [4, 3, 9, 5], [0, 0, 6, 1]], np.int64)
    flat = np.zeros_like(guide)
    for metric, lam, g in itertools.product(PR.METRICS, (1, 2), (guide, flat)):
        lab, cost = PR.propagate_one(seeds, mask, g, metric, lam)
        for target in ((1, 1), (2, 0), (3, 2), (0, 2)):
            want = brute_force_pixel(seeds, mask, g, metric, lam, target)
            got = (int(cost[target]), int(lab[target])) if lab[target] else None
            assert got == want, (metric, lam, target)
    assert brute_force_pixel(seeds, mask, flat, "cityblock", 1, (0, 3)) is None          # closed: nothing arrives


def test_closed_forms_of_the_three_metrics_and_the_tie():
    seeds = np.zeros((21, 31), np.int32)
    seeds[9, 12] = 7
    yy, xx = np.mgrid[0:21, 0:31]
    dy, dx = np.abs(yy - 9), np.abs(xx - 12)
    for metric, want in (("cityblock", dy + dx), ("chessboard", np.maximum(dy, dx)),
                         ("chamfer", 5 * np.maximum(dy, dx) + 2 * np.minimum(dy, dx))):
        for lam in (1, 4):
            lab, cost = PR.propagate_one(seeds, None, None, metric, lam)
            assert np.array_equal(cost, lam * want) and (lab == 7).all()
    two = np.zeros((9, 9), np.int32)
    two[4, 1], two[4, 7] = 2, 1                                                         # the column x = 4 is equally far from both
    for metric in PR.METRICS:
        lab, cost = PR.propagate_one(two, None, None, metric, 1)
        assert (lab[:, 4] == 1).all() and (lab[4, :4] == 2).all() and (lab[4, 5:] == 1).all()
    two[4, 1], two[4, 7] = 1, 2
    assert (PR.propagate_one(two, None, None, "chamfer", 1)[0][:, 4] == 1).all()


def test_restatement_edge_cases():
    z = np.zeros((5, 7), np.int32)
    lab, cost = PR.propagate_one(z)
    assert not lab.any() and (cost == -1).all()
    s = z.copy()
    s[2, 3] = 4
    lab, cost = PR.propagate_one(s, np.zeros((5, 7), np.uint8))                         # an all-zero mask: the seeds as they are
    assert np.array_equal(lab, s) and cost[2, 3] == 0 and (cost < 0).sum() == 34
    lab, cost = PR.propagate(np.stack([s, z, s[::-1]]), max_cost=10)                    # a batch: image by image
    assert np.array_equal(lab[0], PR.propagate_one(s, max_cost=10)[0]) and not lab[1].any() and np.array_equal(lab[2], lab[0][::-1])
    assert (cost[0] <= 10).all() and (cost[0] == -1).any()
    for bad in (-1, PR.MAX_LABEL + 1):
        b = s.copy()
        b[0, 0] = bad
        with pytest.raises(ValueError):
            PR.propagate_one(b)
    s[0, 0] = PR.MAX_LABEL
    assert PR.propagate_one(s, max_cost=5)[0][0, 1] == PR.MAX_LABEL


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_distance_and_params_arithmetic_and_refusals():
    import cellscreen
    assert cellscreen.LabelPropagator is PG.LabelPropagator and cellscreen.propagate_params is PG.propagate_params
    assert PG.NO_LIMIT == PR.NO_LIMIT == (1 << 40) - 2 and PG.MAX_LABEL == PR.MAX_LABEL == 1 << 20
    for d, metric, lam, n in ((16, "chamfer", 1, 80), (16, "cityblock", 1, 16), (16, "chessboard", 3, 48), (2.5, "chamfer", 1, 12),
                              (2.5, "chamfer", 3, 37), (0.3, "chamfer", 1, 1), (np.float32(1.5), "cityblock", 255, 382), (np.int64(7), "chamfer", 8, 280),
                              (1.9999, "cityblock", 1, 1), (1e9, "chamfer", 1, 5 * 10 ** 9)):
        assert PG.max_cost_of(d, metric, lam) == n == PR.max_cost_of(d, metric, lam), (d, metric, lam)
    for d, exc in ((True, TypeError), ("5", TypeError), (None, TypeError), (float("nan"), ValueError), (float("inf"), ValueError), (0, ValueError),
                   (0.1, ValueError), (-3, ValueError), (1 << 40, ValueError)):
        with pytest.raises(exc):
            PG.max_cost_of(d, "chamfer", 1)
    p = PG.propagate_params("chessboard", 9, 2, 123456789012)
    assert (p.metric, p.lam, p.guide_channel, p.reserved, p.max_cost) == (1, 9, 2, 0, 123456789012)
    assert PG.propagate_params().max_cost == PG.NO_LIMIT and PG.propagate_params().metric == 2 and C.sizeof(L.CSPropagateParams) == 24
    for kw, exc in ((dict(metric="euclidean"), ValueError), (dict(metric=2), ValueError), (dict(lam=0), ValueError), (dict(lam=256), ValueError),
                    (dict(lam=1.0), TypeError), (dict(lam=True), TypeError), (dict(max_cost=0), ValueError), (dict(max_cost=PG.NO_LIMIT + 1), ValueError),
                    (dict(max_cost=4.0), TypeError), (dict(guide_channel=-1), ValueError), (dict(guide_channel=4), ValueError),
                    (dict(guide_channel=0.0), TypeError)):
        with pytest.raises(exc):
            PG.propagate_params(**kw)


def test_propagator_refusals_before_a_handle_exists():
    import torch
    t = PG.LabelPropagator(0)
    a = np.zeros((2, 8, 12), np.int32)
    m = np.ones((2, 8, 12), np.uint8)
    g = np.zeros((2, 8, 12, 3), np.uint16)
    ro = a.copy()
    ro.flags.writeable = False
    cases = [
        (a.astype(np.int64), {}, TypeError), (a[:, :, ::2], {}, ValueError), (a[0], {}, ValueError), (a[:0], {}, ValueError), (list(a), {}, TypeError),
        (torch.zeros((2, 8, 12), dtype=torch.int32), {}, ValueError),                            # a CPU tensor
        (np.zeros((1, 2, 4097), np.int32), {}, ValueError), (np.zeros((1, 4097, 2), np.int32), {}, ValueError),
        (a, dict(mask=m.astype(np.int32)), TypeError), (a, dict(mask=m[:1]), ValueError), (a, dict(mask=m[:, :, ::-1]), ValueError),
        (a, dict(mask=torch.ones((2, 8, 12), dtype=torch.uint8)), TypeError),                    # numpy seeds, a tensor mask
        (a, dict(mask=list(m)), TypeError), (a, dict(mask=m[0]), ValueError),
        (a, dict(guide=g.astype(np.float32)), TypeError), (a, dict(guide=g.astype(np.int16)), TypeError), (a, dict(guide=g[:, :4]), ValueError),
        (a, dict(guide=g[..., ::2]), ValueError), (a, dict(guide=np.zeros((2, 8, 12, 5), np.uint8)), ValueError),
        (a, dict(guide=g, guide_channel=3), ValueError), (a, dict(guide=g[..., 0].copy(), guide_channel=1), ValueError),
        (a, dict(guide_channel=1), ValueError), (a, dict(guide=torch.zeros((2, 8, 12), dtype=torch.uint8)), TypeError),
        (a, dict(lam=0), ValueError), (a, dict(lam=256), ValueError), (a, dict(lam=2.0), TypeError), (a, dict(metric="euclid"), ValueError),
        (a, dict(max_cost=0), ValueError), (a, dict(max_cost=1 << 40), ValueError), (a, dict(max_cost=1.5), TypeError),
        (a, dict(distance=4, max_cost=20), ValueError), (a, dict(distance=4, guide=g), ValueError), (a, dict(distance=0), ValueError),
        (a, dict(distance="4"), TypeError), (a, dict(return_cost=1), TypeError),
        (a, dict(out=a[:1].copy()), ValueError), (a, dict(out=a.astype(np.int64)), TypeError), (a, dict(out=ro), ValueError),
        (a, dict(out=torch.zeros((2, 8, 12), dtype=torch.int32)), ValueError), (a, dict(out=np.zeros((2, 8, 24), np.int32)[:, :, ::2]), ValueError),
    ]
    for seeds, kw, exc in cases:
        with pytest.raises(exc):
            t.propagate_batch(seeds, **kw)
    assert t._pre is None
    t.close()
    with pytest.raises(ValueError):
        PG.LabelPropagator(1, extractor=PG.LabelPropagator(0))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_counts_stay():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2 and lib.cs_profile_kernel_count() == 13
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_propagate", "cs_label_propagate_last_timing"):
        assert hasattr(raw, name) and name in L.SIGNATURES


C_TYPES = {"cs_preproc *": C.c_void_p, "const cs_preproc *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t *": C.c_void_p,
           "const uint8_t *": C.c_void_p, "const void *": C.c_void_p, "int64_t *": C.c_void_p, "int32_t": C.c_int32, "int": C.c_int,
           "const cs_propagate_params *": C.POINTER(L.CSPropagateParams), "double *": C.POINTER(C.c_double)}


def test_signatures_and_header_agree_on_the_two_calls():
    with open(os.path.join(ROOT, "include", "cellscreen.h")) as f:
        text = " ".join(f.read().split())
    assert ("typedef struct cs_propagate_params { int32_t metric; /* CS_PROPAGATE_* */ int32_t lam; /* 1..255 */ int32_t guide_channel; "
            "/* 0..guide_channels - 1; 0 without a guide */ int32_t reserved; /* must be 0 */ int64_t max_cost; /* 1..CS_PROPAGATE_NO_LIMIT */ } "
            "cs_propagate_params;") in text
    assert [n for n, _ in L.CSPropagateParams._fields_] == ["metric", "lam", "guide_channel", "reserved", "max_cost"]
    assert "#define CS_PROPAGATE_NO_LIMIT 1099511627774LL " in text and PG.NO_LIMIT == 1099511627774 and "#define CS_ABI_VERSION 2 " in text
    for k, name in enumerate(("CITYBLOCK", "CHESSBOARD", "CHAMFER")):
        assert f"#define CS_PROPAGATE_{name} {k} " in text and PG.METRICS[name.lower()] == k
    for name in ("cs_label_propagate", "cs_label_propagate_last_timing"):
        start = text.index(f"int {name}(")
        args = text[start + len(f"int {name}("):text.index(");", start)]
        args = " ".join(w for w in args.replace("/* or NULL */", "").split())
        types = []
        for arg in args.split(","):
            words = arg.split()
            stars = words[-1].count("*")
            types.append(" ".join(words[:-1]) + (" " + "*" * stars if stars else ""))
        res, sig = L.SIGNATURES[name]
        want = [C_TYPES[t] for t in types]
        if name.endswith("timing"):
            want[-1] = C.POINTER(C.c_int32)                                             # int32_t *rounds: typed in the binding
        assert res is C.c_int and len(sig) == len(want), name
        for s, w in zip(sig, want):
            assert s is w or (s is C.c_int and w is C.c_int32) or (s is C.c_int32 and w is C.c_int), (name, s, w)


def _call(lib, seeds=True, out=True, B=1, H=8, W=8, in_kind=0, out_kind=0, params=(2, 1, 0, 0, 100), mask=False, guide=False, gc=1, gt=0, cost=False):
    n = B * H * W if 0 < B * H * W <= 1 << 20 else 1
    a = np.zeros(n, np.int32)
    m, g, c = np.ones(n, np.uint8), np.zeros(n * max(1, min(gc, 4)), np.uint16), np.zeros(n, np.int64)
    p = None if params is None else L.CSPropagateParams(*params)
    rc = lib.cs_label_propagate(None, a.ctypes.data if seeds else None, B, H, W, in_kind, m.ctypes.data if mask else None,
                                g.ctypes.data if guide else None, gc, gt, None if p is None else C.byref(p), a.ctypes.data if out else None,
                                c.ctypes.data if cost else None, out_kind)
    return rc, lib.cs_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_the_handle():
    lib = L.load_library()
    for over, status in ((dict(seeds=False), -1), (dict(out=False), -1), (dict(params=None), -1), (dict(in_kind=2), -1), (dict(out_kind=-1), -1),
                         (dict(B=0), -1), (dict(H=0), -1), (dict(W=-1), -1), (dict(params=(3, 1, 0, 0, 100)), -1), (dict(params=(-1, 1, 0, 0, 100)), -1),
                         (dict(params=(2, 0, 0, 0, 100)), -1), (dict(params=(2, 256, 0, 0, 100)), -1), (dict(params=(2, 1, 0, 0, 0)), -1),
                         (dict(params=(2, 1, 0, 0, (1 << 40) - 1)), -1), (dict(params=(2, 1, 0, 1, 100)), -1), (dict(params=(2, 1, 1, 0, 100)), -1),
                         (dict(guide=True, gt=2), -1), (dict(guide=True, gc=0), -1), (dict(guide=True, gc=5), -1),
                         (dict(guide=True, gc=3, params=(2, 1, 3, 0, 100)), -1), (dict(guide=True, params=(2, 1, -1, 0, 100)), -1),
                         (dict(H=4097), -6), (dict(W=4097), -6), (dict(B=65536), -6), (dict(B=9, H=4096, W=4096), -6)):
        rc, text = _call(lib, **over)
        assert rc == status and text, over
    assert "lam 256 outside 1..255" in _call(lib, params=(2, 256, 0, 0, 100))[1]
    assert "max_cost 0 outside 1..1099511627774" in _call(lib, params=(2, 1, 0, 0, 0))[1]
    assert lib.cs_label_propagate_last_timing(None, None, None, None, None) == -1


def test_a_null_handle_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(params=(0, 1, 0, 0, 1)), dict(params=(1, 255, 0, 0, (1 << 40) - 2)), dict(mask=True, cost=True), dict(in_kind=1, out_kind=1),
                 dict(guide=True, gc=4, gt=1, params=(2, 8, 3, 0, 100)), dict(H=4096, W=4096), dict(B=8, H=4096, W=4096), dict(B=65535, H=1, W=1)):
        assert _call(lib, **over)[0] == (-4 if no_dev else -1), over      # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            PG.LabelPropagator(0).propagate_batch(np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
