"""CPU tests of the label scoring (cs_label_match, cellscreen/score.py): the restatement of tests/match_reference.py
against a brute force over a dense contingency matrix and against the assignment solver's answers in tests/golden/golden_match.npz
(tie cases included), the uniqueness of the matching, the identities of the statistics, the scene table of DESIGN 3s, and the
wrapper's and the C ABI's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import match_arg_cases as MA
import match_reference as MR
import noise_reference as NR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import score as SC
from cellscreen import segment as S
from test_local_cpu import dim_cell_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_match.npz")


# ---- the brute force: plain loops over a dense matrix, no code shared with the restatement -------------------------------------------
def brute_tables(pred, truth, max_pred, max_truth):
    M = [[0] * (max_truth + 1) for _ in range(max_pred + 1)]
    for y in range(pred.shape[0]):
        for x in range(pred.shape[1]):
            M[int(pred[y, x])][int(truth[y, x])] += 1
    a_p = [sum(row) for row in M]
    a_t = [sum(M[p][t] for p in range(max_pred + 1)) for t in range(max_truth + 1)]
    ptab, ttab = np.zeros((max_pred, 4), np.int32), np.zeros((max_truth, 4), np.int32)
    pairs = 0
    for p in range(1, max_pred + 1):
        best, bt, major = 0, 0, 0
        for t in range(1, max_truth + 1):
            i = M[p][t]
            pairs += i > 0
            if i > best:                                                # strictly: ties stay with the smaller label
                best, bt = i, t
            major += i > 0 and 2 * i > a_t[t]
        ptab[p - 1] = (a_p[p], bt, best, major)
    for t in range(1, max_truth + 1):
        best, bp, major = 0, 0, 0
        for p in range(1, max_pred + 1):
            i = M[p][t]
            if i > best:
                best, bp = i, p
            major += i > 0 and 2 * i > a_p[p]
        ttab[t - 1] = (a_t[t], bp, best, major)
    return ptab, ttab, pairs


def small_cases():
    rng = np.random.default_rng(5)
    out = []
    for shape in ((1, 1), (1, 9), (7, 1), (5, 7), (12, 13), (16, 20)):
        for k in range(4):
            mp, mt = int(rng.integers(1, 7)), int(rng.integers(1, 7))
            out.append((rng.integers(0, mp + 1, shape).astype(np.int32), rng.integers(0, mt + 1, shape).astype(np.int32), mp + k % 2, mt + 1))
        a = MR.voronoi(shape, 5, shape[0] + shape[1], 0.3)
        out.append((a, MR.shifted(a, 1, 1), 5, 5))
        out.append((a, a.copy(), 5, 6))
        out.append((np.zeros(shape, np.int32), a, 1, 5))
        out.append((a, np.zeros(shape, np.int32), 5, 1))
    return out


def test_restatement_equals_the_brute_force():
    for pred, truth, mp, mt in small_cases():
        pt, tt, n = MR.tables(pred, truth, mp, mt)
        bp, bt, bn = brute_tables(pred, truth, mp, mt)
        assert pt.dtype == np.int32 and pt.shape == (1, mp, 4) and tt.shape == (1, mt, 4) and n.dtype == np.int64
        assert np.array_equal(pt[0], bp) and np.array_equal(tt[0], bt) and int(n[0]) == bn, (pred.shape, mp, mt)
    with pytest.raises(ValueError):
        MR.tables(np.full((2, 2), 3, np.int32), np.zeros((2, 2), np.int32), 2, 1)
    with pytest.raises(ValueError):
        MR.tables(np.zeros((2, 2), np.int32), np.full((2, 2), -1, np.int32), 2, 1)


def _tpfpfn(pred, truth, thresholds=MR.THRESHOLDS):
    s = MR.stats(MR.tables(pred, truth, max(1, int(pred.max())), max(1, int(truth.max()))), thresholds)
    return np.array([[r["tp"], r["fp"], r["fn"]] for r in s["total"]["by_threshold"]], np.int64)


def test_restatement_equals_the_assignment_solver_of_the_golden():
    g = np.load(GOLDEN)
    assert tuple(g["thresholds"]) == MR.THRESHOLDS and 24 <= int(g["n_cases"]) <= 36 and int(g["n_ties"]) == 2
    names = set()
    for i in range(int(g["n_cases"])):
        pred, truth = g[f"pred_{i}"], g[f"truth_{i}"]
        assert pred.dtype == np.int32 and max(pred.shape) <= 64
        names.add(str(g[f"name_{i}"]))
        assert np.array_equal(_tpfpfn(pred, truth), g[f"strict_{i}"]), str(g[f"name_{i}"])
        assert np.array_equal(_tpfpfn(truth, pred), g[f"strict_{i}"][:, [0, 2, 1]]), str(g[f"name_{i}"])    # the other direction
        assert np.array_equal(g[f"strict_{i}"][1:], g[f"stardist_{i}"][1:])          # the rules can differ at 0.5 alone
    assert {"identical", "merged", "split", "disconnected", "gaps in the ids", "empty pred", "empty truth"} <= names
    assert len(names) == int(g["n_cases"])


def test_tie_cases_pin_the_difference_from_stardist():
    g = np.load(GOLDEN)
    for i in range(int(g["n_ties"])):
        pred, truth = g[f"tie_pred_{i}"], g[f"tie_truth_{i}"]
        strict, plain = g[f"tie_strict_{i}"], g[f"tie_stardist_{i}"]
        assert np.array_equal(_tpfpfn(pred, truth), strict) and np.array_equal(_tpfpfn(truth, pred), strict[:, [0, 2, 1]])
        assert plain[0, 0] == strict[0, 0] + 1 and np.array_equal(plain[1:], strict[1:])    # one more pair at 0.5, IoU exactly 1/2
    # cut exactly in half: both halves have IoU 1/2 with the object and neither matches; the partner is the smaller label
    pred, truth = g["tie_pred_0"], g["tie_truth_0"]
    pt, tt, n = MR.tables(pred, truth, 2, 1)
    assert pt[0].tolist() == [[8, 1, 8, 0], [8, 1, 8, 0]] and tt[0].tolist() == [[16, 1, 8, 2]] and int(n[0]) == 2
    assert MR.matches(pt[0], tt[0], 32768) == []


def test_no_object_appears_in_two_matches():
    rng = np.random.default_rng(11)
    seen = 0
    for k in range(300):
        shape = (int(rng.integers(8, 40)), int(rng.integers(8, 40)))
        a = MR.voronoi(shape, int(rng.integers(1, 14)), 1000 + k, 0.25)
        kind = k % 4
        if kind == 0:
            b = MR.shifted(a, int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        elif kind == 1:
            b = MR.voronoi(shape, int(rng.integers(1, 14)), 5000 + k, 0.25)
        elif kind == 2:
            b = np.where(a > 0, (a + 1) // 2, 0).astype(np.int32)      # merged in pairs
        else:
            xx = np.arange(shape[1])[None, :]
            b = np.where(a > 0, 2 * a - (xx % 2), 0).astype(np.int32)  # halved, often exactly
        pt, tt, _ = MR.tables(b, a, max(1, int(b.max())), max(1, int(a.max())))
        for tq in (32768, 36045, 49152, 65536):
            m = MR.matches(pt[0], tt[0], tq)
            assert len({p for p, _, _, _ in m}) == len(m) == len({t for _, t, _, _ in m})
            for p, t, i, u in m:                                        # and each is the unique largest overlap of both
                assert 2 * i > int(pt[0, p - 1, 0]) and 2 * i > int(tt[0, t - 1, 0]) and u == int(pt[0, p - 1, 0]) + int(tt[0, t - 1, 0]) - i
            seen += len(m)
    assert seen > 1000


def test_stats_identities_and_the_package_agrees():
    a = MR.voronoi((40, 50), 12, 1, 0.2)
    b = MR.shifted(a, 2, -3)
    z = np.zeros_like(a)
    P, T = np.stack([a, b, z, a, z]), np.stack([a, a, a, z, z])
    tabs = MR.tables(P, T, 12, 13)
    s = MR.stats(tabs)
    assert SC.LabelMatch(*tabs).stats() == s and SC.LabelMatch(*tabs).stats((0.5, 1)) == MR.stats(tabs, (0.5, 1))
    assert s["thresholds"] == MR.THRESHOLDS and len(s["images"]) == 5
    for e in s["images"] + [s["total"]]:
        for r in e["by_threshold"]:
            assert r["tp"] + r["fp"] == e["n_pred"] and r["tp"] + r["fn"] == e["n_true"]
            assert all(isinstance(r[k], int) for k in ("tp", "fp", "fn")) and all(0.0 <= r[k] <= 1.0 for k in r if k not in ("tp", "fp", "fn"))
    n = int((np.unique(a) > 0).sum())
    for r in s["images"][0]["by_threshold"]:                            # identical images: everything is 1
        assert (r["tp"], r["fp"], r["fn"]) == (n, 0, 0)
        assert all(r[k] == 1.0 for k in ("precision", "recall", "accuracy", "f1", "mean_matched_score", "mean_true_score", "panoptic_quality"))
    for j, (n_pred, n_true) in ((2, (0, n)), (3, (n, 0)), (4, (0, 0))):  # empty pred, empty truth, both: zeros, no division error
        e = s["images"][j]
        assert (e["n_pred"], e["n_true"]) == (n_pred, n_true) and e["missed"] == n_true and e["spurious"] == n_pred
        for r in e["by_threshold"]:
            assert (r["tp"], r["fp"], r["fn"]) == (0, n_pred, n_true)
            assert all(r[k] == 0.0 for k in ("precision", "recall", "accuracy", "f1", "mean_matched_score", "mean_true_score", "panoptic_quality"))
    t = s["total"]
    assert t["n_pred"] == sum(e["n_pred"] for e in s["images"]) and t["by_threshold"][0]["tp"] == sum(e["by_threshold"][0]["tp"] for e in s["images"])
    tps = [r["tp"] for r in s["images"][1]["by_threshold"]]
    assert tps == sorted(tps, reverse=True) and tps[0] > tps[-1]         # a higher threshold never matches more
    assert MR.tq_of(0.5) == SC.threshold_q16(0.5) == 32768 and SC.threshold_q16(1) == 65536 and SC.threshold_q16(0.55) == 36045


# ---- the scene table of DESIGN 3s -------------------------------------------------------------------------------------------------
def disk_truth(cells, side=512):
    yy, xx = np.mgrid[0:side, 0:side]
    t = np.zeros((side, side), np.int32)
    for k, (y, x, rad, _) in enumerate(cells):
        t[(yy - y) ** 2 + (xx - x) ** 2 <= rad * rad] = k + 1
    return t


def test_scene_table():
    got = {}
    for seed in (0, 1):
        img, cells = dim_cell_scene(seed)
        truth = disk_truth(cells)
        assert len(np.unique(truth)) == 41                              # the cells do not overlap
        for rule, plane in (("otsu", img > R.otsu(img)), ("k6w3", NR.noise_mask(img, 64, 1536, 768) > 0)):
            lab, n = R.label_mask(plane, 1)[:2]
            got[seed, rule] = (int(n), MR.stats(MR.tables(lab.astype(np.int32), truth, max(1, int(n)), 40), (0.5, 0.7))["total"])
    tpfpfn = lambda e, k: tuple(e["by_threshold"][k][c] for c in ("tp", "fp", "fn"))
    n, e = got[0, "otsu"]
    assert n == 20 and tpfpfn(e, 0) == (20, 0, 20) and tpfpfn(e, 1) == (20, 0, 20) and e["missed"] == 20
    n, e = got[0, "k6w3"]
    assert n == 40 and tpfpfn(e, 0) == (40, 0, 0) and tpfpfn(e, 1) == (20, 20, 20) and e["merged"] == 0      # the dim rims: IoU about 0.6
    n, e = got[1, "k6w3"]
    assert n == 38 and tpfpfn(e, 0) == (36, 2, 4) and tpfpfn(e, 1) == (19, 19, 21)
    assert e["merged"] == 2 and e["missed"] == 0 and e["split"] == 0 and e["spurious"] == 0   # two components swallow two cells each:
    assert e["n_true"] - e["by_threshold"][0]["tp"] == 2 * e["merged"]                         # they account for the four lost cells


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------
def test_match_params_and_thresholds_refuse_every_bad_value():
    for v, exc in ((9, ValueError), (27, ValueError), (0, ValueError), (-1, ValueError), (True, TypeError), (12.0, TypeError), ("12", TypeError)):
        with pytest.raises(exc):
            SC.match_params(v)
        with pytest.raises(exc):
            SC.LabelMatcher(0, table_log2=v)
    assert (SC.match_params().table_log2, SC.match_params().reserved) == (0, 0) and SC.match_params(np.int64(10)).table_log2 == 10
    assert SC.match_params(26).table_log2 == 26 and C.sizeof(L.CSMatchParams) == 8
    m = SC.LabelMatch(*MR.tables(np.ones((1, 2, 2), np.int32), np.ones((1, 2, 2), np.int32), 1, 1))
    for tau, exc in ((0.49, ValueError), (1.01, ValueError), (0, ValueError), (float("nan"), ValueError), (-0.5, ValueError), ("0.5", TypeError),
                     (None, TypeError), (True, TypeError)):
        with pytest.raises(exc):
            m.stats((0.5, tau))
        with pytest.raises(exc):
            SC.threshold_q16(tau)
    with pytest.raises(ValueError):
        m.stats(())
    with pytest.raises(ValueError):
        MR.stats((m.pred, m.truth), (0.4,))
    assert m.stats(0.75)["total"]["by_threshold"][0]["tp"] == 1


def test_matcher_refusals_before_a_handle_exists():
    import torch
    m = SC.LabelMatcher(0)
    a = np.zeros((2, 8, 12), np.int32)
    for pred, truth, kw, exc in ((a.astype(np.int64), a, {}, TypeError), (a, a.astype(np.uint16), {}, TypeError), (a, a[:, :, :8].copy(), {}, ValueError),
                                 (a[:, :, ::2], a[:, :, ::2], {}, ValueError), (a, a.transpose(0, 2, 1), {}, ValueError),
                                 (a[0], a[0], {}, ValueError), (a[:0], a[:0], {}, ValueError), (list(a), a, {}, TypeError),
                                 (torch.zeros((2, 8, 12), dtype=torch.int32), a, {}, ValueError),                  # a CPU tensor
                                 (a, torch.zeros((2, 8, 12), dtype=torch.int64), {}, TypeError),
                                 (np.zeros((1, 2, 4097), np.int32), np.zeros((1, 2, 4097), np.int32), {}, ValueError),
                                 (a, a, dict(max_pred=0), ValueError), (a, a, dict(max_truth=(1 << 20) + 1), ValueError),
                                 (a, a, dict(max_pred=(1 << 21) + 1), ValueError), (a, a, dict(max_pred=2.0), TypeError),
                                 (a, a, dict(max_truth=True), TypeError)):
        with pytest.raises(exc):
            m.match_batch(pred, truth, **kw)
    assert m._pre is None
    s = S.ThresholdSegmenter(0)
    img = np.zeros((2, 8, 12), np.uint16)
    for im, truth, kw, exc in ((img, a.astype(np.int64), {}, TypeError), (img, a[:1], {}, ValueError), (img, a[:, :, ::2], {}, ValueError),
                               (img, a, dict(thresholds=(0.4,)), ValueError), (img.astype(np.float32), a, {}, TypeError),
                               (img, torch.zeros((2, 8, 12), dtype=torch.int32), {}, ValueError)):
        with pytest.raises(exc):
            s.score_batch(im, truth, **kw)
    assert s._pre is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = L.load_library()
    assert lib.cs_abi_version() == 2
    raw = C.CDLL(L.LIB_PATH)
    for name in ("cs_label_match", "cs_label_match_last_timing", "cs_label_match_last_table"):
        assert hasattr(raw, name) and name in L.SIGNATURES


def test_c_abi_refusals_status_and_text():
    lib = L.load_library()
    names = set()
    for over, status, text in MA.CASES:
        assert MA.call(lib, over) == (status, text), over
        names.add(tuple(sorted((k, repr(v)) for k, v in over.items())))
    assert len(names) == len(MA.CASES) >= 40                          # no case twice
    assert lib.cs_label_match_last_timing(None, None, None) == -1 and lib.cs_label_match_last_table(None, None, None) == -1


def test_c_abi_reports_no_device_for_valid_arguments():
    lib = L.load_library()
    no_dev = lib.cs_device_count() <= 0
    for over in (dict(), dict(params=None), dict(params=(10, 0)), dict(params=(26, 0)), dict(pairs=None), dict(kind=1, tkind=1),
                 dict(mp=1 << 20, mt=1 << 20), dict(B=4, mp=1 << 20), dict(H=4096, W=4096)):
        assert MA.call(lib, over)[0] == (-4 if no_dev else -1), over  # no handle: no device here, else a NULL handle
    if no_dev:
        with pytest.raises(L.CellScreenError) as ei:
            SC.LabelMatcher(0).match_batch(np.zeros((1, 8, 8), np.int32), np.zeros((1, 8, 8), np.int32))
        assert ei.value.status == -4
