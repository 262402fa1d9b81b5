"""Generates tests/golden/golden_match.npz: small label pairs with TP / FP / FN of object matching by intersection over union
(cs_label_match) from an assignment solver, the outside witness of tests/match_reference.py.

    python tools/make_golden_match.py

The witness is StarDist's `matching` restated from its published form: the IoU matrix of the true and the predicted objects,
costs = -(ok) - IoU / (2 * min(n_true, n_pred)) with ok = IoU >= tau, scipy.optimize.linear_sum_assignment, TP = the assigned
pairs that are ok.  Two answers per pair and threshold:
    strict     ok also needs 2 * I > U: the rule of this project, whose matching needs no solver
    stardist   ok as published
Both compare in integers, I * 65536 >= int(tau * 65536 + 0.5) * U, so that no threshold falls between two float roundings.
Per case i:  pred_i, truth_i (int32, at most 64 x 64), name_i, strict_i and stardist_i (int64 [9, 3]: tp, fp, fn at tau = 0.5,
0.55 .. 0.9).  n_cases ordinary cases, then n_ties tie cases tie_pred_i ... where the two answers differ at tau = 0.5."""
import os
import sys

import numpy as np
import scipy
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_reference as MR                                                   # noqa: E402


def witness(pred, truth, tau, strict):
    """(tp, fp, fn) from the assignment solver on a dense contingency matrix."""
    pl, tl = [v for v in np.unique(pred) if v > 0], [v for v in np.unique(truth) if v > 0]
    if not pl or not tl:
        return 0, len(pl), len(tl)
    inter = np.array([[int(((truth == t) & (pred == p)).sum()) for p in pl] for t in tl], np.int64)
    a_p = np.array([int((pred == p).sum()) for p in pl], np.int64)
    a_t = np.array([int((truth == t).sum()) for t in tl], np.int64)
    union = a_t[:, None] + a_p[None, :] - inter
    tq = int(tau * 65536 + 0.5)
    ok = inter * 65536 >= tq * union
    if strict:
        ok &= 2 * inter > union
    costs = -ok.astype(float) - (inter / union) / (2 * min(len(pl), len(tl)))
    ti, pi = linear_sum_assignment(costs)
    tp = int(ok[ti, pi].sum())
    return tp, len(pl) - tp, len(tl) - tp


def cases():
    out = []
    for seed, shape, n, bg in ((1, (48, 64), 14, 0.0), (2, (64, 40), 25, 0.3), (3, (33, 47), 9, 0.2), (4, (64, 64), 40, 0.4),
                               (5, (17, 63), 6, 0.0), (6, (50, 30), 18, 0.5)):
        a = MR.voronoi(shape, n, seed, bg)
        for dy, dx in ((1, 0), (2, -3), (-4, 5)):
            out.append((f"voronoi{seed} shifted {dy},{dx}", MR.shifted(a, dy, dx), a))
        out.append((f"voronoi{seed} against voronoi{seed + 10}", MR.voronoi(shape, n + 3, seed + 10, bg), a))
    a = MR.voronoi((40, 56), 16, 21, 0.25)
    out.append(("identical", a.copy(), a))
    merged = a.copy()
    for k in (2, 5, 9, 12):
        merged[merged == k] = k - 1                                             # pred merges neighbours of the id order
    out.append(("merged", merged, a))
    out.append(("split", a, merged))
    yy, xx = np.mgrid[0:40, 0:56]
    halves = np.where(a > 0, 2 * a - (xx % 2), 0).astype(np.int32)             # every object cut into interleaved columns: disconnected
    out.append(("interleaved halves", halves, a))
    out.append(("disconnected", np.where(a > 8, a - 8, a).astype(np.int32), MR.shifted(a, 1, 1)))
    out.append(("gaps in the ids", (MR.shifted(a, 0, 2) * 7).astype(np.int32), (a * 3).astype(np.int32)))
    out.append(("empty pred", np.zeros_like(a), a))
    out.append(("empty truth", a, np.zeros_like(a)))
    out.append(("both empty", np.zeros_like(a), np.zeros_like(a)))
    return out


def ties():
    t = np.zeros((8, 12), np.int32)
    t[1:5, 1:5] = 1                                                             # 16 px
    p = np.zeros_like(t)
    p[1:5, 1:3], p[1:5, 3:5] = 1, 2                                             # cut exactly in half: IoU 1/2 twice
    out = [("cut exactly in half", p, t)]
    t = np.zeros((8, 12), np.int32)
    t[1:3, 1:5], t[3:8, 0:12] = 1, 2                                            # 8 px beside a large neighbour
    p = np.zeros_like(t)
    p[1:3, 3:5], p[3:8, 0:12] = 1, 2                                            # half of the small one, all of the neighbour
    out.append(("a half facing a larger neighbour", p, t))
    return out


def main():
    out = {}
    taus = MR.THRESHOLDS
    for prefix, items in (("", cases()), ("tie_", ties())):
        out["n_ties" if prefix else "n_cases"] = np.int64(len(items))
        for i, (name, pred, truth) in enumerate(items):
            assert pred.shape == truth.shape and max(pred.shape) <= 64 and pred.dtype == truth.dtype == np.int32
            out[f"{prefix}name_{i}"] = np.array(name)
            out[f"{prefix}pred_{i}"], out[f"{prefix}truth_{i}"] = pred, truth
            out[f"{prefix}strict_{i}"] = np.array([witness(pred, truth, t, True) for t in taus], np.int64)
            out[f"{prefix}stardist_{i}"] = np.array([witness(pred, truth, t, False) for t in taus], np.int64)
            if prefix:
                assert (out[f"tie_strict_{i}"][0] != out[f"tie_stardist_{i}"][0]).any(), name
                assert (out[f"tie_strict_{i}"][1:] == out[f"tie_stardist_{i}"][1:]).all(), name
    out["thresholds"] = np.array(taus)
    out["versions"] = np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_match.npz")
    np.savez_compressed(path, **out)
    differ = sum(int((out[f"strict_{i}"] != out[f"stardist_{i}"]).any()) for i in range(int(out["n_cases"])))
    print("wrote", path, os.path.getsize(path), "bytes,", int(out["n_cases"]), "cases,", int(out["n_ties"]), "ties;",
          differ, "ordinary cases where the two rules differ")


if __name__ == "__main__":
    main()
