"""The numpy restatement of cs_label_match (include/cellscreen.h) and of the statistics cellscreen/score.py takes
from its tables: object matching by intersection over union between a predicted and a true label image.  numpy only.

Per image, with A the pixel count of an object (a label value > 0, connected or not) and I(p, t) that of an intersection:
  partner   the object of the other image with the largest I, ties to the smaller label, 0 when it meets none
  n_major   the number of objects of the other image with 2 * I > A_other
  match at tq / 65536: p and t each other's partner, 2 * I > U and I * 65536 >= tq * U, with U = A_p + A_t - I.
Tables are int32 [B, max, 4] = area, partner, overlap, n_major, row l - 1 for label l."""
import numpy as np

THRESHOLDS = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9)


def tq_of(tau):
    tau = float(tau)
    if not 0.5 <= tau <= 1.0:
        raise ValueError(f"threshold {tau!r} outside [0.5, 1]")
    return int(tau * 65536 + 0.5)


def _one(pred, truth, max_pred, max_truth):
    p = pred.ravel().astype(np.int64)
    t = truth.ravel().astype(np.int64)
    if p.min() < 0 or t.min() < 0 or p.max() > max_pred or t.max() > max_truth:
        raise ValueError("a label is negative or above its max")
    code, n = np.unique(p * (max_truth + 1) + t, return_counts=True)
    cp, ct = code // (max_truth + 1), code % (max_truth + 1)
    ptab, ttab = np.zeros((max_pred, 4), np.int32), np.zeros((max_truth, 4), np.int32)
    a_p = np.bincount(p, minlength=max_pred + 1)
    a_t = np.bincount(t, minlength=max_truth + 1)
    ptab[:, 0], ttab[:, 0] = a_p[1:], a_t[1:]
    both = (cp > 0) & (ct > 0)
    cp, ct, n = cp[both], ct[both], n[both]
    for tab, own, other, a_other in ((ptab, cp, ct, a_t), (ttab, ct, cp, a_p)):
        order = np.lexsort((other, -n, own))                         # by own label, then the larger I, then the smaller label
        first = np.ones(order.size, bool)
        first[1:] = own[order][1:] != own[order][:-1]
        sel = order[first]
        tab[own[sel] - 1, 1] = other[sel]
        tab[own[sel] - 1, 2] = n[sel]
        major = 2 * n > a_other[other]
        tab[:, 3] = np.bincount(own[major], minlength=tab.shape[0] + 1)[1:]
    return ptab, ttab, int(cp.size)


def tables(pred, truth, max_pred, max_truth):
    """pred, truth: integer [B,H,W] (or [H,W], one image).  Returns (pred_table, truth_table, n_pairs): int32 [B,max_pred,4] and
    [B,max_truth,4], int64 [B]."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.shape != truth.shape or pred.ndim not in (2, 3):
        raise ValueError(f"shapes {pred.shape} and {truth.shape}")
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
    rows = [_one(a, b, int(max_pred), int(max_truth)) for a, b in zip(pred, truth)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int64)


def matches(ptab, ttab, tq):
    """[(p, t, I, U)] of one image at tq, in the order of p: plain Python integers."""
    out = []
    for row in range(ptab.shape[0]):
        a_p, t, i, _ = (int(v) for v in ptab[row])
        if t == 0 or int(ttab[t - 1, 1]) != row + 1:
            continue
        u = a_p + int(ttab[t - 1, 0]) - i
        if 2 * i > u and i * 65536 >= tq * u:
            out.append((row + 1, t, i, u))
    return out


def _ratio(a, b):
    return a / b if b else 0.0


def _scores(tp, fp, fn, n_true, s):
    return dict(tp=tp, fp=fp, fn=fn, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn), accuracy=_ratio(tp, tp + fp + fn),
                f1=_ratio(2 * tp, 2 * tp + fp + fn), mean_matched_score=_ratio(s, tp), mean_true_score=_ratio(s, n_true),
                panoptic_quality=_ratio(s, tp + fp / 2 + fn / 2))


def stats(tabs, thresholds=THRESHOLDS):
    """tabs: (pred_table, truth_table[, n_pairs]) of tables().  Returns {"thresholds": the thresholds as floats, "images": one
    entry per image, "total": one for the batch}; an entry holds n_pred, n_true, merged, split, missed, spurious and
    "by_threshold": per threshold a dict of tp, fp, fn, precision, recall, accuracy, f1, mean_matched_score, mean_true_score,
    panoptic_quality (StarDist's names and formulas; a zero denominator gives 0).  The sums of I / U are float64 additions one
    after another in (image, pred label) order; everything before the last division is Python integers."""
    ptabs, ttabs = np.asarray(tabs[0]), np.asarray(tabs[1])
    tqs = [tq_of(t) for t in thresholds]
    images = []
    tot = dict(n_pred=0, n_true=0, merged=0, split=0, missed=0, spurious=0)
    tot_rows = [[0, 0, 0, 0.0] for _ in tqs]
    for ptab, ttab in zip(ptabs, ttabs):
        pp, tp_ = ptab[ptab[:, 0] > 0], ttab[ttab[:, 0] > 0]
        e = dict(n_pred=int(pp.shape[0]), n_true=int(tp_.shape[0]), merged=int((pp[:, 3] >= 2).sum()), split=int((tp_[:, 3] >= 2).sum()),
                 missed=int((tp_[:, 1] == 0).sum()), spurious=int((pp[:, 1] == 0).sum()))
        for k in tot:
            tot[k] += e[k]
        e["by_threshold"] = []
        for k, tq in enumerate(tqs):
            m = matches(ptab, ttab, tq)
            s = 0.0
            for _, _, i, u in m:
                s += i / u
                tot_rows[k][3] += i / u
            tp, fp, fn = len(m), e["n_pred"] - len(m), e["n_true"] - len(m)
            tot_rows[k][0] += tp
            tot_rows[k][1] += fp
            tot_rows[k][2] += fn
            e["by_threshold"].append(dict(threshold=float(thresholds[k]), **_scores(tp, fp, fn, e["n_true"], s)))
        images.append(e)
    tot["by_threshold"] = [dict(threshold=float(thresholds[k]), **_scores(r[0], r[1], r[2], tot["n_true"], r[3]))
                           for k, r in enumerate(tot_rows)]
    return dict(thresholds=tuple(float(t) for t in thresholds), images=images, total=tot)


# ---- inputs the tests and the golden share --------------------------------------------------------------------------------------
def voronoi(shape, n, seed, background=0.0):
    """int32 labels 1..n (0 where `background` of the cells were dropped): the cells of n random sites."""
    rng = np.random.default_rng(seed)
    H, W = shape
    n = max(1, min(n, H * W))
    sy, sx = rng.integers(0, H, n), rng.integers(0, W, n)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    lab = (np.argmin(d, axis=2) + 1).astype(np.int32)
    if background > 0:
        drop = np.flatnonzero(rng.random(n) < background) + 1
        lab[np.isin(lab, drop)] = 0
    return lab


def shifted(lab, dy, dx):
    """`lab` moved by (dy, dx), 0 where nothing moves in."""
    out = np.zeros_like(lab)
    H, W = lab.shape
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[yd, xd] = lab[ys, xs]
    return out
