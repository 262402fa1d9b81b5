"""The rule of cs_label_colocalize restated in numpy integers and Python ints: no tiles, no runs and no tables in
between, so that it shares nothing with the kernels.  The rule is this project's; it corresponds to CellProfiler's
MeasureColocalization (correlation, slope, Manders, overlap, K, rank-weighted coefficients; thresholds as a fraction of the
object's maximum) and to scipy.stats.pearsonr / linregress / rankdata(method='dense'), without a promise of bit equality with
CellProfiler.

An object is cs_label_intensity's: the pixels of one image with one label in 1..max_label, connected or not, less the pixels where
`exclude` is non-zero.  Channels C = 2..4; the pairs (i, j), i < j, in lexicographic order, P = C (C - 1) / 2.  A pixel is "above"
in channel c iff v * den >= num * max_c (threshold=(num, den), max_c the object's own maximum; a tie is above), or iff v >= t_c
(absolute=[t_0..]); "both" of a pair: above in both.  With rwc, per image and channel, the dense rank of a value among the values
on the image's object pixels (0 upwards, R_c distinct values), R = max(R_i, R_j) and w = R - |rank_i - rank_j|.  The tables:

    geom   [B, max_label, 3]     int64   area, sum r, sum c                                   (cs_label_intensity's)
    chan   [B, max_label, C, 5]  int64   sum v, sum v^2, max v, n_above, sum v[above]
    pair   [B, max_label, P, 9]  int64   sum v_i v_j (all pixels); over both: n, sum v_i, sum v_j, sum v_i^2, sum v_j^2,
                                         sum v_i v_j, sum v_i w, sum v_j w (the last two zero without rwc)
    levels [B, C]                int32   R_c, zeros without rwc

measure() is the vectorised form (a stable sort by label and np.add.reduceat on int64), measure_slow() gathers the pixels of
every object and works in Python ints and fractions.Fraction, and also returns the derived values that are rational as exact
Fractions.  derive() takes the floats a table reports from the integers."""
import math
from fractions import Fraction

import numpy as np

from intensity_reference import _planes, contents, disks, noise        # noqa: F401  (the generators, for the tests and tools)

FIELDS = ("pearson", "slope", "overlap", "k1", "k2", "manders1", "manders2", "rwc1", "rwc2")


def pairs_of(C):
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def _rule(C, threshold, absolute):
    """(num, den, None) or (None, None, [t_c])"""
    if absolute is not None:
        t = [int(x) for x in absolute]
        if len(t) != C or any(not 0 <= x <= 65536 for x in t):
            raise ValueError("absolute: one threshold in 0..65536 per channel")
        return None, None, t
    num, den = (int(x) for x in threshold)
    if not (0 <= num <= den and 1 <= den <= 65536):
        raise ValueError("threshold: 0 <= num <= den, den in 1..65536")
    return num, den, None


def measure(image, labels, exclude=None, max_label=None, threshold=(15, 100), absolute=None, rwc=True):
    """(geom, chan, pair, levels) of image [B,H,W,C], labels [B,H,W] and exclude (None or [B,H,W])."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    B, C = labels.shape[0], image.shape[3]
    if not 2 <= C <= 4:
        raise ValueError("2 to 4 channels")
    num, den, tabs = _rule(C, threshold, absolute)
    pp = pairs_of(C)
    geom = np.zeros((B, max_label, 3), np.int64)
    chan = np.zeros((B, max_label, C, 5), np.int64)
    pair = np.zeros((B, max_label, len(pp), 9), np.int64)
    levels = np.zeros((B, C), np.int32)
    for b in range(B):
        rr, cc = np.nonzero((labels[b] > 0) & (exclude[b] == 0))
        if rr.size == 0:
            continue
        lab = labels[b][rr, cc].astype(np.int64)
        order = np.argsort(lab, kind="stable")
        lab, rr, cc = lab[order], rr[order].astype(np.int64), cc[order].astype(np.int64)
        starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
        rows = lab[starts] - 1
        seg = np.cumsum(np.r_[False, lab[1:] != lab[:-1]])             # the object of every pixel, 0..
        add = lambda x: np.add.reduceat(x.astype(np.int64), starts)
        geom[b, rows, 0] = add(np.ones_like(lab))
        geom[b, rows, 1] = add(rr)
        geom[b, rows, 2] = add(cc)
        v = [image[b][rr, cc, ch].astype(np.int64) for ch in range(C)]
        above, rank = [], []
        for ch in range(C):
            top = np.maximum.reduceat(v[ch], starts)
            up = v[ch] >= tabs[ch] if tabs is not None else v[ch] * den >= num * top[seg]
            above.append(up)
            chan[b, rows, ch, 0] = add(v[ch])
            chan[b, rows, ch, 1] = add(v[ch] * v[ch])
            chan[b, rows, ch, 2] = top
            chan[b, rows, ch, 3] = add(up)
            chan[b, rows, ch, 4] = add(v[ch] * up)
            if rwc:
                vals, inv = np.unique(v[ch], return_inverse=True)
                levels[b, ch] = vals.size
                rank.append(inv.astype(np.int64).reshape(-1))
        for p, (i, j) in enumerate(pp):
            both = (above[i] & above[j]).astype(np.int64)
            cols = [v[i] * v[j], both, v[i] * both, v[j] * both, v[i] * v[i] * both, v[j] * v[j] * both, v[i] * v[j] * both]
            if rwc:
                w = max(int(levels[b, i]), int(levels[b, j])) - np.abs(rank[i] - rank[j])
                cols += [v[i] * w * both, v[j] * w * both]
            for k, x in enumerate(cols):
                pair[b, rows, p, k] = add(x)
    return geom, chan, pair, levels


def measure_slow(image, labels, exclude=None, max_label=None, threshold=(15, 100), absolute=None, rwc=True):
    """measure(), object by object over all its pixels in Python ints and Fractions.  Returns (geom, chan, pair, levels, exact):
    exact[(b, label, p)] is a dict of the derived values as Fractions or None (a zero denominator): slope, k1, k2, manders1,
    manders2, rwc1, rwc2, and pearson2 / overlap2, the squares of the two that need a root, with pearson_sign."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    B, H, W = labels.shape
    C = image.shape[3]
    num, den, tabs = _rule(C, threshold, absolute)
    frac = None if tabs is not None else Fraction(num, den)
    pp = pairs_of(C)
    geom = np.zeros((B, max_label, 3), np.int64)
    chan = np.zeros((B, max_label, C, 5), np.int64)
    pair = np.zeros((B, max_label, len(pp), 9), np.int64)
    levels = np.zeros((B, C), np.int32)
    exact = {}
    div = lambda a, b: Fraction(a, b) if b != 0 else None
    for b in range(B):
        objs = {}
        for r in range(H):
            for c in range(W):
                lab = int(labels[b, r, c])
                if lab != 0 and int(exclude[b, r, c]) == 0:
                    objs.setdefault(lab, []).append((r, c, tuple(int(x) for x in image[b, r, c])))
        ranks = []
        for ch in range(C):
            vals = sorted({px[2][ch] for pxs in objs.values() for px in pxs})
            ranks.append({x: k for k, x in enumerate(vals)})
            if rwc:
                levels[b, ch] = len(vals)
        for lab, pxs in objs.items():
            n = len(pxs)
            geom[b, lab - 1] = n, sum(p[0] for p in pxs), sum(p[1] for p in pxs)
            vs = [p[2] for p in pxs]
            top = [max(v[ch] for v in vs) for ch in range(C)]
            up = [[(v[ch] >= tabs[ch]) if tabs is not None else (Fraction(v[ch]) >= frac * top[ch]) for v in vs] for ch in range(C)]
            S = [sum(v[ch] for v in vs) for ch in range(C)]
            S2 = [sum(v[ch] ** 2 for v in vs) for ch in range(C)]
            SA = [sum(v[ch] for v, u in zip(vs, up[ch]) if u) for ch in range(C)]
            for ch in range(C):
                chan[b, lab - 1, ch] = S[ch], S2[ch], top[ch], sum(up[ch]), SA[ch]
            for p, (i, j) in enumerate(pp):
                sij = sum(v[i] * v[j] for v in vs)
                bv = [v for v, a, c in zip(vs, up[i], up[j]) if a and c]
                bi, bj = sum(v[i] for v in bv), sum(v[j] for v in bv)
                bii, bjj, bij = sum(v[i] ** 2 for v in bv), sum(v[j] ** 2 for v in bv), sum(v[i] * v[j] for v in bv)
                R = max(len(ranks[i]), len(ranks[j]))
                ws = [R - abs(ranks[i][v[i]] - ranks[j][v[j]]) for v in bv]
                assert all(1 <= w <= 65536 for w in ws)
                biw, bjw = sum(v[i] * w for v, w in zip(bv, ws)), sum(v[j] * w for v, w in zip(bv, ws))
                pair[b, lab - 1, p] = sij, len(bv), bi, bj, bii, bjj, bij, biw if rwc else 0, bjw if rwc else 0
                cov, di, dj = n * sij - S[i] * S[j], n * S2[i] - S[i] ** 2, n * S2[j] - S[j] ** 2
                exact[(b, lab, p)] = dict(
                    pearson2=div(cov * cov, di * dj), pearson_sign=(cov > 0) - (cov < 0), slope=div(cov, di),
                    overlap2=div(bij * bij, bii * bjj), k1=div(bij, bii), k2=div(bij, bjj), manders1=div(bi, SA[i]),
                    manders2=div(bj, SA[j]), rwc1=div(biw, R * SA[i]) if rwc else None, rwc2=div(bjw, R * SA[j]) if rwc else None)
    return geom, chan, pair, levels, exact


def ratio(a, b):
    """a / b of Python ints, correctly rounded; NaN where b is 0"""
    return a / b if b != 0 else math.nan


def over_root(a, b):
    """a / sqrt(b) of Python ints: b to float64, its root, a to float64, one division; NaN where b is 0"""
    return a / math.sqrt(b) if b != 0 else math.nan


def derive(geom, chan, pair, levels, rwc=True):
    """The present objects in (image, label) order as a dict of arrays: image, label, area [n], the nine floats of FIELDS [n,P]
    (NaN where a denominator is 0; rwc1 / rwc2 NaN without rwc), and the integer records geom [n,3], chan [n,C,5], pair [n,P,9]."""
    B, M, C = chan.shape[:3]
    pp = pairs_of(C)
    keys = [(b, m) for b in range(B) for m in range(M) if geom[b, m, 0] > 0]
    n = len(keys)
    out = dict(image=np.array([b for b, _ in keys], np.int32).reshape(n), label=np.array([m + 1 for _, m in keys], np.int32).reshape(n),
               area=np.zeros(n, np.int64), geom=np.zeros((n, 3), np.int64), chan=np.zeros((n, C, 5), np.int64),
               pair=np.zeros((n, len(pp), 9), np.int64))
    for f in FIELDS:
        out[f] = np.full((n, len(pp)), np.nan)
    for k, (b, m) in enumerate(keys):
        a = int(geom[b, m, 0])
        out["area"][k], out["geom"][k], out["chan"][k], out["pair"][k] = a, geom[b, m], chan[b, m], pair[b, m]
        for p, (i, j) in enumerate(pp):
            si, si2, _, _, ai = (int(x) for x in chan[b, m, i])
            sj, sj2, _, _, aj = (int(x) for x in chan[b, m, j])
            sij, _, bi, bj, bii, bjj, bij, biw, bjw = (int(x) for x in pair[b, m, p])
            cov, di, dj = a * sij - si * sj, a * si2 - si * si, a * sj2 - sj * sj
            out["pearson"][k, p] = over_root(cov, di * dj)
            out["slope"][k, p] = ratio(cov, di)
            out["overlap"][k, p] = over_root(bij, bii * bjj)
            out["k1"][k, p], out["k2"][k, p] = ratio(bij, bii), ratio(bij, bjj)
            out["manders1"][k, p], out["manders2"][k, p] = ratio(bi, ai), ratio(bj, aj)
            if rwc:
                R = max(int(levels[b, i]), int(levels[b, j]))
                out["rwc1"][k, p], out["rwc2"][k, p] = ratio(biw, R * ai), ratio(bjw, R * aj)
    return out


def derive_decimal(geom, chan, pair, levels, rwc=True, digits=50):
    """derive()'s nine fields in `digits`-digit decimal arithmetic on the same integers: {field: [n][P] of Decimal, or None where a
    denominator is 0}, the objects in derive()'s order.  What the float64 derivation and SciPy's floats are measured against."""
    import decimal
    ctx = decimal.Context(prec=digits)
    D = decimal.Decimal
    div = lambda a, b: ctx.divide(D(a), D(b)) if b != 0 else None
    root = lambda a, b: ctx.divide(D(a), ctx.sqrt(D(b))) if b != 0 else None
    B, M, C = chan.shape[:3]
    pp = pairs_of(C)
    out = {f: [] for f in FIELDS}
    for b in range(B):
        for m in range(M):
            a = int(geom[b, m, 0])
            if a == 0:
                continue
            row = {f: [] for f in FIELDS}
            for p, (i, j) in enumerate(pp):
                si, si2, _, _, ai = (int(x) for x in chan[b, m, i])
                sj, sj2, _, _, aj = (int(x) for x in chan[b, m, j])
                sij, _, bi, bj, bii, bjj, bij, biw, bjw = (int(x) for x in pair[b, m, p])
                cov, di, dj = a * sij - si * sj, a * si2 - si * si, a * sj2 - sj * sj
                R = max(int(levels[b, i]), int(levels[b, j]))
                vals = dict(pearson=root(cov, di * dj), slope=div(cov, di), overlap=root(bij, bii * bjj), k1=div(bij, bii), k2=div(bij, bjj),
                            manders1=div(bi, ai), manders2=div(bj, aj), rwc1=div(biw, R * ai) if rwc else None,
                            rwc2=div(bjw, R * aj) if rwc else None)
                for f in FIELDS:
                    row[f].append(vals[f])
            for f in FIELDS:
                out[f].append(row[f])
    return out
