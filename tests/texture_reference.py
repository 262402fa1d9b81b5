"""The rule of cs_label_texture restated in numpy integers: no tiles, no bounding boxes and no triangles, so that it
shares nothing with the kernels.  Per direction one shifted comparison of whole planes, then np.add.at.

An object is cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  Per channel a value v becomes the level

    q(v) = ((min(max(v, lo), hi) - lo) * levels) // (hi - lo + 1)           2 <= levels <= 64, 0 <= lo <= hi <= 65535

With one distance d, 1..127, the directions k = 0..3 have the (row, column) steps (0, d), (d, d), (d, 0), (d, -d).  The pair
(p, p + step_k) counts iff both pixels lie in the image, carry the same label > 0 and neither is excluded; it adds 1 to
G[k][q(p)][q(p')] and 1 to G[k][q(p')][q(p)].  The dense records, row label - 1 for label `label`:

    count [B, max_label]                    int32    the pixels of the object
    marg  [B, max_label, C, 4, 4 * levels]  int32    px[i] = sum_j G[i][j] (levels entries), ps[s] = sum over i + j = s
                                                     (2 * levels - 1 entries and a zero), pd[t] = sum over |i - j| = t (levels)
    sumsq [B, max_label, C, 4]              int64    sum G^2
    clogc [B, max_label, C, 4]              float64  sum over G > 0 of G * log2(G): math.fsum of the float64 terms
    glcm  [B, max_label, C, 4, L, L]        int32    the matrices (None without glcm)

An object without pixels has all-zero rows, as has a direction without pairs.  A negative label, or one above max_label, is
refused whatever `exclude` holds there.  measure() is the vectorised form, measure_slow() walks the pixel pairs in Python ints.
derive() hands the records to the package's host half (cellscreen.texture.texture_table); textbook() evaluates Haralick's double
sums over p = G / N themselves, the rational ones in fractions.Fraction, for the CPU tests to hold that derivation to."""
import math
from fractions import Fraction

import numpy as np

from intensity_reference import _planes
from quantile_reference import contents, disks, noise                  # noqa: F401  (the generators, for the tests and tools)

STEPS = ((0, 1), (1, 1), (1, 0), (1, -1))                               # (row, column) in units of the distance


def check_rule(distance, levels, ranges, channels):
    if not 1 <= int(distance) <= 127:
        raise ValueError(f"distance {distance} is outside the rule")
    if not 2 <= int(levels) <= 64:
        raise ValueError(f"levels {levels} is outside the rule")
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    if len(ranges) != channels:
        raise ValueError(f"{len(ranges)} ranges for {channels} channels")
    for lo, hi in ranges:
        if not 0 <= lo <= hi <= 65535:
            raise ValueError(f"range {lo}..{hi} is outside the rule")
    return int(distance), int(levels), ranges


def full_range(dtype, channels):
    return [(0, int(np.iinfo(dtype).max))] * channels


def quantise(v, lo, hi, levels):
    """the levels of the values v, int64"""
    v = np.clip(np.asarray(v).astype(np.int64), lo, hi) - lo
    return (v * levels) // (hi - lo + 1)


def _shifted(a, dr, dc):
    """(a at p, a at p + (dr, dc)) for every p of the plane a with both inside; dr >= 0"""
    H, W = a.shape
    if dr >= H or abs(dc) >= W:
        return a[:0, :0], a[:0, :0]
    if dc >= 0:
        return a[:H - dr, :W - dc], a[dr:, dc:]
    return a[:H - dr, -dc:], a[dr:, :W + dc]


def records(G):
    """(marg [..., 4 L], sumsq [...], clogc [...]) of matrices G [..., L, L] int64"""
    L = G.shape[-1]
    lead = G.shape[:-2]
    flat = G.reshape((-1, L * L))
    i, j = (x.ravel() for x in np.indices((L, L)))
    marg = np.zeros((flat.shape[0], 4 * L), np.int64)
    marg[:, :L] = G.reshape((-1, L, L)).sum(axis=2)
    for off, width, idx in ((L, 2 * L, i + j), (3 * L, L, np.abs(i - j))):
        part = np.zeros((width, flat.shape[0]), np.int64)
        np.add.at(part, idx, flat.T)
        marg[:, off:off + width] = part.T
    sumsq = (flat * flat).sum(axis=1)
    clogc = np.zeros(flat.shape[0], np.float64)
    for m in np.flatnonzero(flat.any(axis=1)):
        g = flat[m][flat[m] > 0].astype(np.float64)
        clogc[m] = math.fsum((g * np.log2(g)).tolist())
    return marg.reshape(lead + (4 * L,)), sumsq.reshape(lead), clogc.reshape(lead)


def _tables(B, M, C, L, glcm):
    return (np.zeros((B, M), np.int32), np.zeros((B, M, C, 4, 4 * L), np.int32), np.zeros((B, M, C, 4), np.int64),
            np.zeros((B, M, C, 4), np.float64), np.zeros((B, M, C, 4, L, L), np.int32) if glcm else None)


def measure(image, labels, distance, levels, ranges, exclude=None, max_label=None, glcm=False):
    """(count, marg, sumsq, clogc, glcm or None) of image [B,H,W] or [B,H,W,C], labels [B,H,W] and exclude (None or [B,H,W]);
    ranges: a (lo, hi) pair per channel."""
    image, labels, exclude, M = _planes(image, labels, exclude, max_label)
    B, C = labels.shape[0], image.shape[3]
    d, L, ranges = check_rule(distance, levels, ranges, C)
    count, marg, sumsq, clogc, mats = _tables(B, M, C, L, glcm)
    for b in range(B):
        member = np.where(exclude[b] == 0, labels[b], 0).astype(np.int64)     # the object of every pixel, 0: none
        count[b] = np.bincount(member.ravel(), minlength=M + 1)[1:]
        for ch in range(C):
            q = quantise(image[b, :, :, ch], ranges[ch][0], ranges[ch][1], L)
            for k, (sr, sc) in enumerate(STEPS):
                m0, m1 = _shifted(member, sr * d, sc * d)
                q0, q1 = _shifted(q, sr * d, sc * d)
                pair = (m0 > 0) & (m0 == m1)
                G = np.zeros((M, L, L), np.int64)
                np.add.at(G, (m0[pair] - 1, q0[pair], q1[pair]), 1)
                np.add.at(G, (m0[pair] - 1, q1[pair], q0[pair]), 1)
                marg[b, :, ch, k], sumsq[b, :, ch, k], clogc[b, :, ch, k] = records(G)
                if glcm:
                    mats[b, :, ch, k] = G
    return count, marg, sumsq, clogc, mats


def measure_slow(image, labels, distance, levels, ranges, exclude=None, max_label=None, glcm=False):
    """measure(), pixel pair by pixel pair in Python ints."""
    image, labels, exclude, M = _planes(image, labels, exclude, max_label)
    B, H, W = labels.shape
    C = image.shape[3]
    d, L, ranges = check_rule(distance, levels, ranges, C)
    count, marg, sumsq, clogc, mats = _tables(B, M, C, L, glcm)
    for b in range(B):
        lab = [[int(labels[b, r, c]) if int(exclude[b, r, c]) == 0 else 0 for c in range(W)] for r in range(H)]
        for r in range(H):
            for c in range(W):
                if lab[r][c]:
                    count[b, lab[r][c] - 1] += 1
        for ch in range(C):
            lo, hi = ranges[ch]
            q = [[((min(max(int(image[b, r, c, ch]), lo), hi) - lo) * L) // (hi - lo + 1) for c in range(W)] for r in range(H)]
            for k, (sr, sc) in enumerate(STEPS):
                G = [[[0] * L for _ in range(L)] for _ in range(M)]
                for r in range(H):
                    for c in range(W):
                        rr, cc = r + sr * d, c + sc * d
                        if lab[r][c] and 0 <= rr < H and 0 <= cc < W and lab[rr][cc] == lab[r][c]:
                            G[lab[r][c] - 1][q[r][c]][q[rr][cc]] += 1
                            G[lab[r][c] - 1][q[rr][cc]][q[r][c]] += 1
                for m in range(M):
                    g = G[m]
                    for i in range(L):
                        for j in range(L):
                            marg[b, m, ch, k, i] += g[i][j]
                            marg[b, m, ch, k, L + i + j] += g[i][j]
                            marg[b, m, ch, k, 3 * L + abs(i - j)] += g[i][j]
                    sumsq[b, m, ch, k] = sum(x * x for row in g for x in row)
                    clogc[b, m, ch, k] = math.fsum(float(x) * float(np.log2(np.float64(x))) for row in g for x in row if x > 0)
                    if glcm:
                        mats[b, m, ch, k] = g
    return count, marg, sumsq, clogc, mats


def derive(count, marg, sumsq, clogc, levels):
    """The present objects in (image, label) order as a dict of arrays, by the package's host half: image, label, count [n],
    pairs [n,C,4], features [n,C,4,13], mean [n,C,13]."""
    from cellscreen import texture as TX
    t = TX.texture_table(count, marg, sumsq, clogc, levels)
    return dict(image=t.image, label=t.label, count=t.count, pairs=t.pairs, features=t.features, mean=t.mean)


def textbook(G):
    """Haralick's 13 features of one matrix G [L, L] (integers, N = sum G > 0) from the double sums over p = G / N as the paper
    and mahotas write them, py, HXY1 and HXY2 included: the rational ones exactly in Fractions and rounded once, the entropies
    by math.fsum over float64 terms.  Returns 13 floats."""
    L = len(G)
    N = sum(int(x) for row in G for x in row)
    p = [[Fraction(int(G[i][j]), N) for j in range(L)] for i in range(L)]
    px = [sum(p[i]) for i in range(L)]
    py = [sum(p[i][j] for i in range(L)) for j in range(L)]
    ps = [sum(p[i][s - i] for i in range(L) if 0 <= s - i < L) for s in range(2 * L - 1)]
    pd = [sum(p[i][j] for i in range(L) for j in range(L) if abs(i - j) == t) for t in range(L)]
    H = lambda dist: -math.fsum(float(x) * math.log2(float(x)) for x in dist if x > 0)
    mu = sum(i * px[i] for i in range(L))
    var = sum((i - mu) ** 2 * px[i] for i in range(L))
    sij = sum(i * j * p[i][j] for i in range(L) for j in range(L))
    sa = sum(s * ps[s] for s in range(2 * L - 1))
    dm = sum(t * pd[t] for t in range(L))
    hxy = H(x for row in p for x in row)
    hx, hy = H(px), H(py)
    hxy1 = -math.fsum(float(p[i][j]) * math.log2(float(px[i] * py[j])) for i in range(L) for j in range(L) if p[i][j] > 0)
    hxy2 = -math.fsum(float(px[i] * py[j]) * math.log2(float(px[i] * py[j])) for i in range(L) for j in range(L) if px[i] * py[j] > 0)
    f = [sum(x * x for row in p for x in row),
         sum((i - j) ** 2 * p[i][j] for i in range(L) for j in range(L)),
         (sij - mu * mu) / var if var > 0 else Fraction(1),
         sum((i - mu) ** 2 * p[i][j] for i in range(L) for j in range(L)),
         sum(p[i][j] / (1 + (i - j) ** 2) for i in range(L) for j in range(L)),
         sa,
         sum((s - sa) ** 2 * ps[s] for s in range(2 * L - 1)),
         H(ps),
         hxy,
         sum((t - dm) ** 2 * pd[t] for t in range(L)),
         H(pd),
         (hxy - hxy1) / max(hx, hy) if max(hx, hy) > 0 else hxy - hxy1,
         math.sqrt(max(0.0, 1.0 - math.exp(-2.0 * (hxy2 - hxy))))]
    return [float(x) for x in f]
