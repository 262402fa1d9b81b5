"""The rule of cs_label_radial restated in numpy integers and Python ints: no column and row passes, no tiles, no
runs and no tables in between, so that it shares nothing with the kernels.  The rule is this project's; it corresponds to
CellProfiler's MeasureObjectIntensityDistribution and the Edge measures of MeasureObjectIntensity without a promise of bit
equality with CellProfiler.

An object is cs_label_intensity's: the pixels of one image with one label in 1..max_label, connected or not, less the pixels where
`exclude` is non-zero (the effective label of such a pixel is 0).

    E2(p)     the smallest squared Euclidean distance between pixel centres from an object pixel p to a position that is not the
              object's: another label, background, an excluded pixel, any position outside the image.  Exact up to MAX_D2 = 127^2;
              an object with a deeper pixel is refused.
    centre    the deepest pixel of the object, the smallest raster index r W + c among equals; or the caller's.
    C2(p)     the squared Euclidean distance from p to the centre, along the straight line.
    ring(p)   with B bins the number of k in 1..B-1 with (B - k)^2 C2 >= k^2 E2: floor(B dc / (dc + de)) without a root.
    wedge(p)  (r > rc) + 2 (c > cc) + 4 (|r - rc| > |c - cc|)

    geom   [B, max_label, 3]            int64   area, sum r, sum c                                   (cs_label_intensity's)
    center [B, max_label, 4]            int32   row, column, E2 at the deepest pixel (also with given centres), edge pixels
    ring   [B, max_label, bins, 8, 1+C] int64   per (ring, wedge): n, sum v per channel
    edge   [B, max_label, C, 4]         int64   sum v, sum v^2, min v, max v over the pixels with E2 == 1
    d2     [B, H, W]                    uint16  E2, 0 off the objects

measure() finds E2 per object as the minimum of the squared distances to the foreign positions beside the object, in its bounding
window padded by one, by numpy broadcasting (exact integers; no distance transform); measure_slow() walks every object pixel and every
foreign position of the padded image in Python ints and takes the ring from exact Fractions of integer square roots.  derive()
takes the floats from the integers as cellscreen/radial.py does, derive_decimal() in 50 digits."""
import decimal
import math
from fractions import Fraction

import numpy as np

from intensity_reference import _planes, contents, disks, noise        # noqa: F401  (the generators, for the tests and tools)

MAX_D2 = 127 * 127
MAX_BINS = 16


class TooDeep(ValueError):
    """an object holds a pixel with E2 above MAX_D2"""


def effective(labels, exclude):
    return np.where(np.asarray(exclude) != 0, 0, labels).astype(np.int64)


def depth_plane(eff):
    """E2 of one image's effective labels [H,W] as int64, 0 off the objects: per object the minimum over the positions of its
    bounding window padded by one that are not the object's and lie beside it (the pad is outside the image or foreign either
    way, and the nearest foreign position of an object pixel always lies in that window)."""
    H, W = eff.shape
    out = np.zeros((H, W), np.int64)
    for lab in np.unique(eff[eff > 0]):
        rr, cc = np.nonzero(eff == lab)
        r0, r1, c0, c1 = rr.min(), rr.max(), cc.min(), cc.max()
        own = np.zeros((r1 - r0 + 3, c1 - c0 + 3), bool)                  # the bounding box padded by one position all round
        own[rr - r0 + 1, cc - c0 + 1] = True
        # Only a foreign position with a 4-neighbour in the object can be the nearest of a pixel p: from any other one a step
        # towards p along an axis lands on a foreign position that is nearer.
        beside = np.zeros_like(own)
        beside[1:] |= own[:-1]
        beside[:-1] |= own[1:]
        beside[:, 1:] |= own[:, :-1]
        beside[:, :-1] |= own[:, 1:]
        fr, fc = np.nonzero(beside & ~own)
        pr, pc = rr - r0 + 1, cc - c0 + 1
        best = np.empty(pr.shape, np.int64)
        step = max(1, (1 << 22) // fr.size)                               # object pixels in slabs, to bound the memory
        for lo in range(0, pr.size, step):
            d = (pr[lo:lo + step, None] - fr[None, :]) ** 2 + (pc[lo:lo + step, None] - fc[None, :]) ** 2
            best[lo:lo + step] = d.min(axis=1)
        out[rr, cc] = best
    return out


def ring_of(bins, c2, e2):
    """the ring by the integer rule; c2, e2: int64 arrays"""
    ring = np.zeros(np.shape(c2), np.int64)
    for k in range(1, bins):
        ring += ((bins - k) ** 2 * c2 >= k * k * e2).astype(np.int64)
    return ring


def wedge_of(dr, dc):
    return (dr > 0).astype(np.int64) + 2 * (dc > 0) + 4 * (np.abs(dr) > np.abs(dc))


def _check_rule(bins, centers, B, H, W, max_label):
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError("bins: 1..16")
    if centers is not None:
        centers = np.asarray(centers)
        if centers.shape != (B, max_label, 2):
            raise ValueError("centers: [B,max_label,2]")
        if centers.min() < 0 or centers[..., 0].max() >= H or centers[..., 1].max() >= W:
            raise ValueError("centers: outside the image")
    return int(bins), centers


def measure(image, labels, exclude=None, max_label=None, bins=4, centers=None):
    """(geom, center, ring, edge, d2) of image [B,H,W] or [B,H,W,C], labels [B,H,W], exclude (None or [B,H,W]) and centers (None
    or [B,max_label,2])."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    B, H, W = labels.shape
    C = image.shape[3]
    bins, centers = _check_rule(bins, centers, B, H, W, max_label)
    geom = np.zeros((B, max_label, 3), np.int64)
    center = np.zeros((B, max_label, 4), np.int32)
    ring = np.zeros((B, max_label, bins, 8, 1 + C), np.int64)
    edge = np.zeros((B, max_label, C, 4), np.int64)
    d2 = np.zeros((B, H, W), np.uint16)
    for b in range(B):
        eff = effective(labels[b], exclude[b])
        e2 = depth_plane(eff)
        if e2.max(initial=0) > MAX_D2:
            raise TooDeep(f"an object is deeper than E2 = {MAX_D2}")
        d2[b] = e2
        for lab in np.unique(eff[eff > 0]):
            rr, cc = np.nonzero(eff == lab)                               # raster order
            m = lab - 1
            d = e2[rr, cc]
            top = int(np.argmax(d))                                       # the first of the maxima: the smallest raster index
            rc, ccn = (int(rr[top]), int(cc[top])) if centers is None else (int(centers[b, m, 0]), int(centers[b, m, 1]))
            on_edge = d == 1
            geom[b, m] = rr.size, rr.sum(), cc.sum()
            center[b, m] = rc, ccn, d[top], on_edge.sum()
            dr, dc = rr - rc, cc - ccn
            rg, wd = ring_of(bins, dr * dr + dc * dc, d), wedge_of(dr, dc)
            np.add.at(ring[b, m, :, :, 0], (rg, wd), 1)
            for ch in range(C):
                v = image[b][rr, cc, ch].astype(np.int64)
                np.add.at(ring[b, m, :, :, 1 + ch], (rg, wd), v)
                ve = v[on_edge]
                edge[b, m, ch] = ve.sum(), (ve * ve).sum(), ve.min(), ve.max()
    return geom, center, ring, edge, d2


def measure_slow(image, labels, exclude=None, max_label=None, bins=4, centers=None):
    """measure(), position by position in Python ints; the ring from floor(B dc / (dc + de)) decided in exact arithmetic: with
    x = B dc / (dc + de), x >= k iff (B - k) dc >= k de iff (B - k)^2 C2 >= k^2 E2 (both sides non-negative) -- taken here
    through Fractions of the squares, so that the integer rule of measure() is not repeated literally."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    B, H, W = labels.shape
    C = image.shape[3]
    bins, centers = _check_rule(bins, centers, B, H, W, max_label)
    geom = np.zeros((B, max_label, 3), np.int64)
    center = np.zeros((B, max_label, 4), np.int32)
    ring = np.zeros((B, max_label, bins, 8, 1 + C), np.int64)
    edge = np.zeros((B, max_label, C, 4), np.int64)
    d2 = np.zeros((B, H, W), np.uint16)
    for b in range(B):
        eff = [[0 if int(exclude[b, r, c]) != 0 else int(labels[b, r, c]) for c in range(W)] for r in range(H)]
        depth = {}
        for r in range(H):
            for c in range(W):
                lab = eff[r][c]
                if lab == 0:
                    continue
                best = None
                for fr in range(-1, H + 1):                               # one position beyond the image all round is enough:
                    for fc in range(-1, W + 1):                           # a farther one outside is never the nearest
                        inside = 0 <= fr < H and 0 <= fc < W
                        if inside and eff[fr][fc] == lab:
                            continue
                        d = (fr - r) ** 2 + (fc - c) ** 2
                        best = d if best is None or d < best else best
                depth[(r, c)] = best
                d2[b, r, c] = best
        for lab in sorted({x for row in eff for x in row if x > 0}):
            m = lab - 1
            px = [(r, c) for r in range(H) for c in range(W) if eff[r][c] == lab]
            deepest = max(depth[p] for p in px)
            first = min(p[0] * W + p[1] for p in px if depth[p] == deepest)
            rc, cc = divmod(first, W) if centers is None else (int(centers[b, m, 0]), int(centers[b, m, 1]))
            n_edge = 0
            for r, c in px:
                e2, c2 = depth[(r, c)], (r - rc) ** 2 + (c - cc) ** 2
                if c2 == 0:
                    rg = 0
                else:
                    q = Fraction(e2, c2)                                   # (de / dc)^2; x >= k iff (B - k) / k >= de / dc
                    rg = sum(1 for k in range(1, bins) if Fraction(bins - k, k) ** 2 >= q)
                wd = (r > rc) + 2 * (c > cc) + 4 * (abs(r - rc) > abs(c - cc))
                geom[b, m] += (1, r, c)
                ring[b, m, rg, wd, 0] += 1
                for ch in range(C):
                    v = int(image[b, r, c, ch])
                    ring[b, m, rg, wd, 1 + ch] += v
                    if e2 == 1:
                        first_edge = n_edge == 0
                        edge[b, m, ch, 0] += v
                        edge[b, m, ch, 1] += v * v
                        edge[b, m, ch, 2] = v if first_edge else min(int(edge[b, m, ch, 2]), v)
                        edge[b, m, ch, 3] = v if first_edge else max(int(edge[b, m, ch, 3]), v)
                n_edge += e2 == 1
            center[b, m] = rc, cc, deepest, n_edge
    return geom, center, ring, edge, d2


def ring_float(bins, c2, e2):
    """the float form of the ring: floor(B dc / (dc + de)), as CellProfiler's normalized distance times the bin count"""
    dc, de = np.sqrt(np.asarray(c2, np.float64)), np.sqrt(np.asarray(e2, np.float64))
    return np.minimum(np.floor(bins * (dc / (dc + de))), bins - 1).astype(np.int64)


def geodesic_c2(own, rc, cc):
    """For the comparison with CellProfiler's propagated distance: the length of the shortest 8-connected path inside `own` from
    the centre, steps of 1 and sqrt(2), by Dijkstra -- float64 [H,W], inf where unreachable.  Not part of the rule."""
    import heapq
    H, W = own.shape
    dist = np.full((H, W), np.inf)
    dist[rc, cc] = 0.0
    heap = [(0.0, rc, cc)]
    while heap:
        d, r, c = heapq.heappop(heap)
        if d > dist[r, c]:
            continue
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                rr, c2 = r + dr, c + dc
                if (dr or dc) and 0 <= rr < H and 0 <= c2 < W and own[rr, c2]:
                    nd = d + (math.sqrt(2.0) if dr and dc else 1.0)
                    if nd < dist[rr, c2]:
                        dist[rr, c2] = nd
                        heapq.heappush(heap, (nd, rr, c2))
    return dist


def _cv2(nw, sw):
    means = [Fraction(s, k) for k, s in zip(nw, sw) if k > 0]
    if not means:
        return None
    m = sum(means) / len(means)
    if m == 0:
        return None
    return (sum(x * x for x in means) / len(means) - m * m) / (m * m)


def _objects(geom):
    return [(b, m) for b in range(geom.shape[0]) for m in range(geom.shape[1]) if geom[b, m, 0] > 0]


def derive_exact(geom, center, ring, edge):
    """Per present object, in (image, label) order, the exact values as Fractions or None: frac_at_d, mean_frac, radial_cv2 (the
    square of radial_cv) [R][C]; edge_mean, edge_var (the square of edge_std) [C]."""
    out = []
    nb, C = ring.shape[2], edge.shape[2]
    for b, m in _objects(geom):
        area, ne = int(geom[b, m, 0]), int(center[b, m, 3])
        o = dict(frac_at_d=[], mean_frac=[], radial_cv2=[], edge_mean=[], edge_var=[])
        for r in range(nb):
            fr, mf, cv = [], [], []
            for ch in range(C):
                total = int(ring[b, m, :, :, 1 + ch].sum())
                nw = [int(x) for x in ring[b, m, r, :, 0]]
                sw = [int(x) for x in ring[b, m, r, :, 1 + ch]]
                fr.append(Fraction(sum(sw), total) if total else None)
                mf.append(Fraction(sum(sw) * area, total * sum(nw)) if total and sum(nw) else None)
                cv.append(_cv2(nw, sw))
            o["frac_at_d"].append(fr)
            o["mean_frac"].append(mf)
            o["radial_cv2"].append(cv)
        for ch in range(C):
            sv, sv2 = int(edge[b, m, ch, 0]), int(edge[b, m, ch, 1])
            o["edge_mean"].append(Fraction(sv, ne) if ne else None)
            o["edge_var"].append(Fraction(ne * sv2 - sv * sv, ne * ne) if ne else None)
        out.append(o)
    return out


def derive(geom, center, ring, edge):
    """The present objects in (image, label) order as a dict of arrays, as cellscreen.radial.radial_table derives them: a
    quotient is one correctly rounded division of Python ints, a root the root of one such quotient."""
    keys = _objects(geom)
    n, nb, C = len(keys), ring.shape[2], edge.shape[2]
    ex = derive_exact(geom, center, ring, edge)
    fl = lambda f: math.nan if f is None else f.numerator / f.denominator
    rt = lambda f: math.nan if f is None else math.sqrt(f.numerator / f.denominator)
    out = dict(image=np.array([b for b, _ in keys], np.int32).reshape(n), label=np.array([m + 1 for _, m in keys], np.int32).reshape(n),
               area=np.array([geom[k][0] for k in keys], np.int64).reshape(n),
               center_rc=np.array([center[k][:2] for k in keys], np.int32).reshape(n, 2),
               max_d2=np.array([center[k][2] for k in keys], np.int32).reshape(n),
               edge_count=np.array([center[k][3] for k in keys], np.int64).reshape(n),
               frac_at_d=np.array([[[fl(x) for x in row] for row in o["frac_at_d"]] for o in ex], np.float64).reshape(n, nb, C),
               mean_frac=np.array([[[fl(x) for x in row] for row in o["mean_frac"]] for o in ex], np.float64).reshape(n, nb, C),
               radial_cv=np.array([[[rt(x) for x in row] for row in o["radial_cv2"]] for o in ex], np.float64).reshape(n, nb, C),
               edge_integrated=np.array([edge[k][:, 0] for k in keys], np.int64).reshape(n, C),
               edge_mean=np.array([[fl(x) for x in o["edge_mean"]] for o in ex], np.float64).reshape(n, C),
               edge_std=np.array([[rt(x) for x in o["edge_var"]] for o in ex], np.float64).reshape(n, C),
               edge_min=np.array([edge[k][:, 2] for k in keys], np.int64).reshape(n, C),
               edge_max=np.array([edge[k][:, 3] for k in keys], np.int64).reshape(n, C))
    return out


def to_decimal(f, root=False):
    """a Fraction (or None) in 50 digits; root: its square root"""
    if f is None:
        return None
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        d = decimal.Decimal(f.numerator) / decimal.Decimal(f.denominator)
        return d.sqrt() if root else d


def u_shape(side=21, gap=7, arm=5):
    """One U-shaped object in a [side + 2, 2 arm + gap + 2] image: two arms joined at the bottom."""
    lab = np.zeros((side + 2, 2 * arm + gap + 2), np.int32)
    lab[1:side + 1, 1:2 * arm + gap + 1] = 1
    lab[1:side + 1 - arm, 1 + arm:1 + arm + gap] = 0
    return lab
