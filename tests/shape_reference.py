"""The rule of cs_label_shape restated in numpy integers: no tiles, no strips and no bitmaps, so that it shares nothing
with the kernels.

An object is cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  Let e be the effective plane: the label, or 0 where excluded or outside the image.  Everything is a function of e
alone.  The dense records, row label - 1 for label L:

    moments [B, max_label, 10] int64   n and the sums of r, c, r^2, rc, c^2, r^3, r^2 c, r c^2, c^3 over the pixels (r, c) of L
    box     [B, max_label, 4]  int32   minr, minc, maxr, maxc, the max exclusive
    quads   [B, max_label, 16] int32   the histogram of [e(r,c)==L] + 2 [e(r+1,c)==L] + 4 [e(r,c+1)==L] + 8 [e(r+1,c+1)==L] over
                                       r = -1 .. H-1, c = -1 .. W-1; bin 0 is left zero
    perim   [B, max_label, 3]  int32   the classes of skimage.measure.perimeter(mask, neighbourhood=4): a border pixel is a pixel
                                       of L with a 4-neighbour where e != L; with a and d its 4-neighbours and diagonal neighbours
                                       that are border pixels of L, 1 + 2a + 10d in {5, 7, 15, 17, 25, 27} counts in class 0
                                       (weight 1), in {21, 33} in class 1 (sqrt 2), in {13, 23} in class 2 ((1 + sqrt 2) / 2)
    hull    [B, max_label, 4]  int64   convex_area, feret_max2, feret_min_num, feret_min_den (None without hull)

The hull is that of the points (2r +- 1, 2c) and (2r, 2c +- 1) of the object's pixels, doubled coordinates.  convex_area counts the
pixels whose centre (2r, 2c) lies inside or on it.  feret_max2 is the largest squared distance between two of its vertices.  Every
edge (a, b) has the width w = max over the vertices v of |cross(b - a, v - a)|; the edge with the smallest w^2 / |b - a|^2, among
equal quotients the one with the smaller |b - a|^2, gives feret_min_num = w and feret_min_den = |b - a|^2.

An object without pixels has all-zero rows.  A negative label, or one above max_label, is refused whatever `exclude` holds there.
measure() is the vectorised form; measure_slow() walks the pixels in Python ints, takes the hull from scipy.spatial.ConvexHull and
compares widths as fractions.Fraction.  derive() hands the records to the package's host half (cellscreen.shape.shape_table);
derive_slow() takes the same values from exact rationals rounded once, for the CPU tests to hold that derivation to."""
import math
from fractions import Fraction

import numpy as np

from texture_reference import contents, disks          # noqa: F401  (the generators, for the tests and tools)

CLASS_OF = {5: 0, 7: 0, 15: 0, 17: 0, 25: 0, 27: 0, 21: 1, 33: 1, 13: 2, 23: 2}
MIDPOINTS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def _planes(labels, exclude, max_label):
    labels = np.asarray(labels)
    if labels.ndim != 3:
        raise ValueError(f"labels {labels.shape}: [B,H,W] expected")
    if exclude is None:
        exclude = np.zeros(labels.shape, np.int32)
    exclude = np.asarray(exclude)
    if exclude.shape != labels.shape:
        raise ValueError("exclude and labels differ in shape")
    if max_label is None:
        max_label = max(1, int(labels.max()))
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) > max_label):
        raise ValueError("a label is negative or exceeds max_label")
    return labels, exclude, int(max_label)


def _tables(B, M, hull):
    return (np.zeros((B, M, 10), np.int64), np.zeros((B, M, 4), np.int32), np.zeros((B, M, 16), np.int32), np.zeros((B, M, 3), np.int32),
            np.zeros((B, M, 4), np.int64) if hull else None)


# ---- the hull of a set of doubled points, in Python ints ------------------------------------------------------------------------
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_vertices(points):
    """the strictly convex hull of integer points [(y, x)], counter-clockwise in (y, x), no collinear vertex: Andrew's chain"""
    pts = sorted(set((int(y), int(x)) for y, x in points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def feret_records(v):
    """(feret_max2, feret_min_num, feret_min_den) of hull vertices v in order, numpy int64 throughout: the products stay below 2^56
    but the comparison of two quotients, which is made in Python ints"""
    v = np.asarray(v, np.int64)
    d = v[:, None, :] - v[None, :, :]
    max2 = int((d * d).sum(axis=2).max())
    a, b = v, np.roll(v, -1, axis=0)
    e = b - a
    den = (e * e).sum(axis=1)
    rel = v[None, :, :] - a[:, None, :]                 # [edge, vertex, 2]
    w = np.abs(e[:, None, 0] * rel[:, :, 1] - e[:, None, 1] * rel[:, :, 0]).max(axis=1)
    best = None
    for wk, dk in zip(w.tolist(), den.tolist()):
        if dk == 0:
            continue
        if best is None or wk * wk * best[1] < best[0] * best[0] * dk or (wk * wk * best[1] == best[0] * best[0] * dk and dk < best[1]):
            best = (wk, dk)
    return max2, best[0], best[1]


def hull_records(rr, cc):
    """hull row of the pixels (rr, cc) of one object"""
    rr, cc = np.asarray(rr, np.int64), np.asarray(cc, np.int64)
    pts = set()
    for r in np.unique(rr):                             # the row extremes carry the hull: every other midpoint lies between them
        sel = cc[rr == r]
        for c in (int(sel.min()), int(sel.max())):
            pts.update((2 * int(r) + dy, 2 * c + dx) for dy, dx in MIDPOINTS)
    v = np.array(hull_vertices(pts), np.int64)
    r0, r1, c0, c1 = int(rr.min()), int(rr.max()), int(cc.min()), int(cc.max())
    gr, gc = np.mgrid[r0:r1 + 1, c0:c1 + 1]
    py, px = 2 * gr.ravel().astype(np.int64), 2 * gc.ravel().astype(np.int64)
    inside = np.ones(py.shape, bool)
    for k in range(len(v)):
        a, b = v[k], v[(k + 1) % len(v)]
        inside &= (b[0] - a[0]) * (px - a[1]) - (b[1] - a[1]) * (py - a[0]) >= 0
    return (int(inside.sum()),) + feret_records(v)


# ---- closed forms of the h x w rectangle at (r0, c0) ----------------------------------------------------------------------------
def _power_sums(a, k):
    """sum of r, r^2, r^3 over r = a .. a + k - 1, Python ints"""
    p = lambda n: (n * (n - 1) // 2, (n - 1) * n * (2 * n - 1) // 6, (n * (n - 1) // 2) ** 2)
    return tuple(x - y for x, y in zip(p(a + k), p(a)))


def rectangle_records(r0, c0, h, w):
    """(moments, box, quads, perim, hull) rows of one full h x w rectangle, in closed form; perim for h, w >= 3 or a single pixel"""
    R1, R2, R3 = _power_sums(r0, h)
    C1, C2, C3 = _power_sums(c0, w)
    moments = [h * w, w * R1, h * C1, w * R2, R1 * C1, h * C2, w * R3, R2 * C1, R1 * C2, h * C3]
    quads = [0] * 16
    for code, n in ((8, 1), (2, 1), (4, 1), (1, 1), (10, w - 1), (5, w - 1), (12, h - 1), (3, h - 1), (15, (h - 1) * (w - 1))):
        quads[code] += n
    if h >= 3 and w >= 3:
        perim = [2 * (h + w) - 4, 0, 0]
    elif h == 1 and w == 1:
        perim = [0, 0, 0]
    else:
        raise ValueError("no closed form of the perimeter classes for this rectangle here")
    # the hull in the rectangle's own doubled coordinates: an octagon, its corners cut between the midpoints of the corner pixels
    y1, x1 = 2 * h - 1, 2 * w - 1
    octagon = hull_vertices([(-1, 0), (-1, x1 - 1), (0, x1), (y1 - 1, x1), (y1, x1 - 1), (y1, 0), (y1 - 1, -1), (0, -1)])
    return moments, [r0, c0, r0 + h, c0 + w], quads, perim, [h * w] + list(feret_records(octagon))


# ---- the vectorised form ------------------------------------------------------------------------------------------------------
def measure(labels, exclude=None, max_label=None, hull=True):
    """(moments, box, quads, perim, hull or None) of labels [B,H,W] and exclude (None or [B,H,W])."""
    labels, exclude, M = _planes(labels, exclude, max_label)
    B, H, W = labels.shape
    moments, box, quads, perim, hl = _tables(B, M, hull)
    for b in range(B):
        e = np.where(exclude[b] == 0, labels[b], 0).astype(np.int64)
        rr, cc = np.nonzero(e)
        if rr.size == 0:
            continue
        lab = e[rr, cc]
        order = np.argsort(lab, kind="stable")
        lab, rr, cc = lab[order], rr[order].astype(np.int64), cc[order].astype(np.int64)
        starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
        rows = lab[starts] - 1
        for k, x in enumerate((np.ones_like(lab), rr, cc, rr * rr, rr * cc, cc * cc, rr ** 3, rr * rr * cc, rr * cc * cc, cc ** 3)):
            moments[b, rows, k] = np.add.reduceat(x, starts)
        box[b, rows, 0], box[b, rows, 1] = np.minimum.reduceat(rr, starts), np.minimum.reduceat(cc, starts)
        box[b, rows, 2], box[b, rows, 3] = np.maximum.reduceat(rr, starts) + 1, np.maximum.reduceat(cc, starts) + 1
        P = np.pad(e, 1)
        # the quads: every corner and every label at one of its four places once, under the first place that holds the label
        v = (P[:-1, :-1], P[1:, :-1], P[:-1, 1:], P[1:, 1:])
        for k in range(4):
            first = v[k] > 0
            for j in range(k):
                first &= v[j] != v[k]
            code = sum((v[j] == v[k]).astype(np.int64) << j for j in range(4))
            np.add.at(quads[b], (v[k][first] - 1, code[first]), 1)
        # the perimeter classes: the border pixels of all objects at once, each object background to the others
        c = P[1:-1, 1:-1]
        border = (c > 0) & ((P[:-2, 1:-1] != c) | (P[2:, 1:-1] != c) | (P[1:-1, :-2] != c) | (P[1:-1, 2:] != c))
        Bd = np.pad(np.where(border, c, 0), 1)
        m = Bd[1:-1, 1:-1]
        a = sum((x == m).astype(np.int64) for x in (Bd[:-2, 1:-1], Bd[2:, 1:-1], Bd[1:-1, :-2], Bd[1:-1, 2:]))
        d = sum((x == m).astype(np.int64) for x in (Bd[:-2, :-2], Bd[:-2, 2:], Bd[2:, :-2], Bd[2:, 2:]))
        value = 1 + 2 * a + 10 * d
        for cls, vals in enumerate(((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))):
            sel = border & np.isin(value, vals)
            np.add.at(perim[b, :, cls], m[sel] - 1, 1)
        if hull:
            ends = np.r_[starts[1:], lab.size]
            for row, s, t in zip(rows, starts, ends):
                hl[b, row] = hull_records(rr[s:t], cc[s:t])
    return moments, box, quads, perim, hl


# ---- the slow form ------------------------------------------------------------------------------------------------------------
def hull_records_slow(px):
    """hull row of the pixels [(r, c)] of one object: scipy's hull of all their midpoints, its collinear vertices dropped by an
    exact test, the inside test and the widths in Python ints and Fractions"""
    from scipy.spatial import ConvexHull
    pts = sorted({(2 * r + dy, 2 * c + dx) for r, c in px for dy, dx in MIDPOINTS})
    hv = [pts[i] for i in ConvexHull(np.array(pts, np.float64)).vertices]
    v = [p for k, p in enumerate(hv) if _cross(hv[k - 1], p, hv[(k + 1) % len(hv)]) != 0]
    if _cross(v[0], v[1], v[2]) < 0:
        v.reverse()
    n = len(v)
    r0, r1 = min(r for r, _ in px), max(r for r, _ in px)
    c0, c1 = min(c for _, c in px), max(c for _, c in px)
    convex = sum(1 for r in range(r0, r1 + 1) for c in range(c0, c1 + 1)
                 if all(_cross(v[k], v[(k + 1) % n], (2 * r, 2 * c)) >= 0 for k in range(n)))
    max2 = max((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for p in v for q in v)
    best = None
    for k in range(n):
        a, b = v[k], v[(k + 1) % n]
        den = (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
        w = max(abs(_cross(a, b, p)) for p in v)
        key = (Fraction(w * w, den), den)
        if best is None or key < best[0]:
            best = (key, w, den)
    return convex, max2, best[1], best[2]


def measure_slow(labels, exclude=None, max_label=None, hull=True):
    """measure(), pixel by pixel in Python ints."""
    labels, exclude, M = _planes(labels, exclude, max_label)
    B, H, W = labels.shape
    moments, box, quads, perim, hl = _tables(B, M, hull)
    for b in range(B):
        e = [[int(labels[b, r, c]) if int(exclude[b, r, c]) == 0 else 0 for c in range(W)] for r in range(H)]
        at = lambda r, c: e[r][c] if 0 <= r < H and 0 <= c < W else 0
        members = {}
        for r in range(H):
            for c in range(W):
                if e[r][c]:
                    members.setdefault(e[r][c], []).append((r, c))
        for L, px in members.items():
            mom = [0] * 10
            for r, c in px:
                for k, x in enumerate((1, r, c, r * r, r * c, c * c, r ** 3, r * r * c, r * c * c, c ** 3)):
                    mom[k] += x
            moments[b, L - 1] = mom
            box[b, L - 1] = (min(r for r, _ in px), min(c for _, c in px), max(r for r, _ in px) + 1, max(c for _, c in px) + 1)
            is_border = lambda r, c: at(r, c) == L and any(at(r + dr, c + dc) != L for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            for r, c in px:
                if not is_border(r, c):
                    continue
                a = sum(is_border(r + dr, c + dc) for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)))
                d = sum(is_border(r + dr, c + dc) for dr, dc in ((-1, -1), (-1, 1), (1, -1), (1, 1)))
                cls = CLASS_OF.get(1 + 2 * a + 10 * d)
                if cls is not None:
                    perim[b, L - 1, cls] += 1
            if hull:
                hl[b, L - 1] = hull_records_slow(px)
        for r in range(-1, H):
            for c in range(-1, W):
                four = (at(r, c), at(r + 1, c), at(r, c + 1), at(r + 1, c + 1))
                for L in set(four) - {0}:
                    quads[b, L - 1, sum(1 << j for j in range(4) if four[j] == L)] += 1
    return moments, box, quads, perim, hl


# ---- what a table reports -------------------------------------------------------------------------------------------------------
FLOAT_FIELDS = ("extent", "centroid", "equivalent_diameter", "mu", "inertia_tensor", "inertia_eigvals", "major_axis_length",
                "minor_axis_length", "eccentricity", "orientation", "hu", "perimeter", "form_factor")
HULL_FIELDS = ("solidity", "feret_diameter_max", "feret_diameter_min")
INT_FIELDS = ("image", "label", "area", "bbox", "bbox_area", "euler_number", "euler_number_4")


def derive(moments, box, quads, perim, hull=None):
    """The present objects in (image, label) order as a dict of arrays, by the package's host half."""
    from cellscreen import shape as SH
    t = SH.shape_table(moments, box, quads, perim, hull)
    names = INT_FIELDS + FLOAT_FIELDS + (("convex_area",) + HULL_FIELDS if hull is not None else ())
    return {k: getattr(t, k) for k in names}


def derive_slow(moments, box, quads, perim, hull=None):
    """derive() from exact rationals: every rational value is a Fraction rounded once, every irrational one is taken by one libm
    call from such a value."""
    B, M = moments.shape[:2]
    keys = [(b, m) for b in range(B) for m in range(M) if moments[b, m, 0] > 0]
    out = {k: [] for k in INT_FIELDS + FLOAT_FIELDS + (("convex_area",) + HULL_FIELDS if hull is not None else ())}
    for b, m in keys:
        n, sr, sc, srr, src, scc, srrr, srrc, srcc, sccc = (int(x) for x in moments[b, m])
        rb, cb = Fraction(sr, n), Fraction(sc, n)
        minr, minc, maxr, maxc = (int(x) for x in box[b, m])
        mu20, mu11, mu02 = srr - rb * sr, src - rb * sc, scc - cb * sc
        mu30 = srrr - 3 * rb * srr + 2 * rb * rb * sr
        mu03 = sccc - 3 * cb * scc + 2 * cb * cb * sc
        mu21 = srrc - 2 * rb * src - cb * srr + 2 * rb * rb * sc
        mu12 = srcc - 2 * cb * src - rb * scc + 2 * cb * cb * sr
        trr, trc, tcc = mu20 / n, mu11 / n, mu02 / n
        rad = math.sqrt(float(((tcc - trr) / 2) ** 2 + trc * trc))
        l1, l2 = float((tcc + trr) / 2) + rad, max(float((tcc + trr) / 2) - rad, 0.0)
        q = [int(x) for x in quads[b, m]]
        q1, q3, qd = q[1] + q[2] + q[4] + q[8], q[7] + q[11] + q[13] + q[14], q[6] + q[9]
        p = float(perim[b, m, 0]) + float(perim[b, m, 1]) * math.sqrt(2.0) + float(perim[b, m, 2]) * ((1.0 + math.sqrt(2.0)) / 2.0)
        # Hu's invariants of eta_pq = mu_pq / n^(1 + (p + q) / 2): the square root of n leaves every one of them
        e20, e11, e02 = mu20 / n ** 2, mu11 / n ** 2, mu02 / n ** 2
        s, t, u, v = mu30 + mu12, mu21 + mu03, mu30 - 3 * mu12, 3 * mu21 - mu03      # times n^2.5
        hu = [e20 + e02, (e20 - e02) ** 2 + 4 * e11 * e11, (u * u + v * v) / n ** 5, (s * s + t * t) / n ** 5,
              (u * s * (s * s - 3 * t * t) + v * t * (3 * s * s - t * t)) / n ** 10,
              ((e20 - e02) * (s * s - t * t) + 4 * e11 * s * t) / n ** 5,
              (v * s * (s * s - 3 * t * t) - u * t * (3 * s * s - t * t)) / n ** 10]
        row = dict(image=b, label=m + 1, area=n, bbox=[minr, minc, maxr, maxc], bbox_area=(maxr - minr) * (maxc - minc),
                   euler_number=Fraction(q1 - q3 - 2 * qd, 4), euler_number_4=Fraction(q1 - q3 + 2 * qd, 4),
                   extent=float(Fraction(n, (maxr - minr) * (maxc - minc))), centroid=[float(rb), float(cb)],
                   equivalent_diameter=math.sqrt(4.0 * n / math.pi), mu=[float(x) for x in (mu20, mu11, mu02, mu30, mu21, mu12, mu03)],
                   inertia_tensor=[[float(tcc), float(-trc)], [float(-trc), float(trr)]], inertia_eigvals=[l1, l2],
                   major_axis_length=4.0 * math.sqrt(l1), minor_axis_length=4.0 * math.sqrt(l2),
                   eccentricity=0.0 if l1 == 0.0 else 1.0 if l2 <= 0.0 else math.sqrt(2.0 * rad / l1),
                   orientation=0.5 * math.atan2(float(2 * mu11 * n), float((mu20 - mu02) * n)), hu=[float(x) for x in hu], perimeter=p,
                   form_factor=4.0 * math.pi * n / (p * p) if p > 0 else math.nan)
        assert row["euler_number"].denominator == 1 and row["euler_number_4"].denominator == 1
        row["euler_number"], row["euler_number_4"] = int(row["euler_number"]), int(row["euler_number_4"])
        if hull is not None:
            cv, f2, w, den = (int(x) for x in hull[b, m])
            row.update(convex_area=cv, solidity=float(Fraction(n, cv)), feret_diameter_max=math.sqrt(float(Fraction(f2, 4))),
                       feret_diameter_min=math.sqrt(float(Fraction(w * w, 4 * den))))
        for k, x in row.items():
            out[k].append(x)
    n = len(keys)
    dt = dict(image=np.int32, label=np.int32, area=np.int64, bbox=np.int32, bbox_area=np.int64, euler_number=np.int64, euler_number_4=np.int64,
              convex_area=np.int64)
    tail = dict(bbox=(4,), centroid=(2,), mu=(7,), inertia_tensor=(2, 2), inertia_eigvals=(2,), hu=(7,))
    return {k: np.array(x, dt.get(k, np.float64)).reshape((n,) + tail.get(k, ())) for k, x in out.items()}
