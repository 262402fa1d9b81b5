"""CPU restatement of the quality-cell extraction (improved_detection.py:61-111) with numpy and scipy.spatial.ConvexHull,
for the tests only: the library never imports it.

scikit-image 0.18.3's regionprops pieces, restated:
* bbox, area: min/max of the region's pixel coordinates (max exclusive), pixel count.
* eccentricity: the inertia tensor of the central moments, [[mu02, -mu11], [-mu11, mu20]] / mu00 (_moments.inertia_tensor),
  its eigenvalues l1 >= l2 clipped at 0, sqrt(1 - l2/l1), 0 when l1 == 0.  The moments are exact integers here (n * S2 - S1^2,
  one rounding to float64, one division by n^2), the eigenvalues are the closed form of the symmetric 2x2 matrix, and
  1 - l2/l1 is evaluated as 2 rad / l1, its cancellation-free form.  Every float operation is spelled out so that the
  device's explicitly rounded arithmetic (csrc/extract.hip) reproduces it to the bit.
* solidity: area / convex_area, convex_area = the bbox pixel centres inside or on the convex hull of the pixel-edge
  midpoints of the row and column extremes (convex_hull_image: possible_hull + offset_coordinates + grid_points_in_poly),
  counted with an exact integer test on doubled coordinates.
* mean / std of green_channel[minr:maxr, minc:maxc]: the exact integer sums, Sx / N and sqrt((N Sxx - Sx^2) / N^2).
"""
import math

import numpy as np
from scipy.spatial import ConvexHull

QC_BORDER, QC_AREA, QC_ECCENTRICITY, QC_INTENSITY = 1, 2, 4, 8
IMAGE_OK, IMAGE_NO_CELLS, IMAGE_UNSUPPORTED = 0, 1, 2
REFERENCE_QC = dict(border=10, min_area=200, max_area=8000, max_eccentricity=0.95, min_mean=0.5, min_std=0.1)


def convex_area(mask: np.ndarray) -> int:
    """convex_hull_image(mask, offset_coordinates=True).sum() with 'inside or on the hull' counted exactly."""
    rr, cc = np.nonzero(mask)
    pts = set()
    for axis_vals, other in ((rr, cc), (cc, rr)):                 # extremes of every row, then of every column
        for v in np.unique(axis_vals):
            sel = other[axis_vals == v]
            for o in (sel.min(), sel.max()):
                pts.add((int(v), int(o)) if axis_vals is rr else (int(o), int(v)))
    coords = np.array(sorted(pts), np.int64)
    # doubled coordinates of the pixel-edge midpoints (r +- 1/2, c), (r, c +- 1/2)
    off = np.array([[-1, 0], [1, 0], [0, -1], [0, 1]], np.int64)
    dbl = np.unique((2 * coords[:, None, :] + off[None]).reshape(-1, 2), axis=0)
    hull = ConvexHull(dbl.astype(np.float64))
    v = dbl[hull.vertices]                                        # counter-clockwise in (x=row, y=col) for 2-D hulls
    h, w = mask.shape
    gr, gc = np.mgrid[0:h, 0:w]
    P = np.stack([2 * gr.ravel(), 2 * gc.ravel()], 1).astype(np.int64)
    inside = np.ones(len(P), bool)
    for k in range(len(v)):
        a, b = v[k], v[(k + 1) % len(v)]
        cross = (b[0] - a[0]) * (P[:, 1] - a[1]) - (b[1] - a[1]) * (P[:, 0] - a[0])
        inside &= cross >= 0
    return int(inside.sum())


def eccentricity(rr: np.ndarray, cc: np.ndarray) -> float:
    i = [int(x) for x in rr]
    j = [int(x) for x in cc]
    return eccentricity_from_sums(len(i), sum(i), sum(j), sum(x * x for x in i), sum(x * x for x in j),
                                  sum(x * y for x, y in zip(i, j)))


def inertia_eigenvalues(n: int, si: int, sj: int, sii: int, sjj: int, sij: int):
    """(rad, l1, l2) of the inertia tensor from the region's exact moment sums (Python ints): pixel count, sums of the rows,
    of the columns, of their squares and of their products.  l1 = mean + rad >= l2 = mean - rad."""
    n2 = float(n) * float(n)
    trr = float(n * sii - si * si) / n2
    tcc = float(n * sjj - sj * sj) / n2
    trc = float(n * sij - si * sj) / n2
    mean2 = (tcc + trr) * 0.5
    half = (tcc - trr) * 0.5
    rad = math.sqrt(half * half + trc * trc)
    return rad, mean2 + rad, mean2 - rad


def eccentricity_from_sums(n: int, si: int, sj: int, sii: int, sjj: int, sij: int) -> float:
    rad, l1, l2 = inertia_eigenvalues(n, si, sj, sii, sjj, sij)
    if l1 == 0.0:
        return 0.0
    if l2 <= 0.0:
        return 1.0
    return math.sqrt((2.0 * rad) / l1)


def eccentricity_eigvalsh(rr, cc) -> float:
    """The same quantity the way skimage 0.18.3 evaluates it (float moments, np.linalg.eigvalsh): for loose cross-checks."""
    r = rr - rr.mean()
    c = cc - cc.mean()
    n = len(rr)
    mu20, mu02, mu11 = (r * r).sum(), (c * c).sum(), (r * c).sum()
    T = np.array([[mu02, -mu11], [-mu11, mu20]]) / n
    ev = np.clip(np.linalg.eigvalsh(T), 0, None)
    l1, l2 = sorted(ev, reverse=True)
    return 0.0 if l1 == 0 else math.sqrt(1 - l2 / l1)


def intensity(crop: np.ndarray):
    x = [int(v) for v in crop.ravel()]
    N = len(x)
    sx = sum(x)
    sxx = sum(v * v for v in x)
    mean = float(sx) / float(N)
    std = math.sqrt(float(N * sxx - sx * sx) / float(N * N))
    return mean, std


def regions(labels: np.ndarray, ana: np.ndarray, qc=None):
    """Every region of one [H,W] label image in ascending label order, with the fields of cs_region (as a dict)."""
    q = dict(REFERENCE_QC, **(qc or {}))
    H, W = labels.shape
    flat = labels.ravel()
    order = np.argsort(flat, kind="stable")
    vals = flat[order]
    starts = np.searchsorted(vals, np.unique(vals), side="left")
    out = []
    for k, s in enumerate(starts):
        lab = int(vals[s])
        if lab <= 0:
            continue
        e = starts[k + 1] if k + 1 < len(starts) else len(vals)
        idx = order[s:e]
        rr, cc = idx // W, idx % W
        minr, minc, maxr, maxc = int(rr.min()), int(cc.min()), int(rr.max()) + 1, int(cc.max()) + 1
        mask = labels[minr:maxr, minc:maxc] == lab
        area = int(len(idx))
        cvx = convex_area(mask)
        ecc = eccentricity(rr - minr, cc - minc)
        mean, std = intensity(ana[minr:maxr, minc:maxc])
        failed = 0
        b = q["border"]
        if minr < b or minc < b or maxr > H - b or maxc > W - b:
            failed |= QC_BORDER
        if area < q["min_area"] or area > q["max_area"]:
            failed |= QC_AREA
        if ecc > q["max_eccentricity"]:
            failed |= QC_ECCENTRICITY
        if mean < q["min_mean"] or std < q["min_std"]:
            failed |= QC_INTENSITY
        out.append(dict(label=lab, minr=minr, minc=minc, maxr=maxr, maxc=maxc, area=area, convex_area=cvx, eccentricity=ecc,
                        solidity=area / cvx, mean_intensity=mean, std_intensity=std, failed=failed))
    return out


def image_status(regs) -> int:
    sides = [(r["maxr"] - r["minr"], r["maxc"] - r["minc"]) for r in regs if r["failed"] == 0]
    if any(min(s) < 8 for s in sides):
        return IMAGE_NO_CELLS
    if any(max(s) > 1024 for s in sides):
        return IMAGE_UNSUPPORTED
    return IMAGE_OK


def extract(labels: np.ndarray, ana: np.ndarray, qc=None):
    """(raw crops of the passing regions, all regions, status) for one image, as the reference's loop cuts them."""
    regs = regions(labels, ana, qc)
    st = image_status(regs)
    crops = [] if st != IMAGE_OK else [ana[r["minr"]:r["maxr"], r["minc"]:r["maxc"]] for r in regs if r["failed"] == 0]
    return crops, regs, st


def stats(regs):
    """The reference's stats dicts (improved_detection.py:100-106) of the passing regions."""
    return [{"area": r["area"], "eccentricity": r["eccentricity"], "solidity": r["solidity"],
             "mean_intensity": r["mean_intensity"], "std_intensity": r["std_intensity"]} for r in regs if r["failed"] == 0]
