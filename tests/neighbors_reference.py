"""The rule of cs_label_neighbors restated in numpy integers: no tiles, no halos and no tables, so that it shares nothing
with the kernels.

An object is cs_label_intensity's without an `exclude` plane: the pixels of one image with one label > 0, connected or not.  Nothing
crosses between the images of a batch; outside the image there is nothing.  d2 is the squared Euclidean distance between two pixel
centres, an integer.

    border pixel of a      a pixel of a with a 4-neighbour that is not a's, outside the image included
    D2(a, b), a != b       the smallest d2 between a pixel of a and a pixel of b; b is a neighbour of a iff D2(a, b) <= max_d2
    touching               a border pixel of a with a pixel of a label other than 0 and a within max_d2; its nearest foreign label is
                           the label of that pixel at the smallest (d2, label)

The records, row b * max_label + L - 1 for label L of image b:

    geom    [B, max_label, 3] int64    area, sum r, sum c
    objects [B, max_label, 3] int32    border, touching, degree (the number of neighbours)
    offsets [B * max_label + 1] int64  CSR row starts; the last entry is the number of directed pairs
    pairs   [n_pairs, 3] int32         neighbour label, D2(a, b), n_near: the number of a's border pixels whose nearest foreign label is
                                       that neighbour; every row sorted by neighbour label

Only border pixels need to look: the pixel of a closest to any pixel outside a is a border pixel.  measure() looks from the border
pixels over the offsets of the disk, all at once; measure_slow() takes every pair of pixels of an image in Python ints and looks from
every pixel of a, border or not, so that it also holds that sentence.  A negative label, or one above max_label, is refused.
derive() hands the records to the package's host half (cellscreen.neighbors.neighbor_table)."""
import math

import numpy as np

from intensity_reference import contents as _contents
from intensity_reference import disks                   # noqa: F401  (the generators, for the tests and tools)

BIG = 1 << 62


def _check(labels, max_d2, max_label):
    labels = np.asarray(labels)
    if labels.ndim != 3:
        raise ValueError(f"labels {labels.shape}: [B,H,W] expected")
    if not 1 <= int(max_d2) <= 1024:
        raise ValueError(f"max_d2 {max_d2} outside 1..1024")
    if max_label is None:
        max_label = max(1, int(labels.max()))
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) > max_label):
        raise ValueError("a label is negative or exceeds max_label")
    return labels, int(max_d2), int(max_label)


def disk_offsets(max_d2):
    """(dr, dc, d2) int64 arrays of the offsets with 0 < dr^2 + dc^2 <= max_d2"""
    R = math.isqrt(max_d2)
    dr, dc = (x.ravel().astype(np.int64) for x in np.mgrid[-R:R + 1, -R:R + 1])
    d2 = dr * dr + dc * dc
    keep = (d2 > 0) & (d2 <= max_d2)
    return dr[keep], dc[keep], d2[keep]


def border_mask(lab):
    """the border pixels of all objects of one image [H,W]"""
    P = np.pad(lab, 1)
    c = P[1:-1, 1:-1]
    return (c > 0) & ((P[:-2, 1:-1] != c) | (P[2:, 1:-1] != c) | (P[1:-1, :-2] != c) | (P[1:-1, 2:] != c))


def _assemble(B, M, geom, objects, rows):
    """offsets and pairs of rows: {(b, a): {neighbour: [D2, n_near]}}"""
    offsets = np.zeros(B * M + 1, np.int64)
    out = []
    for b in range(B):
        for a in range(1, M + 1):
            row = rows.get((b, a), {})
            objects[b, a - 1, 2] = len(row)
            offsets[b * M + a] = offsets[b * M + a - 1] + len(row)
            out.extend((nb, row[nb][0], row[nb][1]) for nb in sorted(row))
    return geom, objects, offsets, np.array(out, np.int32).reshape(len(out), 3)


# ---- the vectorised form ------------------------------------------------------------------------------------------------------
def measure(labels, max_d2, max_label=None):
    """(geom, objects, offsets, pairs) of labels [B,H,W]."""
    labels, max_d2, M = _check(labels, max_d2, max_label)
    B, H, W = labels.shape
    geom, objects = np.zeros((B, M, 3), np.int64), np.zeros((B, M, 3), np.int32)
    odr, odc, od2 = disk_offsets(max_d2)
    R = math.isqrt(max_d2)
    rows = {}
    for b in range(B):
        lab = labels[b].astype(np.int64)
        rr, cc = np.nonzero(lab)
        if rr.size == 0:
            continue
        for k, x in enumerate((np.ones_like(rr), rr, cc)):
            np.add.at(geom[b, :, k], lab[rr, cc] - 1, x)
        br, bc = np.nonzero(border_mask(lab))
        a = lab[br, bc]
        np.add.at(objects[b, :, 0], a - 1, 1)
        P = np.pad(lab, R)
        best = {}                                       # (a << 21 | neighbour) -> D2
        step = max(1, (1 << 21) // max(1, od2.size))    # border pixels at a time
        for lo in range(0, a.size, step):
            sl = slice(lo, lo + step)
            V = P[br[sl, None] + R + odr[None, :], bc[sl, None] + R + odc[None, :]]      # [border pixel, offset]
            foreign = (V != 0) & (V != a[sl, None])
            near = np.where(foreign, (od2[None, :] << 21) | V, BIG).min(axis=1)
            hit = near < BIG
            np.add.at(objects[b, :, 1], a[sl][hit] - 1, 1)
            for key, cnt in zip(*np.unique((a[sl][hit] << 21) | (near[hit] & ((1 << 21) - 1)), return_counts=True)):
                rows.setdefault((b, int(key) >> 21), {}).setdefault(int(key) & ((1 << 21) - 1), [None, 0])[1] += int(cnt)
            i, j = np.nonzero(foreign)
            pair = (((a[sl][i] << 21) | V[i, j]) << 11) | od2[j]                        # d2 <= 1024 < 2^11: the pair's smallest first
            pair = np.unique(pair)
            first = np.r_[True, (pair[1:] >> 11) != (pair[:-1] >> 11)][:pair.size]
            for p in pair[first].tolist():
                k, d = p >> 11, p & 2047
                if d < best.get(k, BIG):
                    best[k] = d
        for k, d in best.items():
            rows.setdefault((b, k >> 21), {}).setdefault(k & ((1 << 21) - 1), [None, 0])[0] = d
    return _assemble(B, M, geom, objects, rows)


# ---- the slow form ------------------------------------------------------------------------------------------------------------
def measure_slow(labels, max_d2, max_label=None):
    """measure() from all pairs of pixels in Python ints, for tiny images."""
    labels, max_d2, M = _check(labels, max_d2, max_label)
    B, H, W = labels.shape
    geom, objects = np.zeros((B, M, 3), np.int64), np.zeros((B, M, 3), np.int32)
    rows = {}
    for b in range(B):
        at = lambda r, c: int(labels[b, r, c]) if 0 <= r < H and 0 <= c < W else 0
        px = [(r, c, at(r, c)) for r in range(H) for c in range(W) if at(r, c)]
        for r, c, a in px:
            geom[b, a - 1] += (1, r, c)
            is_border = any(at(r + dr, c + dc) != a for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            near = None
            for r2, c2, v in px:                        # from every pixel of a, border or not
                if v == a:
                    continue
                d = (r - r2) ** 2 + (c - c2) ** 2
                if d > max_d2:
                    continue
                e = rows.setdefault((b, a), {}).setdefault(v, [d, 0])
                e[0] = min(e[0], d)
                if near is None or (d, v) < near:
                    near = (d, v)
            if is_border:
                objects[b, a - 1, 0] += 1
                if near is not None:
                    objects[b, a - 1, 1] += 1
                    rows[(b, a)][near[1]][1] += 1
    return _assemble(B, M, geom, objects, rows)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def two_rectangles(h, w, gap, shape=None):
    """labels [1,H,W]: two h x w rectangles, label 1 left of label 2, `gap` background columns between them, one pixel off the image's
    sides (or anywhere in `shape`).  D2(1, 2) = (gap + 1)^2.  For (gap + 1)^2 <= max_d2 < (gap + 2)^2 the touching border pixels of
    either are the h pixels of its facing side: every other border pixel is at least gap + 2 columns from the other rectangle."""
    H, W = shape if shape is not None else (h + 2, 2 * w + gap + 2)
    lab = np.zeros((1, H, W), np.int32)
    lab[0, 1:1 + h, 1:1 + w] = 1
    lab[0, 1:1 + h, 1 + w + gap:1 + 2 * w + gap] = 2
    return lab


# ---- content --------------------------------------------------------------------------------------------------------------------
def contents(shape, seed):
    """The kinds of label content of the device tests on one image shape, as (name, labels [H,W] int32): intensity_reference's three
    (random disks, single pixels with five labels, one label in two far-apart pieces) and a partition of the whole image into random
    Voronoi cells, where every pixel is labelled and every border is shared."""
    H, W = shape
    rng = np.random.default_rng(seed + 1000)
    n = max(2, H * W // 400)
    sr, sc = rng.integers(0, H, n), rng.integers(0, W, n)
    rr, cc = np.indices(shape)
    cells = (np.argmin((rr[..., None] - sr) ** 2 + (cc[..., None] - sc) ** 2, axis=2) + 1).astype(np.int32)
    return _contents(shape, seed) + [("cells", cells)]


# ---- what a table reports -------------------------------------------------------------------------------------------------------
INT_FIELDS = ("image", "label", "area", "border", "touching", "number_of_neighbors", "nearest_edge_label", "first_closest_label",
              "second_closest_label", "row_start", "row_end")
FLOAT_FIELDS = ("centroid", "percent_touching", "nearest_edge_distance", "first_closest_distance", "second_closest_distance",
                "angle_between_neighbors")


def derive(geom, objects, offsets, pairs):
    """The present objects in (image, label) order as a dict of arrays, by the package's host half."""
    from cellscreen import neighbors as NB
    t = NB.neighbor_table(geom, objects, offsets, pairs)
    return {k: getattr(t, k) for k in INT_FIELDS + FLOAT_FIELDS}


def derive_slow(geom, objects, offsets, pairs):
    """derive() object by object with math.sqrt, math.acos and sorted(): the CPU tests hold the package's host half to it."""
    B, M = geom.shape[:2]
    out = {k: [] for k in INT_FIELDS + FLOAT_FIELDS}
    for b in range(B):
        present = [m for m in range(M) if geom[b, m, 0] > 0]
        cen = {m: (int(geom[b, m, 1]) / int(geom[b, m, 0]), int(geom[b, m, 2]) / int(geom[b, m, 0])) for m in present}
        for m in present:
            s, e = int(offsets[b * M + m]), int(offsets[b * M + m + 1])
            row = [(int(d), int(nb)) for nb, d, _ in pairs[s:e]]
            others = sorted((math.sqrt((cen[o][0] - cen[m][0]) ** 2 + (cen[o][1] - cen[m][1]) ** 2), o + 1) for o in present if o != m)
            first = others[0] if len(others) > 0 else (math.nan, 0)
            second = others[1] if len(others) > 1 else (math.nan, 0)
            angle = math.nan
            if len(others) > 1 and first[0] > 0.0 and second[0] > 0.0:
                v1 = (cen[first[1] - 1][0] - cen[m][0], cen[first[1] - 1][1] - cen[m][1])
                v2 = (cen[second[1] - 1][0] - cen[m][0], cen[second[1] - 1][1] - cen[m][1])
                angle = math.degrees(math.acos(max(-1.0, min(1.0, (v1[0] * v2[0] + v1[1] * v2[1]) / (first[0] * second[0])))))
            vals = dict(image=b, label=m + 1, area=int(geom[b, m, 0]), border=int(objects[b, m, 0]), touching=int(objects[b, m, 1]),
                        number_of_neighbors=int(objects[b, m, 2]), nearest_edge_label=min(row)[1] if row else 0,
                        first_closest_label=first[1], second_closest_label=second[1], row_start=s, row_end=e, centroid=list(cen[m]),
                        percent_touching=100.0 * int(objects[b, m, 1]) / int(objects[b, m, 0]),
                        nearest_edge_distance=math.sqrt(min(row)[0]) if row else math.nan, first_closest_distance=first[0],
                        second_closest_distance=second[0], angle_between_neighbors=angle)
            for k, x in vals.items():
                out[k].append(x)
    n = len(out["label"])
    dt = dict(image=np.int32, label=np.int32, area=np.int64, border=np.int32, touching=np.int32, number_of_neighbors=np.int32,
              nearest_edge_label=np.int32, first_closest_label=np.int32, second_closest_label=np.int32, row_start=np.int64, row_end=np.int64)
    return {k: np.array(x, dt.get(k, np.float64)).reshape((n, 2) if k == "centroid" else (n,)) for k, x in out.items()}
