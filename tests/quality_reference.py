"""The focus and saturation records of an image, of a mesh over it and of the objects of a label image (cs_image_quality,
cs_object_focus), restated in numpy int64 and Python ints: what the device tables must equal, entry for entry.

For one channel x of an image [H][W] a pixel is interior iff 1 <= r <= H - 2 and 1 <= c <= W - 2; there is no reflection and no
padding.  At an interior pixel
    L  = x[r-1,c] + x[r+1,c] + x[r,c-1] + x[r,c+1] - 4 x[r,c]
    G  = gx^2 + gy^2, gx and gy the 3 x 3 Sobel responses (weights 1-2-1)
    Br = (x[r,c+1] - x[r,c-1])^2 + (x[r+1,c] - x[r-1,c])^2
    records [B, C, 13]                 int64   n, sum v, sum v^2, min, max, n_at_min, n_at_max, n_sat, n_int, sum L, sum L^2,
                                               sum G, sum Br
    mesh    [B, C, m_r, m_c, 8]        int64   n, sum v, sum v^2, n_int, sum L, sum L^2, sum G, sum Br; m = ceil(side / tile),
                                               pixel (r, c) in tile ((r m_r) // H, (c m_c) // W)
    geom    [B, max_label, 3]          int64   area, sum r, sum c (cs_label_intensity's)
    focus   [B, max_label, C, 5]       int64   n_int, sum L, sum L^2, sum G, sum Br over the object's pixels interior to the image
"""
import math
from fractions import Fraction

import numpy as np

REC = ("n", "sv", "sv2", "min", "max", "n_at_min", "n_at_max", "n_sat", "n_int", "sl", "sl2", "sg", "sbr")
TILE = ("n", "sv", "sv2", "n_int", "sl", "sl2", "sg", "sbr")


def _image4(image):
    image = np.asarray(image)
    if image.dtype not in (np.uint8, np.uint16):
        raise TypeError(f"image dtype {image.dtype}")
    if image.ndim == 3:
        image = image[..., None]
    if image.ndim != 4:
        raise ValueError(f"image shape {image.shape}")
    return image


def focus_planes(x):
    """(interior, L, G, Br) of one channel x [H,W]: int64 planes [H,W], 0 off the interior; interior is a bool plane."""
    x = np.asarray(x).astype(np.int64)
    H, W = x.shape
    inside = np.zeros((H, W), bool)
    L, G, Br = (np.zeros((H, W), np.int64) for _ in range(3))
    if H < 3 or W < 3:
        return inside, L, G, Br
    inside[1:-1, 1:-1] = True
    a, m, n = x[:-2], x[1:-1], x[2:]                    # the rows above, of and below the interior rows
    L[1:-1, 1:-1] = a[:, 1:-1] + n[:, 1:-1] + m[:, :-2] + m[:, 2:] - 4 * m[:, 1:-1]
    gx = (a[:, 2:] + 2 * m[:, 2:] + n[:, 2:]) - (a[:, :-2] + 2 * m[:, :-2] + n[:, :-2])
    gy = (n[:, :-2] + 2 * n[:, 1:-1] + n[:, 2:]) - (a[:, :-2] + 2 * a[:, 1:-1] + a[:, 2:])
    G[1:-1, 1:-1] = gx * gx + gy * gy
    Br[1:-1, 1:-1] = (m[:, 2:] - m[:, :-2]) ** 2 + (n[:, 1:-1] - a[:, 1:-1]) ** 2
    return inside, L, G, Br


def mesh_dims(H, W, tile):
    return (-(-H // tile), -(-W // tile)) if tile else (1, 1)


def tile_index(side, m):
    """The tile of every pixel along one axis: (i * m) // side."""
    return (np.arange(side, dtype=np.int64) * m) // side


def top_of(dtype):
    return int(np.iinfo(dtype).max)


def measure_image(image, tile=0, sat_level=None):
    """(records, mesh) of image [B,H,W] or [B,H,W,C]; mesh is None with tile == 0.  sat_level: None (the dtype's top) or one
    level per channel."""
    image = _image4(image)
    B, H, W, C = image.shape
    if tile and not 16 <= tile <= 1024:
        raise ValueError(f"tile {tile}")
    sat = [top_of(image.dtype)] * C if sat_level is None else [int(s) for s in sat_level]
    if len(sat) != C:
        raise ValueError("one sat_level per channel")
    m_r, m_c = mesh_dims(H, W, tile)
    flat = (tile_index(H, m_r)[:, None] * m_c + tile_index(W, m_c)[None, :]).ravel()
    records = np.zeros((B, C, 13), np.int64)
    mesh = np.zeros((B, C, m_r, m_c, 8), np.int64)
    for b in range(B):
        for ch in range(C):
            v = image[b, :, :, ch].astype(np.int64)
            inside, L, G, Br = focus_planes(v)
            planes = (np.ones_like(v), v, v * v, inside.astype(np.int64), L, L * L, G, Br)
            for j, q in enumerate(planes):
                # exact: the largest tile sum, sum G at 1024^2 pixels, is below 2^58, and bincount's float64 weights would
                # round it, so the sums are taken in int64 by np.add.at
                acc = np.zeros(m_r * m_c, np.int64)
                np.add.at(acc, flat, q.ravel())
                mesh[b, ch, :, :, j] = acc.reshape(m_r, m_c)
            lo, hi = int(v.min()), int(v.max())
            t = mesh[b, ch].reshape(-1, 8).sum(axis=0)
            records[b, ch] = (t[0], t[1], t[2], lo, hi, int((v == lo).sum()), int((v == hi).sum()), int((v >= sat[ch]).sum()),
                              t[3], t[4], t[5], t[6], t[7])
    return records, (mesh if tile else None)


def measure_image_slow(image, tile=0, sat_level=None):
    """measure_image(), pixel by pixel in Python ints."""
    image = _image4(image)
    B, H, W, C = image.shape
    sat = [top_of(image.dtype)] * C if sat_level is None else [int(s) for s in sat_level]
    m_r, m_c = mesh_dims(H, W, tile)
    records = np.zeros((B, C, 13), np.int64)
    mesh = np.zeros((B, C, m_r, m_c, 8), np.int64)
    for b in range(B):
        for ch in range(C):
            x = [[int(t) for t in row] for row in image[b, :, :, ch]]
            vals = [t for row in x for t in row]
            lo, hi = min(vals), max(vals)
            rec = [0] * 13
            rec[3], rec[4] = lo, hi
            for r in range(H):
                for c in range(W):
                    v = x[r][c]
                    t = [1, v, v * v, 0, 0, 0, 0, 0]
                    if 1 <= r <= H - 2 and 1 <= c <= W - 2:
                        lap = x[r - 1][c] + x[r + 1][c] + x[r][c - 1] + x[r][c + 1] - 4 * v
                        gx = sum(w * (x[r + d][c + 1] - x[r + d][c - 1]) for d, w in ((-1, 1), (0, 2), (1, 1)))
                        gy = sum(w * (x[r + 1][c + d] - x[r - 1][c + d]) for d, w in ((-1, 1), (0, 2), (1, 1)))
                        br = (x[r][c + 1] - x[r][c - 1]) ** 2 + (x[r + 1][c] - x[r - 1][c]) ** 2
                        t[3:] = [1, lap, lap * lap, gx * gx + gy * gy, br]
                    tr, tc = (r * m_r) // H, (c * m_c) // W
                    for j in range(8):
                        mesh[b, ch, tr, tc, j] += t[j]
                    for j, k in enumerate((0, 1, 2, 8, 9, 10, 11, 12)):
                        rec[k] += t[j]
                    rec[5] += v == lo
                    rec[6] += v == hi
                    rec[7] += v >= sat[ch]
            records[b, ch] = rec
    return records, (mesh if tile else None)


def measure_objects(image, labels, exclude=None, max_label=None):
    """(geom, focus) of image [B,H,W] or [B,H,W,C], labels [B,H,W] int32 and exclude (None or [B,H,W])."""
    image, labels = _image4(image), np.asarray(labels)
    B, H, W, C = image.shape
    if labels.shape != (B, H, W):
        raise ValueError("labels and image differ in shape")
    if max_label is None:
        max_label = max(1, int(labels.max()))
    if labels.min() < 0 or labels.max() > max_label:
        raise ValueError("a label is negative or exceeds max_label")
    eff = labels.astype(np.int64) if exclude is None else np.where(np.asarray(exclude) != 0, 0, labels).astype(np.int64)
    geom = np.zeros((B, max_label, 3), np.int64)
    focus = np.zeros((B, max_label, C, 5), np.int64)
    rr, cc = np.mgrid[0:H, 0:W].astype(np.int64)
    for b in range(B):
        on = eff[b] > 0
        row = eff[b][on] - 1
        for j, q in enumerate((np.ones((H, W), np.int64), rr, cc)):
            np.add.at(geom[b, :, j], row, q[on])
        for ch in range(C):
            inside, L, G, Br = focus_planes(image[b, :, :, ch])
            for j, q in enumerate((inside.astype(np.int64), L, L * L, G, Br)):
                np.add.at(focus[b, :, ch, j], row, q[on])
    return geom, focus


# ---- derived values: each one correctly rounded quotient of Python ints -------------------------------------------------------
def ratio(num, den):
    return float(Fraction(int(num), int(den))) if den else float("nan")


def is_rounded_sqrt(f, num, den):
    """Whether the float f is sqrt(num / den) rounded to nearest: num / den lies between the squares of the midpoints to f's two
    neighbours, taken in Fractions."""
    x = Fraction(int(num), int(den))
    if x == 0:
        return f == 0.0
    lo = (Fraction(f) + Fraction(math.nextafter(f, 0.0))) / 2
    hi = (Fraction(f) + Fraction(math.nextafter(f, math.inf))) / 2
    return f > 0 and lo * lo <= x <= hi * hi


def sqrt_ratio(num, den2):
    """sqrt(num / den2) with ONE rounding, by search: start at the twice rounded value and step to the neighbour that brackets."""
    if not den2:
        return float("nan")
    f = math.sqrt(ratio(num, den2))
    for cand in (f, math.nextafter(f, 0.0), math.nextafter(f, math.inf)):
        if is_rounded_sqrt(cand, num, den2):
            return cand
    raise AssertionError("the rounded root is not next to the twice rounded one")


def derive_record(n, sv, sv2, n_int, sl, sl2, sg, sbr):
    n, sv, sv2, n_int, sl, sl2, sg, sbr = (int(t) for t in (n, sv, sv2, n_int, sl, sl2, sg, sbr))
    return dict(mean=ratio(sv, n), std=sqrt_ratio(n * sv2 - sv * sv, n * n), focus_score=ratio(n * sv2 - sv * sv, n * sv),
                laplacian_variance=ratio(n_int * sl2 - sl * sl, n_int * n_int), tenengrad=ratio(sg, n_int), brenner=ratio(sbr, n_int))


def normalised_variance(n, sv, sv2):
    """(n sum v^2 - (sum v)^2) / (n sum v) as a Fraction, None where sum v = 0."""
    n, sv, sv2 = int(n), int(sv), int(sv2)
    return Fraction(n * sv2 - sv * sv, n * sv) if sv > 0 else None


def local_focus_score(tiles):
    """tiles [m, 8]: var(nv) / median(nv) over the tiles with sum v > 0, population variance, numpy's median (the mean of the two
    middle values of an even count), in Fractions; 0 where the median is 0, NaN without such a tile."""
    nv = sorted(t for t in (normalised_variance(*row[:3]) for row in np.asarray(tiles).reshape(-1, 8)) if t is not None)
    if not nv:
        return float("nan")
    k = len(nv)
    med = nv[k // 2] if k % 2 else (nv[k // 2 - 1] + nv[k // 2]) / 2
    if med == 0:
        return 0.0
    mean = sum(nv, Fraction(0)) / k
    var = sum(((t - mean) ** 2 for t in nv), Fraction(0)) / k
    return float(var / med)


# ---- test content -----------------------------------------------------------------------------------------------------------
def noise(shape, channels, dtype, seed):
    """Uniform noise [..., channels] of dtype over its whole range, with pixels forced to 0 and to the dtype's top."""
    rng = np.random.default_rng(seed)
    top = top_of(dtype)
    a = rng.integers(0, top + 1, size=tuple(shape) + (channels,)).astype(dtype)
    flat = a.reshape(-1)
    k = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, k)] = 0
    flat[rng.integers(0, flat.size, k)] = top
    return a


def checkerboard(shape, dtype):
    r, c = np.indices(shape)
    return (((r + c) & 1) * top_of(dtype)).astype(dtype)


def stripes4(shape, dtype):
    """Columns 0, 0, top, top, ..."""
    return np.broadcast_to((((np.arange(shape[1]) >> 1) & 1) * top_of(dtype)).astype(dtype), shape).copy()
