"""CPU restatement of the spot detector (cs_spot_detect / cs_spot_fill in csrc/spots.hip, cellscreen.SpotDetector): what the device
kernels are compared against bit for bit, with numpy only.

  response   R = (A_a - A_b + 2^23) >> 24, int32 in 1/256 counts: A_t = sum w_t sum w_t x, the separable 48-bit sums of
             smooth_reference._pass under the fine table w_a (None or [65536]: the identity, A_a = x * 2^32) and the coarse
             table w_b, indices folded by local_reference.fold; the shift floors the signed difference.  |R| < 2^24, and a constant
             image gives 0 everywhere.
  response_direct   the same straight from the 2-D definition, Python ints
  peaks      a pixel is a spot iff R >= T and its key (R, -raster index) is strictly the greatest among the pixels with
             |dr| <= m, |dc| <= m, clipped to the image: no two spots within Chebyshev distance m, of a plateau the first pixel
             in raster order where any
  detect     a batch: counts [B,2] (spots, spots on label 0), offsets [B+1], the list [n,8] int32 (r, c, label, R, R above, below,
             left, right; INT32_MIN outside) sorted by image and raster order, and with labels geom [B,max_label,3] (area, sum r,
             sum c: cs_label_intensity's) and spots [B,max_label,6] (n, sum R, sum R^2, max R, sum r, sum c), int64; the label of
             a spot is labels[b, r, c], 0 where exclude is non-zero or without labels; the response planes [B,H,W] int32
Deliberately not skimage.feature.peak_local_max / blob_dog: the response is a floor-rounded integer, ties go to the raster order
and the window is a square (Chebyshev), where peak_local_max prunes by Euclidean distance.  tests/golden/golden_spots.npz
(tools/make_golden_spots.py) pins the response to SciPy's float64 gaussian_filter difference within the quantisation bound."""
import numpy as np

from local_reference import fold
from smooth_reference import ONE, _pass

MAX_R = 64
MAX_M = 8
INT32_MIN = -(1 << 31)
FIELDS, RECORD = 8, 6


def check_tables(w_a, w_b):
    """(w_a, w_b) as lists of ints, w_a [65536] for the identity; ValueError as the device refuses."""
    w_a = [ONE] if w_a is None else [int(v) for v in w_a]
    w_b = [int(v) for v in w_b]
    for name, w, lo in (("w_a", w_a, 0), ("w_b", w_b, 1)):
        r = len(w) - 1
        if not lo <= r <= MAX_R:
            raise ValueError(f"{name}: radius {r} outside {lo}..{MAX_R}")
        if min(w) < 0 or w[0] < 1 or w[0] + 2 * sum(w[1:]) != ONE:
            raise ValueError(f"{name}: weights must be non-negative with w[0] >= 1 and w[0] + 2 * sum(w[1:]) == 65536")
    if w_a == w_b:
        raise ValueError("equal tables")
    return w_a, w_b


def _sum48(x, w):
    t = _pass(x.astype(np.uint64), w)
    assert int(t.max()) < 1 << 32
    a = _pass(np.ascontiguousarray(t.T), w).T
    assert int(a.max()) < 1 << 48
    return a.astype(np.int64)


def response(x: np.ndarray, w_a, w_b) -> np.ndarray:
    """R of one 2-D uint8 / uint16 plane, int32."""
    if x.ndim != 2 or x.dtype not in (np.uint8, np.uint16):
        raise TypeError("2-D uint8 / uint16 image expected")
    w_a, w_b = check_tables(w_a, w_b)
    d = _sum48(x, w_a) - _sum48(x, w_b)
    out = (d + np.int64(1 << 23)) >> np.int64(24)        # numpy's >> of a signed integer floors
    assert int(np.abs(out).max()) < 1 << 24
    return out.astype(np.int32)


def response_direct(x: np.ndarray, w_a, w_b) -> np.ndarray:
    w_a, w_b = check_tables(w_a, w_b)
    H, W = x.shape
    xo = x.astype(object)
    out = np.zeros((H, W), np.int32)

    def sum2(w, i, j):
        r = len(w) - 1
        rows, cols = fold(np.arange(i - r, i + r + 1), H), fold(np.arange(j - r, j + r + 1), W)
        k = np.array([w[abs(d)] for d in range(-r, r + 1)], dtype=object)
        return int((k[:, None] * k[None, :] * xo[np.ix_(rows, cols)]).sum())

    for i in range(H):
        for j in range(W):
            out[i, j] = (sum2(w_a, i, j) - sum2(w_b, i, j) + (1 << 23)) >> 24      # Python's >> floors
    return out


def keys(R: np.ndarray) -> np.ndarray:
    """int64 keys that order the pixels as (R, -raster index) does."""
    H, W = R.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    return R.astype(np.int64) * (1 << 32) + ((1 << 32) - 1 - idx)


def peaks(R: np.ndarray, T: int, m: int) -> np.ndarray:
    """bool [H,W]: the spots of one response plane."""
    if not 1 <= m <= MAX_M:
        raise ValueError(f"m {m} outside 1..{MAX_M}")
    if T < 1:
        raise ValueError("T must be >= 1")
    H, W = R.shape
    k = keys(R)
    low = np.iinfo(np.int64).min
    p = np.full((H + 2 * m, W + 2 * m), low, np.int64)
    p[m:m + H, m:m + W] = k
    best = np.full((H, W), low, np.int64)
    for dr in range(-m, m + 1):
        for dc in range(-m, m + 1):
            if dr or dc:
                best = np.maximum(best, p[m + dr:m + dr + H, m + dc:m + dc + W])
    return (R >= T) & (k > best)


def geometry(labels, exclude, max_label):
    """geom [B,max_label,3] int64: area, sum r, sum c of every object, less the excluded pixels."""
    B, H, W = labels.shape
    if labels.min() < 0 or labels.max() > max_label:
        raise ValueError("a label is negative or exceeds max_label")
    geom = np.zeros((B, max_label, 3), np.int64)
    keep = labels > 0
    if exclude is not None:
        keep &= exclude == 0
    b, r, c = np.nonzero(keep)
    row = labels[b, r, c] - 1
    np.add.at(geom[:, :, 0], (b, row), 1)
    np.add.at(geom[:, :, 1], (b, row), r)
    np.add.at(geom[:, :, 2], (b, row), c)
    return geom


def detect(images, thresholds, w_a, w_b, m, channel=0, labels=None, exclude=None, max_label=None):
    """(counts, offsets, list, geom, spots, response) of a batch [B,H,W] or [B,H,W,C]; thresholds: one int (1/256 counts) per
    image; geom and spots are None without labels."""
    chan = images if images.ndim == 3 else images[..., channel]
    B, H, W = chan.shape
    thresholds = [int(t) for t in thresholds]
    assert len(thresholds) == B
    if labels is not None:
        max_label = int(labels.max()) if max_label is None else int(max_label)
        max_label = max(1, max_label)
        geom = geometry(labels, exclude, max_label)
        table = np.zeros((B, max_label, RECORD), np.int64)
    else:
        assert exclude is None
        geom = table = None
    counts = np.zeros((B, 2), np.int64)
    offsets = np.zeros(B + 1, np.int64)
    rows, planes = [], []
    for b in range(B):
        R = response(np.ascontiguousarray(chan[b]), w_a, w_b)
        planes.append(R)
        rr, cc = np.nonzero(peaks(R, thresholds[b], m))                    # raster order
        pad = np.full((H + 2, W + 2), INT32_MIN, np.int64)
        pad[1:-1, 1:-1] = R
        lab = np.zeros(len(rr), np.int64)
        if labels is not None:
            lab = labels[b, rr, cc].astype(np.int64)
            if exclude is not None:
                lab[exclude[b, rr, cc] != 0] = 0
        v = R[rr, cc].astype(np.int64)
        rows.append(np.stack([rr, cc, lab, v, pad[rr, cc + 1], pad[rr + 2, cc + 1], pad[rr + 1, cc], pad[rr + 1, cc + 2]], axis=1))
        counts[b] = len(rr), int((lab == 0).sum())
        offsets[b + 1] = offsets[b] + len(rr)
        if labels is not None:
            on = lab > 0
            t, lo = table[b], lab[on] - 1
            np.add.at(t[:, 0], lo, 1)
            np.add.at(t[:, 1], lo, v[on])
            np.add.at(t[:, 2], lo, v[on] * v[on])
            np.maximum.at(t[:, 3], lo, v[on])
            np.add.at(t[:, 4], lo, rr[on])
            np.add.at(t[:, 5], lo, cc[on])
    lst = np.concatenate(rows).astype(np.int32).reshape(-1, FIELDS)
    return counts, offsets, lst, geom, table, np.stack(planes)
