"""CPU restatement of the segmenter's split_touching option (cs_segment_split of csrc/segment.hip): a
distance-transform watershed that is a function of the mask alone, with numpy and scipy.ndimage only, in synchronous rounds.

  dq            Dq = min(isqrt(4 * D2), 255): the distance to the nearest background pixel of the image in half pixels, D2 the
                exact squared Euclidean distance (scipy's distance_transform_edt squared and rounded).  Outside the image is
                not background; an image without background is 255 everywhere.
  reconstruct   R: morphological reconstruction by dilation of max(Dq - h, 0) under Dq, the fixed point of
                R <- min(dilate(R), Dq) (skimage.morphology.reconstruction; tests/golden/golden_split.npz pins it).
  seeds         the regional maxima of R inside the mask (plateaus of equal R without a higher neighbour), numbered by the
                raster order of their first pixels.
  flood         for v = 255 .. 1: unlabelled pixels of mask & (Dq >= v) take, round after round, the smallest label among
                their labelled neighbours: the (steps, label) key of the definition.
  split         all of it, renumbered by each region's first pixel: scipy.ndimage.label's ids where nothing is split.
One neighbourhood (connectivity 1: 4 neighbours, 2: 8) is used throughout."""
import numpy as np
from scipy import ndimage

from segment_reference import STRUCTURES, mask_of, otsu

BIG = np.int32(2 ** 31 - 1)


def dq(mask: np.ndarray):
    """(Dq uint8, D2 int64) of a boolean mask."""
    mask = np.asarray(mask, bool)
    if mask.all():
        return np.full(mask.shape, 255, np.uint8), np.full(mask.shape, 2 ** 62, np.int64)
    d2 = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)
    n = 4 * d2
    s = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    s -= s * s > n
    s += (s + 1) * (s + 1) <= n
    return np.minimum(s, 255).astype(np.uint8), d2


def reconstruct(Dq: np.ndarray, h: int, connectivity: int = 1) -> np.ndarray:
    R = np.maximum(Dq.astype(np.int16) - h, 0).astype(np.uint8)
    while True:
        N = np.minimum(ndimage.grey_dilation(R, footprint=STRUCTURES[connectivity], mode="constant", cval=0), Dq)
        if np.array_equal(N, R):
            return R
        R = N


def seeds(R: np.ndarray, mask: np.ndarray, connectivity: int = 1):
    """(seed labels int32, count): plateaus of equal R inside the mask with no higher neighbour."""
    st = STRUCTURES[connectivity]
    plat = np.zeros(R.shape, np.int64)
    n = 0
    for val in np.unique(R[mask]):
        lab, k = ndimage.label(mask & (R == val), structure=st)
        plat[lab > 0] = lab[lab > 0] + n
        n += k
    higher = mask & (ndimage.grey_dilation(R, footprint=st, mode="constant", cval=0) > R)
    ok = np.ones(n + 1, bool)
    ok[0] = False
    ok[np.unique(plat[higher])] = False
    first = np.full(n + 1, R.size, np.int64)
    np.minimum.at(first, plat.ravel(), np.arange(R.size))
    ids = np.flatnonzero(ok)
    rank = np.zeros(n + 1, np.int32)
    rank[ids[np.argsort(first[ids])]] = np.arange(1, len(ids) + 1)
    return rank[plat], len(ids)


def flood(seed_lab: np.ndarray, Dq: np.ndarray, mask: np.ndarray, connectivity: int = 1) -> np.ndarray:
    lab = seed_lab.astype(np.int32).copy()
    st = STRUCTURES[connectivity]
    for v in range(int(Dq.max()) if Dq.size else 0, 0, -1):
        E = mask & (Dq >= v)
        while (E & (lab == 0)).any():
            nb = ndimage.minimum_filter(np.where(lab > 0, lab, BIG), footprint=st, mode="constant", cval=BIG)
            new = E & (lab == 0) & (nb < BIG)
            if not new.any():
                break
            lab[new] = nb[new]
    return lab


def renumber(lab: np.ndarray):
    n = int(lab.max()) if lab.size else 0
    first = np.full(n + 1, lab.size, np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(lab.size))
    rank = np.zeros(n + 1, np.int32)
    rank[1 + np.argsort(first[1:])] = np.arange(1, n + 1)
    return rank[lab], n


def split_mask(mask: np.ndarray, connectivity: int = 1, h: int = 3):
    """(labels int32, n_labels, Dq uint8) of one boolean mask."""
    mask = np.asarray(mask, bool)
    Dq, _ = dq(mask)
    s, _ = seeds(reconstruct(Dq, h, connectivity), mask, connectivity)
    lab, n = renumber(flood(s, Dq, mask, connectivity))
    return lab.astype(np.int32), n, Dq


def split(channel: np.ndarray, threshold="otsu", connectivity: int = 1, fill_holes: bool = True, h: int = 3):
    """(labels, n_labels, threshold, Dq) of one 2-D integer image: segment_reference.segment with the split."""
    t = otsu(channel) if threshold == "otsu" else int(threshold)
    lab, n, Dq = split_mask(mask_of(channel, t, fill_holes), connectivity, h)
    return lab, n, t, Dq


def split_batch(images: np.ndarray, channel=None, **kw):
    """The restatement of ThresholdSegmenter(split_touching=True).segment_batch(..., return_distance=True)."""
    if images.ndim == 3:
        chan = images
    else:
        chan = images[..., channel if channel is not None else (2 if images.shape[3] >= 3 else 0)]
    out = [split(c, **kw) for c in chan]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32),
            np.stack([o[3] for o in out]))


def ten_disks():
    """The scene the option was specified on: 200 x 300, ten disks, three touching pairs and a touching triple."""
    disks = [(60, 60, 20), (60, 95, 20), (150, 60, 30), (150, 98, 10), (100, 200, 25), (60, 250, 6), (60, 262, 7), (150, 250, 15),
             (165, 270, 15), (140, 275, 15)]
    yy, xx = np.mgrid[0:200, 0:300]
    each = [(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r for cy, cx, r in disks]
    return np.any(each, axis=0), each
