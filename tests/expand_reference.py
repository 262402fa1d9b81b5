"""The rule of cs_label_expand restated from its definition in numpy, all integers: for every background pixel the
squared distances to ALL labelled pixels of its image, no transform and no passes, so that it shares nothing with the kernels.

    D2      the least squared Euclidean distance from a background pixel to a pixel with a label > 0 of the same image
    label   where D2 <= max_d2: the smallest label among the pixels at that D2; labelled pixels keep theirs; else 0
    d2      uint16: 0 on labelled pixels, D2 where it is <= max_d2, 65535 elsewhere

max_d2_of(distance) is the largest integer n with math.sqrt(n) <= float(distance): skimage.segmentation.expand_labels decides
`distance_transform_edt(labels == 0) <= distance` on float64 square roots of exact integers, which is this."""
import math

import numpy as np

FAR = 65535
MAX_DISTANCE = 127


def max_d2_of(distance):
    if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, float, np.integer, np.floating)):
        raise TypeError(f"distance {distance!r}: a number")
    d = float(distance)
    if not 1.0 <= d <= MAX_DISTANCE:                    # a NaN fails both
        raise ValueError(f"distance {distance!r} outside 1..{MAX_DISTANCE}")
    n = int(d) ** 2                                     # sqrt is exact on squares: n is never above the answer
    while math.sqrt(n + 1) <= d:
        n += 1
    return n


NONE = 1 << 40                                          # the D2 of a pixel in an image without labels


def nearest_one(labels, chunk_elems=1 << 22):
    """(D2 int64 [H,W], label int32 [H,W]) of one image, whatever the distance: the least squared distance to a labelled pixel
    (0 on labelled pixels, NONE in an image without any) and the smallest label at that distance."""
    lab = np.asarray(labels)
    if lab.ndim != 2:
        raise ValueError(f"one image expected, got shape {lab.shape}")
    if lab.size and int(lab.min()) < 0:
        raise ValueError("negative label")
    who = lab.astype(np.int32).copy()
    best = np.where(lab > 0, 0, NONE).astype(np.int64)
    ys, xs = np.nonzero(lab > 0)
    by, bx = np.nonzero(lab == 0)
    if ys.size == 0 or by.size == 0:
        return best, who
    ys, xs, ids = ys.astype(np.int64), xs.astype(np.int64), lab[ys, xs].astype(np.int64)
    step = max(1, chunk_elems // ys.size)
    for a in range(0, by.size, step):
        py, px = by[a:a + step].astype(np.int64), bx[a:a + step].astype(np.int64)
        dist = (py[:, None] - ys[None, :]) ** 2 + (px[:, None] - xs[None, :]) ** 2
        key = ((dist << 32) | ids[None, :]).min(axis=1)                 # (D2, label) in lexicographic order
        best[py, px] = key >> 32
        who[py, px] = (key & 0xFFFFFFFF).astype(np.int32)
    return best, who


def nearest(labels):
    """nearest_one of an image [H,W] or of every image of a batch [B,H,W]."""
    lab = np.asarray(labels)
    if lab.ndim == 2:
        return nearest_one(lab)
    b, w = zip(*(nearest_one(x) for x in lab))
    return np.stack(b), np.stack(w)


def cut(near, max_d2):
    """(grown int32, d2 uint16) at max_d2 from what nearest returned."""
    best, who = near
    ok = best <= max_d2
    return np.where(ok, who, 0).astype(np.int32), np.where(ok, best, FAR).astype(np.uint16)


def expand(labels, max_d2):
    """(grown, d2) of an image [H,W] or of a batch [B,H,W], image by image."""
    return cut(nearest(labels), max_d2)


def disks(shape, n, seed, radii=(3, 7), ids=None):
    """n random disks of radius radii[0]..radii[1] on `shape`, later ones over earlier ones; ids: the labels (default 1..n)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    lab = np.zeros(shape, np.int32)
    for k in range(n):
        y, x, r = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1])), int(rng.integers(radii[0], radii[1] + 1))
        lab[(yy - y) ** 2 + (xx - x) ** 2 <= r * r] = (k + 1) if ids is None else ids[k]
    return lab
