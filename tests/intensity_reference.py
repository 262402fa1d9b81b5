"""The rule of cs_label_intensity restated in numpy integers: no tiles, no runs and no tables in between, so that
it shares nothing with the kernels.

An object is the set of pixels of one image with one label > 0, connected or not, less the pixels where `exclude` is non-zero.
With r, c the row and column of a pixel in its image and v its value in a channel, the dense tables are

    geom  [B, max_label, 3]     int64   area, sum r, sum c
    stats [B, max_label, C, 6]  int64   sum v, sum v^2, sum v*r, sum v*c, min v, max v

row label - 1 for label `label`; an object without pixels has all-zero rows, its minimum included.  A negative label, or one
above max_label, is refused whatever `exclude` holds there.  measure() is the vectorised form (a stable sort by label and
np.add.reduceat on int64), measure_slow() walks the pixels with Python ints.  derive() takes the values a table reports from the
integers: Python-int true division and math.sqrt of the exact numerator."""
import math

import numpy as np

from expand_reference import disks                      # noqa: F401  (the small label generator, for the tests and tools)


def _planes(image, labels, exclude, max_label):
    image, labels = np.asarray(image), np.asarray(labels)
    if image.ndim == labels.ndim:
        image = image[..., None]
    if labels.ndim != 3 or image.shape[:3] != labels.shape:
        raise ValueError(f"image {image.shape} and labels {labels.shape}: [B,H,W(,C)] and [B,H,W] expected")
    if exclude is None:
        exclude = np.zeros(labels.shape, np.int32)
    exclude = np.asarray(exclude)
    if exclude.shape != labels.shape:
        raise ValueError("exclude and labels differ in shape")
    if max_label is None:
        max_label = max(1, int(labels.max()))
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) > max_label):
        raise ValueError("a label is negative or exceeds max_label")
    return image, labels, exclude, int(max_label)


def measure(image, labels, exclude=None, max_label=None):
    """(geom, stats) of image [B,H,W] or [B,H,W,C], labels [B,H,W] and exclude (None or [B,H,W])."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    B, C = labels.shape[0], image.shape[3]
    geom = np.zeros((B, max_label, 3), np.int64)
    stats = np.zeros((B, max_label, C, 6), np.int64)
    for b in range(B):
        rr, cc = np.nonzero((labels[b] > 0) & (exclude[b] == 0))
        if rr.size == 0:
            continue
        lab = labels[b][rr, cc].astype(np.int64)
        order = np.argsort(lab, kind="stable")
        lab, rr, cc = lab[order], rr[order].astype(np.int64), cc[order].astype(np.int64)
        starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
        rows = lab[starts] - 1
        geom[b, rows, 0] = np.add.reduceat(np.ones_like(lab), starts)
        geom[b, rows, 1] = np.add.reduceat(rr, starts)
        geom[b, rows, 2] = np.add.reduceat(cc, starts)
        for ch in range(C):
            v = image[b][rr, cc, ch].astype(np.int64)
            for k, x in enumerate((v, v * v, v * rr, v * cc)):
                stats[b, rows, ch, k] = np.add.reduceat(x, starts)
            stats[b, rows, ch, 4] = np.minimum.reduceat(v, starts)
            stats[b, rows, ch, 5] = np.maximum.reduceat(v, starts)
    return geom, stats


def measure_slow(image, labels, exclude=None, max_label=None):
    """measure(), pixel by pixel in Python ints."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    B, H, W = labels.shape
    C = image.shape[3]
    geom = [[[0, 0, 0] for _ in range(max_label)] for _ in range(B)]
    stats = [[[[0, 0, 0, 0, None, None] for _ in range(C)] for _ in range(max_label)] for _ in range(B)]
    for b in range(B):
        for r in range(H):
            for c in range(W):
                lab = int(labels[b, r, c])
                if lab == 0 or int(exclude[b, r, c]) != 0:
                    continue
                g = geom[b][lab - 1]
                g[0] += 1
                g[1] += r
                g[2] += c
                for ch in range(C):
                    v = int(image[b, r, c, ch])
                    s = stats[b][lab - 1][ch]
                    s[0] += v
                    s[1] += v * v
                    s[2] += v * r
                    s[3] += v * c
                    s[4] = v if s[4] is None else min(s[4], v)
                    s[5] = v if s[5] is None else max(s[5], v)
    st = np.array([[[[0 if x is None else x for x in s] for s in row] for row in im] for im in stats], np.int64).reshape(B, max_label, C, 6)
    return np.array(geom, np.int64).reshape(B, max_label, 3), st


def derive(geom, stats):
    """The present objects in (image, label) order as a dict of arrays: image, label, area, centroid [n,2], integrated, mean,
    std, min, max [n,C], weighted_centroid [n,C,2] (NaN where sum v = 0), geom [n,3], stats [n,C,6]."""
    B, M, C = stats.shape[:3]
    keys = [(b, m) for b in range(B) for m in range(M) if geom[b, m, 0] > 0]
    n = len(keys)
    out = dict(image=np.array([b for b, _ in keys], np.int32).reshape(n), label=np.array([m + 1 for _, m in keys], np.int32).reshape(n),
               area=np.zeros(n, np.int64), centroid=np.zeros((n, 2)), integrated=np.zeros((n, C), np.int64), mean=np.zeros((n, C)),
               std=np.zeros((n, C)), min=np.zeros((n, C), np.int64), max=np.zeros((n, C), np.int64),
               weighted_centroid=np.full((n, C, 2), np.nan), geom=np.zeros((n, 3), np.int64), stats=np.zeros((n, C, 6), np.int64))
    for i, (b, m) in enumerate(keys):
        a, sr, sc = (int(x) for x in geom[b, m])
        out["area"][i] = a
        out["centroid"][i] = sr / a, sc / a
        out["geom"][i] = geom[b, m]
        out["stats"][i] = stats[b, m]
        for ch in range(C):
            sv, sv2, svr, svc, lo, hi = (int(x) for x in stats[b, m, ch])
            out["integrated"][i, ch], out["min"][i, ch], out["max"][i, ch] = sv, lo, hi
            out["mean"][i, ch] = sv / a
            out["std"][i, ch] = math.sqrt(a * sv2 - sv * sv) / a
            if sv > 0:
                out["weighted_centroid"][i, ch] = svr / sv, svc / sv
    return out


def contents(shape, seed):
    """The three kinds of label content of the device tests on one image shape, as (name, labels [H,W] int32): random disks,
    single pixels with five labels, and one label in two far-apart pieces."""
    H, W = shape
    rng = np.random.default_rng(seed)
    d = disks(shape, max(2, H * W // 600), seed)
    px = np.zeros(shape, np.int32)
    k = max(1, H * W // 7)
    px.reshape(-1)[rng.choice(H * W, k, replace=False)] = rng.integers(1, 6, k)
    two = np.zeros(shape, np.int32)
    two[: max(1, H // 5), : max(1, W // 5)] = 3
    two[H - max(1, H // 5):, W - max(1, W // 5):] = 3
    return [("disks", d), ("pixels", px), ("two pieces", two)]


def noise(shape, channels, dtype, seed, base=0, spread=None):
    """A uniform noise image [..., channels] of dtype: base + U[0, spread), spread by default the whole range."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max + 1
    spread = top - base if spread is None else spread
    return (base + rng.integers(0, spread, tuple(shape) + (channels,))).astype(dtype)
