"""Per-object Haralick texture on the device (cs_label_texture, include/cellscreen.h): the grey-level co-occurrence
matrix of every object and the 13 features of Haralick, Shanmugam and Dinstein (1973) taken from it -- mahotas.features.haralick,
scikit-image's graycomatrix / graycoprops, CellProfiler's MeasureTexture.

    t = TextureMeasurer().measure_batch(image, labels, distance=3, levels=32)
    t.mean[:, 0, t.FEATURE_NAMES.index("contrast")]    # channel 0, the mean over the directions
    ring = TextureMeasurer().measure_batch(image, grown, exclude=nuclei)

The objects are IntensityMeasurer's: the pixels of one image with one label > 0, connected or not, less the pixels where
`exclude` is non-zero.  Per channel a value becomes a level q(v) = ((min(max(v, lo), hi) - lo) * levels) // (hi - lo + 1); the
pairs of one distance d in the four directions (0, d), (d, d), (d, 0), (d, -d) (row, column; mahotas' 2-D order) count when both
pixels belong to the object, each once in G[q][q'] and once in G[q'][q].  The device returns integers -- the three marginals of
G, the sum of its squares -- and one float64, clogc = sum G log2 G; the features follow here in float64.  With p = G / N, logs
to base 2, mu and var the mean and variance of the row marginal px, ps and pd the marginals of i + j and |i - j|:

     0 angular second moment   sum p^2                          7 sum entropy             H(ps)
     1 contrast                sum k^2 pd[k]                    8 entropy                 HXY = log2 N - clogc / N
     2 correlation             (sum ij p - mu^2) / var, or 1    9 difference variance     the variance of k under pd
     3 variance                var                             10 difference entropy      H(pd)
     4 inverse diff. moment    sum pd[k] / (1 + k^2)           11 info. measure 1         (HXY - 2 HX) / HX, or HXY - 2 HX
     5 sum average             sum k ps[k]                     12 info. measure 2         sqrt(max(0, 1 - exp(-2 (2 HX - HXY))))
     6 sum variance            sum (k - sum average)^2 ps[k]

G is symmetric, so py = px and HXY1 = HXY2 = 2 HX.  HXY is held to HX <= HXY <= 2 HX, which every joint entropy obeys, so that
the rounding of clogc cannot push a flat object's entropy below zero.  A direction without pairs gives NaN in all 13.

One distance per call, at most 64 levels, symmetric matrices, 2-D, no per-object automatic range, no 14th feature (the maximal
correlation coefficient), no Gabor or granularity measures."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import ClassVar, Tuple

import numpy as np

from . import _lib as L
from ._labels import MAX_LABEL, LabelTool
from .intensity import IntensityMeasurer
from .preprocess import PIX_U8

MIN_LEVELS, MAX_LEVELS = 2, 64
MAX_DISTANCE = 127
MAX_VALUE = 65535
MAX_CELLS = 1 << 24                     # batch * max_label * channels * levels, and * levels^2 with glcm
DIRECTIONS = ((0, 1), (1, 1), (1, 0), (1, -1))          # (row, column) steps in units of the distance
FEATURE_NAMES = ("angular_second_moment", "contrast", "correlation", "variance", "inverse_difference_moment", "sum_average",
                 "sum_variance", "sum_entropy", "entropy", "difference_variance", "difference_entropy", "info_measure_1",
                 "info_measure_2")


def _entropy(x, n):
    """H of the integer marginal x [..., K] with total n [...] > 0, base 2"""
    p = x / n[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(x > 0, p * np.log2(p), 0.0)
    return -t.sum(axis=-1)


def texture_features(marg, sumsq, clogc, levels) -> np.ndarray:
    """features [..., 13] float64 of the records marg [..., 4 * levels] (px, ps with its padding, pd), sumsq [...] and
    clogc [...]; NaN where the matrix is empty.  The integer moments are taken in int64, where all of them fit."""
    Lv = int(levels)
    marg = np.asarray(marg).astype(np.int64)
    sumsq = np.asarray(sumsq).astype(np.int64)
    clogc = np.asarray(clogc, np.float64)
    if marg.shape[-1] != 4 * Lv or marg.shape[:-1] != sumsq.shape or sumsq.shape != clogc.shape:
        raise ValueError(f"marg {marg.shape}, sumsq {sumsq.shape} and clogc {clogc.shape}: [..., {4 * Lv}], [...] and [...] expected")
    px, ps, pd = marg[..., :Lv], marg[..., Lv:3 * Lv], marg[..., 3 * Lv:]
    N = px.sum(axis=-1)
    has = N > 0
    n = np.where(has, N, 1)                             # the empty ones are NaN at the end
    nf = n.astype(np.float64)
    i, k2 = np.arange(Lv, dtype=np.int64), np.arange(2 * Lv, dtype=np.int64)
    s1, s2 = (i * px).sum(axis=-1), (i * i * px).sum(axis=-1)       # below 2^31 and 2^37
    d1, d2 = (i * pd).sum(axis=-1), (i * i * pd).sum(axis=-1)
    var_num = s2 * n - s1 * s1                          # N^2 var, below 2^60
    f = np.empty(marg.shape[:-1] + (13,), np.float64)
    f[..., 0] = sumsq / (nf * nf)
    f[..., 1] = d2 / nf
    # sum ij p - mu^2 = (2 var_num - d2 N) / (2 N^2), since sum ij p = (2 sum i^2 px - sum k^2 pd) / (2 N)
    with np.errstate(divide="ignore", invalid="ignore"):
        f[..., 2] = np.where(var_num > 0, (2 * var_num - d2 * n) / (2.0 * var_num), 1.0)
    f[..., 3] = var_num / (nf * nf)
    f[..., 4] = (pd / (1.0 + i * i)).sum(axis=-1) / nf
    sa = (k2 * ps).sum(axis=-1) / nf
    f[..., 5] = sa
    f[..., 6] = ((k2 - sa[..., None]) ** 2 * ps).sum(axis=-1) / nf
    f[..., 7] = _entropy(ps, nf)
    hx = _entropy(px, nf)
    hxy = np.clip(np.log2(nf) - clogc / nf, hx, 2.0 * hx)
    f[..., 8] = hxy
    f[..., 9] = (d2 * n - d1 * d1) / (nf * nf)
    f[..., 10] = _entropy(pd, nf)
    with np.errstate(divide="ignore", invalid="ignore"):
        f[..., 11] = np.where(hx > 0, (hxy - 2.0 * hx) / hx, hxy - 2.0 * hx)
    f[..., 12] = np.sqrt(np.maximum(0.0, 1.0 - np.exp(-2.0 * (2.0 * hx - hxy))))
    f[~has] = np.nan
    return f


@dataclass
class TextureTable:
    """The objects present in a batch, in (image, label) order; n objects, C channels, the 4 directions of DIRECTIONS.  All numpy
    arrays on the host."""
    FEATURE_NAMES: ClassVar[Tuple[str, ...]] = FEATURE_NAMES
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    count: np.ndarray                   # [n] int32: pixels
    levels: int
    pairs: np.ndarray                   # [n,C,4] int64: the pixel pairs of a direction, N / 2
    features: np.ndarray                # [n,C,4,13] float64, NaN in a direction without pairs
    mean: np.ndarray                    # [n,C,13] float64: the mean over the directions that have pairs (mahotas' return_mean)

    def __len__(self):
        return int(self.label.shape[0])


def texture_table(count, marg, sumsq, clogc, levels) -> TextureTable:
    """The table of the dense records cs_label_texture writes: count [B,max_label] int32, marg [B,max_label,C,4,4 * levels]
    int32, sumsq [B,max_label,C,4] int64 and clogc [B,max_label,C,4] float64.  The rows of absent objects (count 0) are dropped."""
    count, marg, sumsq, clogc = np.asarray(count), np.asarray(marg), np.asarray(sumsq), np.asarray(clogc)
    levels = _check_levels(levels)
    if count.dtype != np.int32 or marg.dtype != np.int32 or sumsq.dtype != np.int64 or clogc.dtype != np.float64:
        raise TypeError("count and marg must be int32, sumsq int64 and clogc float64")
    if (count.ndim != 2 or marg.ndim != 5 or marg.shape[:2] != count.shape or marg.shape[3:] != (4, 4 * levels)
            or sumsq.shape != marg.shape[:4] or clogc.shape != marg.shape[:4]):
        raise ValueError(f"count {count.shape}, marg {marg.shape}, sumsq {sumsq.shape}, clogc {clogc.shape}: [B,max_label], "
                         f"[B,max_label,C,4,{4 * levels}] and twice [B,max_label,C,4] expected")
    img, row = np.nonzero(count > 0)
    m = marg[img, row]                                  # [n,C,4,4L]
    feats = texture_features(m, sumsq[img, row], clogc[img, row], levels)
    pairs = m[..., :levels].astype(np.int64).sum(axis=-1) // 2
    has = pairs > 0
    k = has.sum(axis=2)                                 # [n,C]: the directions with pairs
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(has[..., None], feats, 0.0).sum(axis=2) / np.where(k > 0, k, np.nan)[..., None]
    return TextureTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), count=count[img, row].copy(), levels=levels,
                        pairs=pairs, features=feats, mean=mean)


def _check_int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
    if not lo <= int(v) <= hi:
        raise ValueError(f"{name} {int(v)}: must lie in {lo}..{hi}")
    return int(v)


def _check_levels(levels):
    return _check_int("levels", levels, MIN_LEVELS, MAX_LEVELS)


def as_ranges(value_range, channels, top) -> np.ndarray:
    """[channels, 2] int32 (lo, hi) of value_range: None (0..top, the dtype's full range), one (lo, hi) pair for every channel,
    or a sequence of `channels` pairs; integers with 0 <= lo <= hi <= 65535."""
    if value_range is None:
        return np.tile(np.array([[0, top]], np.int32), (channels, 1))
    if isinstance(value_range, (str, bytes)) or not hasattr(value_range, "__iter__"):
        raise TypeError("value_range must be None, a (lo, hi) pair or a sequence of pairs")
    v = list(value_range)
    if len(v) == 2 and not any(hasattr(x, "__len__") for x in v):     # two scalars: one pair for every channel
        v = [tuple(v)] * channels
    if len(v) != channels:
        raise ValueError(f"{len(v)} value ranges for {channels} channels")
    out = np.empty((channels, 2), np.int32)
    for c, pair in enumerate(v):
        if isinstance(pair, (str, bytes)) or not hasattr(pair, "__len__") or len(pair) != 2:
            raise TypeError(f"value range {pair!r}: a (lo, hi) pair expected")
        if any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in pair):
            raise TypeError(f"value range {pair!r}: lo and hi must be integers")
        lo, hi = int(pair[0]), int(pair[1])
        if not 0 <= lo <= hi <= MAX_VALUE:
            raise ValueError(f"value range {lo}..{hi} of channel {c}: 0 <= lo <= hi <= {MAX_VALUE} is required")
        out[c] = lo, hi
    return out


class TextureMeasurer(LabelTool):
    """cs_label_texture on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read
    in stream order."""
    _noun = "the measurer"
    FEATURE_NAMES = FEATURE_NAMES

    # the planes are IntensityMeasurer's, with its rules, messages and order; distance, levels and the ranges follow, then the sizes
    def _check(self, image, labels, distance, levels, value_range, exclude, max_label, glcm):
        B, H, W, nc, ptype, on_dev = IntensityMeasurer._check(self, image, labels, exclude, None)
        distance = _check_int("distance", distance, 1, MAX_DISTANCE)
        levels = _check_levels(levels)
        ranges = as_ranges(value_range, nc, 255 if ptype == PIX_U8 else MAX_VALUE)
        if max_label is not None:
            if isinstance(max_label, (bool, np.bool_)) or not isinstance(max_label, (int, np.integer)):
                raise TypeError(f"max_label must be an integer or None, got {type(max_label).__name__}")
            self._check_size(B, int(max_label), nc, levels, glcm)
        return B, H, W, nc, ptype, on_dev, distance, levels, ranges

    @staticmethod
    def _check_size(B, max_label, nc, levels, glcm):
        if max_label < 1:
            raise ValueError(f"max_label {max_label}: must be >= 1")
        if max_label > MAX_LABEL:
            raise ValueError(f"max_label {max_label} above {MAX_LABEL}: relabel sparse ids first")
        if B * max_label * nc * levels > MAX_CELLS:
            raise ValueError(f"batch {B} x max_label {max_label} x channels {nc} x levels {levels} above {MAX_CELLS}: "
                             "measure fewer images or levels per call")
        if glcm and B * max_label * nc * levels * levels > MAX_CELLS:
            raise ValueError(f"batch {B} x max_label {max_label} x channels {nc} x levels {levels}^2 above {MAX_CELLS}: "
                             "the matrices of fewer images or levels per call, or glcm=False")

    def measure_dense(self, image, labels, distance=1, levels=32, value_range=None, exclude=None, max_label=None, glcm=False):
        """The dense records as the device writes them, numpy on the host: count int32 [B,max_label], marg int32
        [B,max_label,C,4,4 * levels] (px, ps and a zero, pd), sumsq int64 [B,max_label,C,4], clogc float64 [B,max_label,C,4] and
        the matrices int32 [B,max_label,C,4,levels,levels] (None without glcm=True), row label - 1 for a label; the rows of an
        absent object are all zero.  Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev, distance, levels, ranges = self._check(image, labels, distance, levels, value_range, exclude,
                                                                           max_label, glcm)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc, levels, glcm)
        max_label = int(max_label)
        lo, hi = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
        count = np.empty((B, max_label), np.int32)
        marg = np.empty((B, max_label, nc, 4, 4 * levels), np.int32)
        sumsq = np.empty((B, max_label, nc, 4), np.int64)
        clogc = np.empty((B, max_label, nc, 4), np.float64)
        mats = np.empty((B, max_label, nc, 4, levels, levels), np.int32) if glcm else None
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_texture(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                           max_label, levels, distance, L._ptr(lo), L._ptr(hi), L._ptr(count), L._ptr(marg),
                                           L._ptr(sumsq), L._ptr(clogc), L._ptr(mats), L.CS_MEM_HOST))
        return count, marg, sumsq, clogc, mats

    def measure_batch(self, image, labels, distance=1, levels=32, value_range=None, exclude=None, max_label=None) -> TextureTable:
        """image, labels, exclude, max_label: as IntensityMeasurer.measure_batch.  distance: 1..127 pixels between the two ends
        of a pair.  levels: 2..64 grey levels.  value_range: what the levels divide, None (the dtype's full range), one (lo, hi)
        pair or one per channel; values outside are clipped to it.  Returns the TextureTable of the objects present, in
        (image, label) order.  A negative label, or one above max_label, raises CellScreenError (CS_ERR_INVALID); the measurer
        stays usable."""
        count, marg, sumsq, clogc, _ = self.measure_dense(image, labels, distance, levels, value_range, exclude, max_label)
        return texture_table(count, marg, sumsq, clogc, levels)

    def last_timing(self):
        """Device milliseconds of the last measure_batch: texture_boxes_ms (clearing, the counts and bounding boxes) and
        texture_matrices_ms (the matrices and their reduction to the records)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.cs_label_texture_last_timing(self._handle, C.byref(a), C.byref(b)))
        return dict(texture_boxes_ms=a.value, texture_matrices_ms=b.value)
