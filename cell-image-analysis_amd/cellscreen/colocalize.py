"""Per-object colocalization between channels on the device (cs_label_colocalize, include/cellscreen.h): whether
two stains go together inside every object of a label image -- CellProfiler's MeasureColocalization, scipy.stats.pearsonr and
linregress per object.  The rule is this project's (tests/colocalize_reference.py restates it); it corresponds to those
measurements without a promise of bit equality with CellProfiler.

    t = ColocalizationMeasurer().measure_batch(image, labels)               # image [B,H,W,C], C = 2..4
    t.pairs                                                                 # [(0, 1), (0, 2), (1, 2)] at C = 3
    t.pearson[:, 0], t.manders1[:, 0]                                       # of every object, channels 0 and 1

An object is IntensityMeasurer's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  A pixel is "above" in channel c iff v * den >= num * max_c (threshold=(num, den), by default 15 / 100 of the
object's own maximum in c; a tie is above), or iff v >= t_c (absolute=[t_0, ..]); "both" of a pair (i, j), i < j: above in both.
With rwc, the dense rank of a value among the values on the object pixels of its image and channel, R = max(R_i, R_j) of the
numbers of distinct values, and w = R - |rank_i - rank_j|.  The device returns exact integer sums; the floats are taken from them
here in Python ints, so they do not depend on a summation order (n * sum v_i v_j reaches 2^80: no int64 arithmetic):

    pearson  = (n S_ij - S_i S_j) / sqrt(d_i d_j)       d_x = n S_xx - S_x^2          slope = (n S_ij - S_i S_j) / d_i
    overlap  = B_ij / sqrt(B_ii B_jj)     k1 = B_ij / B_ii     k2 = B_ij / B_jj       (B: over the pixels above in both)
    manders1 = B_i / A_i     manders2 = B_j / A_j                                      (A_c: sum v over the pixels above in c)
    rwc1     = sum v_i w [both] / (R A_i)     rwc2 likewise

NaN where a denominator is 0.  A quotient of two integers is correctly rounded; the two with a root take the product to float64,
its root, and one division: within 4 * 2^-53 relative of the exact value.  No Costes threshold, no per-object ranks,
2-D only, 2 to 4 channels and one threshold rule per call."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import List, Tuple

import numpy as np

from . import _lib as L
from ._labels import LabelTool
from .intensity import MAX_CHANNELS, IntensityMeasurer

MAX_DENOMINATOR = 65536
MAX_SCRATCH = 1 << 30
SCRATCH_PER_PLANE = 3 * 65536           # bytes per image and channel: presence + uint16 ranks
FIELDS = ("pearson", "slope", "overlap", "k1", "k2", "manders1", "manders2", "rwc1", "rwc2")


def pairs_of(channels: int) -> List[Tuple[int, int]]:
    """The pairs (i, j), i < j, in the order of the tables."""
    return [(i, j) for i in range(channels) for j in range(i + 1, channels)]


def as_threshold(threshold) -> Tuple[int, int]:
    """(num, den) of the fraction of an object's maximum: a (num, den) pair of integers with 0 <= num <= den, den in 1..65536,
    taken as it is (not reduced); a fractions.Fraction; or a float in [0, 1], which becomes
    Fraction(x).limit_denominator(65536), so that 0.15 comes out as 3/20."""
    if isinstance(threshold, (bool, np.bool_)):
        raise TypeError("threshold must be a float, a Fraction or a (num, den) pair, got a bool")
    if isinstance(threshold, (tuple, list)):
        if len(threshold) != 2 or any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in threshold):
            raise TypeError(f"a threshold pair must be (num, den) integers, got {threshold!r}")
        num, den = int(threshold[0]), int(threshold[1])
    elif isinstance(threshold, Fraction):
        num, den = threshold.numerator, threshold.denominator
    elif isinstance(threshold, (int, np.integer)):
        num, den = int(threshold), 1
    elif isinstance(threshold, (float, np.floating)):
        x = float(threshold)
        if math.isnan(x) or not 0.0 <= x <= 1.0:
            raise ValueError(f"threshold {threshold!r}: must lie in [0, 1]")
        f = Fraction(x).limit_denominator(MAX_DENOMINATOR)
        num, den = f.numerator, f.denominator
    else:
        raise TypeError(f"threshold must be a float, a Fraction or a (num, den) pair, got {type(threshold).__name__}")
    if den < 1 or den > MAX_DENOMINATOR:
        raise ValueError(f"threshold {num}/{den}: the denominator must be in 1..{MAX_DENOMINATOR}")
    if not 0 <= num <= den:
        raise ValueError(f"threshold {num}/{den}: must lie in [0, 1]")
    return num, den


def colocalize_params(channels: int, threshold=(15, 100), absolute=None, rwc=True) -> "L.CSColocalizeParams":
    """cs_colocalize_params of a call's rule; absolute: None, or one threshold in 0..65536 per channel, which replaces `threshold`."""
    p = L.CSColocalizeParams()
    if isinstance(rwc, (bool, np.bool_)):
        p.rwc = 1 if rwc else 0
    else:
        raise TypeError(f"rwc must be a bool, got {type(rwc).__name__}")
    if absolute is None:
        p.thr_num, p.thr_den = as_threshold(threshold)
        return p
    if isinstance(absolute, (str, bytes)) or not hasattr(absolute, "__len__"):
        raise TypeError("absolute must be a sequence of integers, one per channel")
    if any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in absolute):
        raise TypeError(f"absolute must hold integers, got {absolute!r}")
    if len(absolute) != channels:
        raise ValueError(f"absolute holds {len(absolute)} thresholds for {channels} channels")
    if any(not 0 <= int(x) <= 65536 for x in absolute):
        raise ValueError(f"absolute {list(absolute)!r}: every threshold must be in 0..65536")
    p.absolute = 1
    for c, x in enumerate(absolute):
        p.abs_thr[c] = int(x)
    return p


@dataclass
class ColocalizationTable:
    """The objects present in a batch, in (image, label) order; n objects, C channels, P pairs.  All numpy arrays on the host.
    The floats are NaN where a denominator is 0; rwc1 and rwc2 are NaN throughout without rwc."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    pairs: List[Tuple[int, int]]        # the P pairs (i, j), i < j
    pearson: np.ndarray                 # [n,P] float64, over all pixels of the object
    slope: np.ndarray                   # [n,P]: the least-squares slope of channel j on channel i
    overlap: np.ndarray                 # [n,P], over the pixels above in both
    k1: np.ndarray                      # [n,P]
    k2: np.ndarray                      # [n,P]
    manders1: np.ndarray                # [n,P]
    manders2: np.ndarray                # [n,P]
    rwc1: np.ndarray                    # [n,P]
    rwc2: np.ndarray                    # [n,P]
    geom: np.ndarray                    # [n,3] int64: area, sum r, sum c
    chan: np.ndarray                    # [n,C,5] int64: sum v, sum v^2, max, n_above, sum v[above]
    pair: np.ndarray                    # [n,P,9] int64: sum v_i v_j; over both: n, sum v_i, v_j, v_i^2, v_j^2, v_i v_j, v_i w, v_j w
    levels: np.ndarray                  # [B,C] int32: the distinct values per image and channel, zeros without rwc

    def __len__(self):
        return int(self.label.shape[0])


def _ratio(a: int, b: int) -> float:
    return a / b if b != 0 else math.nan                # Python ints: correctly rounded


def _over_root(a: int, b: int) -> float:
    return a / math.sqrt(b) if b != 0 else math.nan     # b to float64, its root, a to float64, one division


def colocalization_table(geom, chan, pair, levels, rwc=True) -> ColocalizationTable:
    """The table of the dense tables cs_label_colocalize writes: geom [B,max_label,3], chan [B,max_label,C,5], pair
    [B,max_label,P,9] int64 and levels [B,C] int32.  The rows of absent objects (area 0) are dropped."""
    geom, chan, pair, levels = np.asarray(geom), np.asarray(chan), np.asarray(pair), np.asarray(levels)
    if geom.dtype != np.int64 or chan.dtype != np.int64 or pair.dtype != np.int64 or levels.dtype != np.int32:
        raise TypeError("geom, chan and pair must be int64, levels int32")
    nc = chan.shape[2] if chan.ndim == 4 else 0
    pp = pairs_of(nc)
    if (geom.ndim != 3 or geom.shape[2] != 3 or chan.ndim != 4 or chan.shape[3] != 5 or not 2 <= nc <= MAX_CHANNELS or
            pair.shape != geom.shape[:2] + (len(pp), 9) or chan.shape[:2] != geom.shape[:2] or levels.shape != (geom.shape[0], nc)):
        raise ValueError(f"geom {geom.shape}, chan {chan.shape}, pair {pair.shape}, levels {levels.shape}: [B,max_label,3], "
                         "[B,max_label,C,5], [B,max_label,P,9] and [B,C] expected")
    img, row = np.nonzero(geom[:, :, 0] > 0)
    g, c, q = geom[img, row], chan[img, row], pair[img, row]
    n = g.shape[0]
    out = {f: np.full((n, len(pp)), np.nan) for f in FIELDS}
    for k in range(n):
        a = int(g[k, 0])
        ch = [[int(x) for x in c[k, i]] for i in range(nc)]
        for p, (i, j) in enumerate(pp):
            si, si2, _, _, ai = ch[i]
            sj, sj2, _, _, aj = ch[j]
            sij, _, bi, bj, bii, bjj, bij, biw, bjw = (int(x) for x in q[k, p])
            cov = a * sij - si * sj
            di, dj = a * si2 - si * si, a * sj2 - sj * sj
            out["pearson"][k, p] = _over_root(cov, di * dj)
            out["slope"][k, p] = _ratio(cov, di)
            out["overlap"][k, p] = _over_root(bij, bii * bjj)
            out["k1"][k, p] = _ratio(bij, bii)
            out["k2"][k, p] = _ratio(bij, bjj)
            out["manders1"][k, p] = _ratio(bi, ai)
            out["manders2"][k, p] = _ratio(bj, aj)
            if rwc:
                R = max(int(levels[img[k], i]), int(levels[img[k], j]))
                out["rwc1"][k, p] = _ratio(biw, R * ai)
                out["rwc2"][k, p] = _ratio(bjw, R * aj)
    return ColocalizationTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), area=g[:, 0].copy(), pairs=pp, geom=g, chan=c,
                               pair=q, levels=levels.copy(), **out)


class ColocalizationMeasurer(LabelTool):
    """cs_label_colocalize on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read
    in stream order.  The argument checks of the planes are IntensityMeasurer's, in its order."""
    _noun = "the measurer"
    _check = IntensityMeasurer._check
    _check_size = staticmethod(IntensityMeasurer._check_size)

    def _check_rule(self, image, labels, exclude, max_label, threshold, absolute, rwc):
        B, H, W, nc, ptype, on_dev = self._check(image, labels, exclude, max_label)
        if image.ndim != 4 or nc < 2:
            raise ValueError(f"image must be [B,H,W,C] with 2 to {MAX_CHANNELS} channels, got shape {tuple(image.shape)}")
        prm = colocalize_params(nc, threshold, absolute, rwc)
        if prm.rwc and B * nc * SCRATCH_PER_PLANE > MAX_SCRATCH:
            raise ValueError(f"batch {B} x channels {nc}: the rank tables would exceed {MAX_SCRATCH} bytes, split the batch")
        return B, H, W, nc, ptype, on_dev, prm

    def measure_dense(self, image, labels, exclude=None, max_label=None, threshold=(15, 100), absolute=None, rwc=True):
        """The dense tables as the device writes them, numpy on the host: geom int64 [B,max_label,3], chan int64
        [B,max_label,C,5], pair int64 [B,max_label,P,9] and levels int32 [B,C] (ColocalizationTable names the fields), row
        label - 1 for a label; the rows of an absent object are all zero.  Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev, prm = self._check_rule(image, labels, exclude, max_label, threshold, absolute, rwc)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc)
        max_label = int(max_label)
        npairs = nc * (nc - 1) // 2
        geom = np.empty((B, max_label, 3), np.int64)
        chan = np.empty((B, max_label, nc, 5), np.int64)
        pair = np.empty((B, max_label, npairs, 9), np.int64)
        levels = np.empty((B, nc), np.int32)
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_colocalize(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                              max_label, C.byref(prm), L._ptr(geom), L._ptr(chan), L._ptr(pair), L._ptr(levels),
                                              L.CS_MEM_HOST))
        return geom, chan, pair, levels

    def measure_batch(self, image, labels, exclude=None, max_label=None, threshold=(15, 100), absolute=None, rwc=True) -> ColocalizationTable:
        """image: [B,H,W,C] uint8 / uint16 with C = 2..4, every pair of channels is measured; labels, exclude, max_label: as
        IntensityMeasurer.measure_batch.  threshold: the fraction of an object's own maximum at and above which a pixel counts
        in a channel, a (num, den) pair, a Fraction or a float (as_threshold); absolute: None, or one threshold per channel in
        0..65536 that replaces it.  rwc: also the rank-weighted coefficients.  Returns the ColocalizationTable of the objects
        present, in (image, label) order.  A negative label, or one above max_label, raises CellScreenError (CS_ERR_INVALID);
        the measurer stays usable."""
        return colocalization_table(*self.measure_dense(image, labels, exclude, max_label, threshold, absolute, rwc), rwc=bool(rwc))

    def last_timing(self):
        """Device milliseconds of the last measure_batch: colocalize_clear_ms, colocalize_moments_ms, colocalize_ranks_ms (0
        without rwc) and colocalize_thresholded_ms."""
        v = [C.c_double() for _ in range(4)]
        L.check(self._lib.cs_label_colocalize_last_timing(self._handle, *(C.byref(x) for x in v)))
        return dict(zip(("colocalize_clear_ms", "colocalize_moments_ms", "colocalize_ranks_ms", "colocalize_thresholded_ms"), (x.value for x in v)))
