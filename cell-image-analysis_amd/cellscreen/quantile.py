"""Per-object median, quantiles and MAD on the device (cs_label_quantiles, include/cellscreen.h): the robust half of
the per-object measurement -- scipy.ndimage.median over labels, numpy.quantile per object, scipy.stats.median_abs_deviation,
CellProfiler's MedianIntensity / MADIntensity / LowerQuartileIntensity / UpperQuartileIntensity.

    t = QuantileMeasurer().measure_batch(image, labels, quantiles=(0.25, 0.5, 0.75), mad=True)
    ring = QuantileMeasurer().measure_batch(image, grown, quantiles=(0.5,), exclude=nuclei)
    t.value[:, 0, 1] / ring.value[:, 0, 0]            # a nuclear / cytoplasmic ratio on medians, where both hold the same objects

The objects are IntensityMeasurer's: the pixels of one image with one label > 0, connected or not, less the pixels where
`exclude` is non-zero.  A quantile is a fraction num / den with 0 <= num <= den <= 65536.  For an object of n pixels whose
values in a channel, sorted, are s[0 .. n-1]:

    t = num * (n - 1);  lo = t // den;  rem = t % den;  hi = lo + (rem > 0)

The device returns the integers s[lo] (`lower`, numpy's method="lower") and s[hi] (`upper`, "higher"); `value` is
s[lo] + (s[hi] - s[lo]) * rem / den in float64, numpy's "linear".  With mad=True it also returns the median's two order
statistics m_lo, m_hi and those of the doubled deviations d = |2 v - (m_lo + m_hi)| at the same ranks, d_lo, d_hi:
median = (m_lo + m_hi) / 2 and mad = (d_lo + d_hi) / 4, both exact, no scale factor (scipy's scale=1).

2-D only, at most 4 channels and 8 quantiles per call, no weighted quantiles, no mode."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np

from . import _lib as L
from ._labels import MAX_LABEL, LabelTool
from .intensity import IntensityMeasurer

MAX_QUANTILES = 8
MAX_DENOMINATOR = 65536
MAX_CELLS = 1 << 22                     # batch * max_label * channels * quantiles


def as_fraction(q) -> Fraction:
    """A quantile as the fraction the device works with.  q: a float (or an integer 0 or 1), which becomes
    Fraction(q).limit_denominator(65536), so that 0.01, 0.95 and 1 / 3 come out as 1/100, 19/20 and 1/3; a fractions.Fraction;
    or a (num, den) pair of integers.  NaN, values outside [0, 1] and denominators above 65536 are refused."""
    if isinstance(q, (bool, np.bool_)):
        raise TypeError("a quantile must be a float, a Fraction or a (num, den) pair, got a bool")
    if isinstance(q, Fraction):
        f = q
    elif isinstance(q, (tuple, list)):
        if len(q) != 2 or any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in q):
            raise TypeError(f"a quantile pair must be (num, den) integers, got {q!r}")
        num, den = int(q[0]), int(q[1])
        if den < 1:
            raise ValueError(f"quantile {num}/{den}: the denominator must be >= 1")
        f = Fraction(num, den)
    elif isinstance(q, (int, np.integer)):
        f = Fraction(int(q))
    elif isinstance(q, (float, np.floating)):
        x = float(q)
        if math.isnan(x) or not 0.0 <= x <= 1.0:
            raise ValueError(f"quantile {q!r}: must lie in [0, 1]")
        f = Fraction(x).limit_denominator(MAX_DENOMINATOR)
    else:
        raise TypeError(f"a quantile must be a float, a Fraction or a (num, den) pair, got {type(q).__name__}")
    if not 0 <= f <= 1:
        raise ValueError(f"quantile {q!r}: must lie in [0, 1]")
    if f.denominator > MAX_DENOMINATOR:
        raise ValueError(f"quantile {q!r}: denominators above {MAX_DENOMINATOR} are not supported")
    return f


def as_fractions(quantiles) -> Tuple[Fraction, ...]:
    """The list of a call: 1 to 8 quantiles; duplicates and any order are allowed and kept."""
    if isinstance(quantiles, (str, bytes)) or not hasattr(quantiles, "__iter__"):
        raise TypeError("quantiles must be a sequence of floats, Fractions or (num, den) pairs")
    out = tuple(as_fraction(q) for q in quantiles)
    if not out:
        raise ValueError("quantiles is empty")
    if len(out) > MAX_QUANTILES:
        raise ValueError(f"{len(out)} quantiles: at most {MAX_QUANTILES} per call")
    return out


@dataclass
class QuantileTable:
    """The objects present in a batch, in (image, label) order; n objects, C channels, K quantiles.  All numpy arrays on the host."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    count: np.ndarray                   # [n] int32: pixels
    fractions: Tuple[Fraction, ...]     # the K quantiles
    lower: np.ndarray                   # [n,C,K] int32: s[lo]
    upper: np.ndarray                   # [n,C,K] int32: s[hi]
    value: np.ndarray                   # [n,C,K] float64: numpy's linear interpolation between them
    median: Optional[np.ndarray] = None     # [n,C] float64, with mad=True
    mad: Optional[np.ndarray] = None        # [n,C] float64, with mad=True
    mad_raw: Optional[np.ndarray] = None    # [n,C,4] int32: m_lo, m_hi, d_lo, d_hi, with mad=True

    def __len__(self):
        return int(self.label.shape[0])


def quantile_table(count: np.ndarray, order: np.ndarray, mad: Optional[np.ndarray], fractions) -> QuantileTable:
    """The table of the dense tables cs_label_quantiles writes: count [B,max_label], order [B,max_label,C,K,2] and mad (None or
    [B,max_label,C,4]), int32; fractions: the K quantiles.  The rows of absent objects (count 0) are dropped."""
    count, order = np.asarray(count), np.asarray(order)
    fractions = as_fractions(fractions)
    if count.dtype != np.int32 or order.dtype != np.int32 or (mad is not None and np.asarray(mad).dtype != np.int32):
        raise TypeError("count, order and mad must be int32")
    if count.ndim != 2 or order.ndim != 5 or order.shape[:2] != count.shape or order.shape[3:] != (len(fractions), 2):
        raise ValueError(f"count {count.shape} and order {order.shape}: [B,max_label] and [B,max_label,C,{len(fractions)},2] expected")
    if mad is not None:
        mad = np.asarray(mad)
        if mad.shape != order.shape[:3] + (4,):
            raise ValueError(f"mad {mad.shape}: {order.shape[:3] + (4,)} expected")
    img, row = np.nonzero(count > 0)
    n = count[img, row]
    o = order[img, row]                                 # [n,C,K,2]
    lower, upper = o[..., 0].copy(), o[..., 1].copy()
    num = np.array([f.numerator for f in fractions], np.int64)
    den = np.array([f.denominator for f in fractions], np.int64)
    rem = (num[None, :] * (n.astype(np.int64)[:, None] - 1)) % den[None, :]         # [n,K], below 2^16
    value = lower + (upper - lower).astype(np.float64) * rem[:, None, :] / den[None, None, :]
    t = QuantileTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), count=n.copy(), fractions=fractions, lower=lower,
                      upper=upper, value=value)
    if mad is not None:
        m = mad[img, row]                               # [n,C,4]
        t.mad_raw = m.copy()
        t.median = (m[..., 0] + m[..., 1]) / 2.0
        t.mad = (m[..., 2] + m[..., 3]) / 4.0
    return t


class QuantileMeasurer(LabelTool):
    """cs_label_quantiles on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read
    in stream order."""
    _noun = "the measurer"

    # the planes are IntensityMeasurer's, with its rules, messages and order; the quantiles follow, then the sizes
    def _check(self, image, labels, quantiles, exclude, max_label):
        B, H, W, nc, ptype, on_dev = IntensityMeasurer._check(self, image, labels, exclude, None)
        fr = as_fractions(quantiles)
        if max_label is not None:
            if isinstance(max_label, (bool, np.bool_)) or not isinstance(max_label, (int, np.integer)):
                raise TypeError(f"max_label must be an integer or None, got {type(max_label).__name__}")
            self._check_size(B, int(max_label), nc, len(fr))
        return B, H, W, nc, ptype, on_dev, fr

    @staticmethod
    def _check_size(B, max_label, nc, nq):
        if max_label < 1:
            raise ValueError(f"max_label {max_label}: must be >= 1")
        if max_label > MAX_LABEL:
            raise ValueError(f"max_label {max_label} above {MAX_LABEL}: relabel sparse ids first")
        if B * max_label * nc * nq > MAX_CELLS:
            raise ValueError(f"batch {B} x max_label {max_label} x channels {nc} x quantiles {nq} above {MAX_CELLS}: "
                             "measure fewer images or quantiles per call")

    def measure_dense(self, image, labels, quantiles=(0.25, 0.5, 0.75), mad=False, exclude=None, max_label=None):
        """The dense tables as the device writes them, numpy int32 on the host: count [B,max_label], order [B,max_label,C,K,2]
        (s[lo], s[hi]) and mad ([B,max_label,C,4]: m_lo, m_hi, d_lo, d_hi; None without mad=True), row label - 1 for a label;
        the rows of an absent object are all zero.  Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev, fr = self._check(image, labels, quantiles, exclude, max_label)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc, len(fr))
        max_label, nq = int(max_label), len(fr)
        q_num = np.array([f.numerator for f in fr], np.int32)
        q_den = np.array([f.denominator for f in fr], np.int32)
        count = np.empty((B, max_label), np.int32)
        order = np.empty((B, max_label, nc, nq, 2), np.int32)
        mad_t = np.empty((B, max_label, nc, 4), np.int32) if mad else None
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_quantiles(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                             max_label, L._ptr(q_num), L._ptr(q_den), nq, 1 if mad else 0, L._ptr(count),
                                             L._ptr(order), L._ptr(mad_t), L.CS_MEM_HOST))
        return count, order, mad_t

    def measure_batch(self, image, labels, quantiles=(0.25, 0.5, 0.75), mad=False, exclude=None, max_label=None) -> QuantileTable:
        """image, labels, exclude, max_label: as IntensityMeasurer.measure_batch.  quantiles: 1 to 8 floats, Fractions or
        (num, den) pairs (as_fraction), kept in their order.  mad: also the median and the median absolute deviation.  Returns
        the QuantileTable of the objects present, in (image, label) order.  A negative label, or one above max_label, raises
        CellScreenError (CS_ERR_INVALID); the measurer stays usable."""
        fr = as_fractions(quantiles)
        return quantile_table(*self.measure_dense(image, labels, fr, mad, exclude, max_label), fr)

    def last_timing(self):
        """Device milliseconds of the last measure_batch: quantiles_count_ms (clearing, counting, offsets), quantiles_scatter_ms
        (the values into their segments) and quantiles_select_ms (the selection)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.check(self._lib.cs_label_quantiles_last_timing(self._handle, C.byref(a), C.byref(b), C.byref(c)))
        return dict(quantiles_count_ms=a.value, quantiles_scatter_ms=b.value, quantiles_select_ms=c.value)
