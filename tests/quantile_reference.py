"""The rule of cs_label_quantiles restated in numpy integers: a sort per object, no histograms, no segments and no
tables in between, so that it shares nothing with the kernels.

An object is cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  A quantile is a rational num / den with 0 <= num <= den and 1 <= den <= 65536.  For an object of n >= 1 pixels whose
values in a channel, sorted, are s[0 .. n-1]:

    t = num * (n - 1)        (int64: below 2^40)
    lo = t // den,  rem = t % den,  hi = lo + (rem > 0)

The tables hold s[lo] and s[hi]; value = s[lo] + (s[hi] - s[lo]) * rem / den in float64 is numpy's method="linear", s[lo] and
s[hi] are its "lower" and "higher".  With mad, the median's ranks (num / den = 1 / 2) give m_lo and m_hi, the doubled deviations
are d = |2 v - (m_lo + m_hi)| and d_lo, d_hi are their order statistics at the same two ranks: median = (m_lo + m_hi) / 2 and
MAD = (d_lo + d_hi) / 4, exact in float64, no scale factor (scipy.stats.median_abs_deviation with scale=1).  The dense tables:

    count [B, max_label]           int32   the pixels of the object
    order [B, max_label, C, K, 2]  int32   s[lo], s[hi]
    mad   [B, max_label, C, 4]     int32   m_lo, m_hi, d_lo, d_hi          (None without mad)

row label - 1 for label `label`; an object without pixels has all-zero rows.  A negative label, or one above max_label, is
refused whatever `exclude` holds there.  measure() is the vectorised form (np.lexsort by label and value), measure_slow() sorts
every object's values as Python ints and takes the ranks with fractions.Fraction.  values() and derive() take what a table
reports from the integers."""
from fractions import Fraction

import numpy as np

from intensity_reference import _planes, contents, disks, noise        # noqa: F401  (the generators, for the tests and tools)

QUANTILES = ((1, 4), (1, 2), (3, 4), (1, 100), (99, 100))               # what the device tests ask for
TWELVE = ((0, 1), (1, 1), (1, 2), (1, 4), (3, 4), (1, 100), (1, 20), (19, 20), (99, 100), (1, 3), (1, 10), (9, 10))


def pairs(quantiles):
    """(num, den) integer pairs of Fractions or pairs, refused outside the rule's range."""
    out = []
    for q in quantiles:
        num, den = (q.numerator, q.denominator) if isinstance(q, Fraction) else (int(q[0]), int(q[1]))
        if not (1 <= den <= 65536 and 0 <= num <= den):
            raise ValueError(f"quantile {num}/{den} is outside the rule")
        out.append((num, den))
    if not out:
        raise ValueError("no quantiles")
    return out


def _select(key, lab, starts, ranks):
    """key, lab: the pixels' sort key and label, any order; the keys at ranks [objects, R] of every object's sorted keys"""
    o = np.lexsort((key, lab))
    return key[o][starts[:, None] + ranks]


def measure(image, labels, quantiles=QUANTILES, mad=False, exclude=None, max_label=None):
    """(count, order, mad or None) of image [B,H,W] or [B,H,W,C], labels [B,H,W] and exclude (None or [B,H,W])."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    q = pairs(quantiles)
    B, C, K = labels.shape[0], image.shape[3], len(q)
    num = np.array([a for a, _ in q], np.int64)
    den = np.array([b for _, b in q], np.int64)
    count = np.zeros((B, max_label), np.int32)
    order = np.zeros((B, max_label, C, K, 2), np.int32)
    mad_t = np.zeros((B, max_label, C, 4), np.int32) if mad else None
    for b in range(B):
        rr, cc = np.nonzero((labels[b] > 0) & (exclude[b] == 0))
        if rr.size == 0:
            continue
        lab = labels[b][rr, cc].astype(np.int64)
        srt = np.sort(lab)
        starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
        rows = srt[starts] - 1
        n = np.diff(np.r_[starts, srt.size]).astype(np.int64)
        count[b, rows] = n
        t = num[None, :] * (n[:, None] - 1)
        lo = t // den[None, :]
        hi = lo + (t % den[None, :] > 0)
        m_lo, m_hi = (n - 1) // 2, (n - 1) // 2 + ((n - 1) % 2 > 0)
        obj = np.searchsorted(srt[starts], lab)          # the object of every pixel
        for ch in range(C):
            v = image[b][rr, cc, ch].astype(np.int64)
            order[b, rows, ch, :, 0] = _select(v, lab, starts, lo)
            order[b, rows, ch, :, 1] = _select(v, lab, starts, hi)
            if mad:
                m = _select(v, lab, starts, np.stack([m_lo, m_hi], axis=1))
                d = np.abs(2 * v - m.sum(axis=1)[obj])
                mad_t[b, rows, ch, 0:2] = m
                mad_t[b, rows, ch, 2:4] = _select(d, lab, starts, np.stack([m_lo, m_hi], axis=1))
    return count, order, mad_t


def _ranks(num, den, n):
    t = Fraction(num, den) * (n - 1)
    lo = t.numerator // t.denominator
    return lo, lo + (1 if t != lo else 0)


def measure_slow(image, labels, quantiles=QUANTILES, mad=False, exclude=None, max_label=None):
    """measure(), object by object in Python ints and Fractions."""
    image, labels, exclude, max_label = _planes(image, labels, exclude, max_label)
    q = pairs(quantiles)
    B, H, W = labels.shape
    C, K = image.shape[3], len(q)
    count = np.zeros((B, max_label), np.int32)
    order = np.zeros((B, max_label, C, K, 2), np.int32)
    mad_t = np.zeros((B, max_label, C, 4), np.int32) if mad else None
    for b in range(B):
        members = {}
        for r in range(H):
            for c in range(W):
                lab = int(labels[b, r, c])
                if lab != 0 and int(exclude[b, r, c]) == 0:
                    members.setdefault(lab, []).append((r, c))
        for lab, px in members.items():
            n = len(px)
            count[b, lab - 1] = n
            for ch in range(C):
                s = sorted(int(image[b, r, c, ch]) for r, c in px)
                for k, (num, den) in enumerate(q):
                    lo, hi = _ranks(num, den, n)
                    order[b, lab - 1, ch, k] = s[lo], s[hi]
                if mad:
                    lo, hi = _ranks(1, 2, n)
                    d = sorted(abs(2 * v - (s[lo] + s[hi])) for v in s)
                    mad_t[b, lab - 1, ch] = s[lo], s[hi], d[lo], d[hi]
    return count, order, mad_t


def values(n, lower, upper, quantiles):
    """value [..., K] float64 of lower, upper [..., K] and the pixel counts n, which broadcast against [...]: the rule's
    interpolation, evaluated left to right"""
    q = pairs(quantiles)
    num = np.array([a for a, _ in q], np.int64)
    den = np.array([b for _, b in q], np.int64)
    rem = (num * (np.asarray(n, np.int64)[..., None] - 1)) % den
    return lower + (upper - lower).astype(np.float64) * rem / den


def derive(count, order, mad, quantiles):
    """The present objects in (image, label) order as a dict of arrays: image, label, count [n], lower, upper [n,C,K] int32, value
    [n,C,K] float64 and, with mad, median, mad [n,C] float64 and mad_raw [n,C,4] int32."""
    B, M, C, K = order.shape[:4]
    keys = [(b, m) for b in range(B) for m in range(M) if count[b, m] > 0]
    n = len(keys)
    out = dict(image=np.array([b for b, _ in keys], np.int32).reshape(n), label=np.array([m + 1 for _, m in keys], np.int32).reshape(n),
               count=np.zeros(n, np.int32), lower=np.zeros((n, C, K), np.int32), upper=np.zeros((n, C, K), np.int32),
               value=np.zeros((n, C, K)))
    if mad is not None:
        out.update(median=np.zeros((n, C)), mad=np.zeros((n, C)), mad_raw=np.zeros((n, C, 4), np.int32))
    q = pairs(quantiles)
    for i, (b, m) in enumerate(keys):
        cnt = int(count[b, m])
        out["count"][i] = cnt
        out["lower"][i], out["upper"][i] = order[b, m, :, :, 0], order[b, m, :, :, 1]
        for ch in range(C):
            for k, (num, den) in enumerate(q):
                lo, hi = (int(x) for x in order[b, m, ch, k])
                out["value"][i, ch, k] = lo + float((hi - lo) * ((num * (cnt - 1)) % den)) / den
            if mad is not None:
                m_lo, m_hi, d_lo, d_hi = (int(x) for x in mad[b, m, ch])
                out["mad_raw"][i, ch] = mad[b, m, ch]
                out["median"][i, ch] = (m_lo + m_hi) / 2
                out["mad"][i, ch] = (d_lo + d_hi) / 4
    return out
