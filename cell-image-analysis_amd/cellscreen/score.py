"""Scoring a label image against ground truth on the device: object matching by intersection over union (cs_label_match,
include/cellscreen.h), the measure of StarDist's `matching` and of the DSB-2018 score.

    m = LabelMatcher().match_batch(pred, truth)          # int32 [B,H,W] each, 0 = background
    s = m.stats((0.5, 0.7))
    s["total"]["by_threshold"][0]["f1"], s["images"][3]["merged"]

The device makes two tables per image, one row per label: area, partner (the object of the other image with the largest
intersection I, ties to the smaller label), overlap (that I) and n_major (how many objects of the other image lie mostly inside
this one: two or more is a merge on the pred side, a split on the truth side).  A pair (p, t) matches at the threshold tau when p
and t are each other's partner, 2 * I > U and I * 65536 >= int(tau * 65536 + 0.5) * U, with U = A_p + A_t - I.  The one
difference from StarDist, which accepts IoU >= tau: a pair whose IoU is exactly 1/2 never matches (it can differ at tau = 0.5
only).  2 * I > U implies that I is more than half of either object, so an object has at most one candidate: the matching is
unique and no assignment problem is solved.  The statistics are Python integers up to the last division; the sum of the matched
pairs' I / U is float64, added one after another in (image, pred label) order.

This measures agreement of objects, not boundary accuracy: there is no Hausdorff distance and no per-pixel Dice here."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_LABEL, MAX_SIDE, LabelTool, _is_tensor, check_label_plane, check_stack_shape  # noqa: F401

MAX_ROWS = 1 << 22                      # batch * max label, for each side
TABLE_LOG2 = (10, 26)
THRESHOLDS = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9)


def match_params(table_log2=None) -> L.CSMatchParams:
    """cs_match_params: table_log2 None (automatic first capacity of the pair table) or an integer in 10..26."""
    p = L.CSMatchParams()
    if table_log2 is not None:
        if isinstance(table_log2, bool) or not isinstance(table_log2, (int, np.integer)):
            raise TypeError(f"table_log2 {table_log2!r}: None or an integer")
        if not TABLE_LOG2[0] <= table_log2 <= TABLE_LOG2[1]:
            raise ValueError(f"table_log2 {table_log2} outside {TABLE_LOG2[0]}..{TABLE_LOG2[1]}")
        p.table_log2 = int(table_log2)
    return p


def threshold_q16(tau) -> int:
    """int(tau * 65536 + 0.5) of an IoU threshold in [0.5, 1]."""
    if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)):
        raise TypeError(f"threshold {tau!r}: a number in [0.5, 1]")
    tau = float(tau)
    if not 0.5 <= tau <= 1.0:                           # a NaN fails both
        raise ValueError(f"threshold {tau!r} outside [0.5, 1]")
    return int(tau * 65536 + 0.5)


def check_thresholds(thresholds):
    """(thresholds as floats, the same in 1/65536); refuses an empty list and anything outside [0.5, 1]."""
    if isinstance(thresholds, (int, float, np.integer, np.floating)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    thresholds = tuple(thresholds)
    if not thresholds:
        raise ValueError("no thresholds")
    tqs = [threshold_q16(t) for t in thresholds]
    return tuple(float(t) for t in thresholds), tqs


def _ratio(a, b):
    return a / b if b else 0.0


def _scores(tp, fp, fn, n_true, s):
    return dict(tp=tp, fp=fp, fn=fn, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn), accuracy=_ratio(tp, tp + fp + fn),
                f1=_ratio(2 * tp, 2 * tp + fp + fn), mean_matched_score=_ratio(s, tp), mean_true_score=_ratio(s, n_true),
                panoptic_quality=_ratio(s, tp + fp / 2 + fn / 2))


class LabelMatch(NamedTuple):
    """The tables of one match_batch: pred int32 [B, max_pred, 4] and truth int32 [B, max_truth, 4] with columns area, partner,
    overlap, n_major (row l - 1 for label l, all zeros for a label that does not occur), and n_pairs int64 [B], the distinct
    (p > 0, t > 0) pairs that intersect."""
    pred: np.ndarray
    truth: np.ndarray
    n_pairs: np.ndarray

    def stats(self, thresholds=THRESHOLDS):
        """{"thresholds": the thresholds, "images": one entry per image, "total": one for the batch}.  An entry holds n_pred,
        n_true, merged (pred with n_major >= 2), split (truth with n_major >= 2), missed (truth with partner 0), spurious (pred
        with partner 0), and "by_threshold": per threshold a dict of threshold, tp, fp, fn, precision = tp / (tp + fp),
        recall = tp / (tp + fn), accuracy = tp / (tp + fp + fn), f1 = 2 tp / (2 tp + fp + fn), mean_matched_score = sum / tp,
        mean_true_score = sum / n_true and panoptic_quality = sum / (tp + fp / 2 + fn / 2), `sum` being that of the matched
        pairs' I / U: StarDist's names and formulas.  A zero denominator gives 0."""
        thresholds, tqs = check_thresholds(thresholds)
        images = []
        tot = dict(n_pred=0, n_true=0, merged=0, split=0, missed=0, spurious=0)
        tot_rows = [[0, 0, 0, 0.0] for _ in tqs]
        for ptab, ttab in zip(self.pred.astype(np.int64), self.truth.astype(np.int64)):
            p_on, t_on = ptab[:, 0] > 0, ttab[:, 0] > 0
            e = dict(n_pred=int(p_on.sum()), n_true=int(t_on.sum()), merged=int((ptab[:, 3] >= 2).sum()),
                     split=int((ttab[:, 3] >= 2).sum()), missed=int((t_on & (ttab[:, 1] == 0)).sum()),
                     spurious=int((p_on & (ptab[:, 1] == 0)).sum()))
            for k in tot:
                tot[k] += e[k]
            t = ptab[:, 1]
            back = ttab[np.maximum(t, 1) - 1]                       # the partner's row (row 0 stands in where there is none)
            i = ptab[:, 2]
            u = ptab[:, 0] + back[:, 0] - i
            cand = (t > 0) & (back[:, 1] == np.arange(1, ptab.shape[0] + 1)) & (2 * i > u)
            e["by_threshold"] = []
            for k, tq in enumerate(tqs):
                m = cand & (i * 65536 >= tq * u)
                q = i[m] / u[m]                                     # exact integers below 2^53: the correctly rounded quotients
                tp = int(q.size)
                if tp:                                              # cumsum adds one after another, in the order of p
                    s = float(np.cumsum(q)[-1])
                    tot_rows[k][3] = float(np.cumsum(np.concatenate(([tot_rows[k][3]], q)))[-1])
                else:
                    s = 0.0
                fp, fn = e["n_pred"] - tp, e["n_true"] - tp
                for j, v in enumerate((tp, fp, fn)):
                    tot_rows[k][j] += v
                e["by_threshold"].append(dict(threshold=thresholds[k], **_scores(tp, fp, fn, e["n_true"], s)))
            images.append(e)
        tot["by_threshold"] = [dict(threshold=thresholds[k], **_scores(r[0], r[1], r[2], tot["n_true"], r[3]))
                               for k, r in enumerate(tot_rows)]
        return dict(thresholds=thresholds, images=images, total=tot)


def _check_max(name, v, B):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} {v!r}: None or an integer")
    if not 1 <= v <= MAX_LABEL or B * int(v) > MAX_ROWS:
        raise ValueError(f"{name} {v} x batch {B}: 1..{MAX_LABEL} labels per image and at most {MAX_ROWS} per batch; relabel sparse "
                         "ids in order first")
    return int(v)


class LabelMatcher(LabelTool):
    """cs_label_match on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter left on the device are read in stream order; table_log2: the
    first capacity of the pair table (None: automatic)."""
    _noun = "the matcher"

    def __init__(self, device_id: int = 0, extractor=None, table_log2=None):
        self._params = match_params(table_log2)
        super().__init__(device_id, extractor)

    # ---- argument checks: everything is refused before the device is touched ---------------------------------------
    def _check(self, pred, truth, max_pred, max_truth):
        check_label_plane("pred", pred, self.device_id, self._noun)
        check_label_plane("truth", truth, self.device_id, self._noun)
        if tuple(pred.shape) != tuple(truth.shape):
            raise ValueError(f"pred {tuple(pred.shape)} and truth {tuple(truth.shape)} differ in shape")
        B, H, W = (int(x) for x in pred.shape)
        check_stack_shape(B, H, W, pred.shape)
        if max_pred is not None:
            max_pred = _check_max("max_pred", max_pred, B)
        if max_truth is not None:
            max_truth = _check_max("max_truth", max_truth, B)
        return B, H, W, max_pred, max_truth

    def match_batch(self, pred, truth, max_pred=None, max_truth=None) -> LabelMatch:
        """pred, truth: int32 [B,H,W], numpy or CUDA tensors of the matcher's device (one of each: the numpy one is uploaded);
        0 is background.  max_pred, max_truth: the largest label each may hold (1..2^20, batch * max at most 2^22); None: the
        array's own maximum, which costs one reduction.  A label that is negative or above its max raises CellScreenError
        (CS_ERR_INVALID); the matcher stays usable."""
        B, H, W, max_pred, max_truth = self._check(pred, truth, max_pred, max_truth)
        if max_pred is None:
            max_pred = _check_max("max_pred", max(1, int(pred.max())), B)
        if max_truth is None:
            max_truth = _check_max("max_truth", max(1, int(truth.max())), B)
        on_dev = _is_tensor(pred) or _is_tensor(truth)
        if on_dev:
            import torch
            dev = pred.device if _is_tensor(pred) else truth.device
            if not _is_tensor(pred):
                pred = torch.from_numpy(pred).to(dev)
            if not _is_tensor(truth):
                truth = torch.from_numpy(truth).to(dev)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, pred, truth)
        ptab = np.empty((B, max_pred, 4), np.int32)
        ttab = np.empty((B, max_truth, 4), np.int32)
        n_pairs = np.zeros(B, np.int64)
        L.check(self._lib.cs_label_match(self._handle, L._ptr(pred), L._ptr(truth), B, H, W, L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST,
                                         max_pred, max_truth, C.byref(self._params), ptab.ctypes.data, ttab.ctypes.data, L.CS_MEM_HOST,
                                         n_pairs.ctypes.data))
        return LabelMatch(ptab, ttab, n_pairs)

    def last_timing(self):
        """Device milliseconds of the last match_batch: match_count_ms (clearing and the one pass over the planes) and
        match_reduce_ms (the reduction into the tables)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.cs_label_match_last_timing(self._handle, C.byref(a), C.byref(b)))
        return dict(match_count_ms=a.value, match_reduce_ms=b.value)

    def last_table(self):
        """(log2 of the pair table's capacity at the end of the last match_batch, how many times the call doubled it)."""
        a, b = C.c_int32(), C.c_int32()
        L.check(self._lib.cs_label_match_last_table(self._handle, C.byref(a), C.byref(b)))
        return a.value, b.value
