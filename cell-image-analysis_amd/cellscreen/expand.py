"""Growing labels by a distance on the device (cs_label_expand, include/cellscreen.h): the step between a nuclear
segmentation and the measurement, skimage.segmentation.expand_labels, CellProfiler's IdentifySecondaryObjects "Distance-N",
QuPath's cell expansion.

    grown = LabelExpander().expand_batch(labels, 6)          # int32 [B,H,W], 0 = background; ids as they are
    grown, d2 = LabelExpander().expand_batch(labels, 6, return_d2=True)

Every object grows outwards by `distance` pixels and stops halfway to its neighbours.  All integers: with D2 the squared
Euclidean distance from a background pixel to the nearest labelled pixel of its image, a pixel with D2 <= max_d2 takes that
pixel's label, where max_d2 is the largest integer n with math.sqrt(n) <= float(distance), the library's `distances <= distance`
exactly.  Ties are the one deliberate difference: where pixels of different labels are equally near, the smallest label wins,
while SciPy's choice follows its scan order; tests/expand_reference.py restates the rule.

Growth sees the labels alone: it is not geodesic and not constrained by a mask or an intensity, spacing is isotropic, and
distances above 127 px are refused."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_SIDE, LabelTool, _is_tensor, check_label_plane, check_stack_shape  # noqa: F401

MAX_DISTANCE = 127
D2_FAR = 65535                          # the d2 of a pixel that no label reaches


def expand_params(distance) -> L.CSExpandParams:
    """cs_expand_params of a distance in pixels, a Python number in 1..127: max_d2 is the largest integer n with
    math.sqrt(n) <= float(distance), d * d for an integer d (1.5 -> 2, 2.9 -> 8).  A bool, NaN, inf and anything outside
    1..127 raise before a handle exists."""
    if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, float, np.integer, np.floating)):
        raise TypeError(f"distance must be a number of pixels in 1..{MAX_DISTANCE}, got {type(distance).__name__}")
    d = float(distance)
    if math.isnan(d) or math.isinf(d) or not 1.0 <= d <= MAX_DISTANCE:
        raise ValueError(f"distance {distance} outside 1..{MAX_DISTANCE}")
    if isinstance(distance, (int, np.integer)):
        n = int(distance) * int(distance)
    else:
        n = int(d * d)                                  # within one of the answer: the search settles the rounding
        while math.sqrt(n + 1) <= d:
            n += 1
        while math.sqrt(n) > d:
            n -= 1
    p = L.CSExpandParams()
    p.max_d2, p.reserved = n, 0
    return p


class LabelExpander(LabelTool):
    """cs_label_expand on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter left on the device are read in stream order and the grown
    labels feed extract_batch without leaving the device."""
    _noun = "the expander"

    # ---- argument checks: everything is refused before the device is touched ---------------------------------------
    def _check(self, labels, out):
        check_label_plane("labels", labels, self.device_id, self._noun)
        B, H, W = (int(x) for x in labels.shape)
        check_stack_shape(B, H, W, labels.shape)
        if out is not None:
            check_label_plane("out", out, self.device_id, self._noun)
            if _is_tensor(out) != _is_tensor(labels):
                raise TypeError("labels and out must both be numpy arrays or both be CUDA tensors")
            if tuple(out.shape) != (B, H, W):
                raise ValueError(f"out {tuple(out.shape)} and labels {tuple(labels.shape)} differ in shape")
            if isinstance(out, np.ndarray) and not out.flags.writeable:
                raise ValueError("out is read-only")
        return B, H, W

    def expand_batch(self, labels, distance, return_d2: bool = False, out=None):
        """labels: int32 [B,H,W], a numpy array or a CUDA tensor of the expander's device; 0 is background.  distance: a number
        of pixels in 1..127 (expand_params).  Returns the grown labels, numpy for numpy input and a CUDA tensor for tensor
        input, ids unchanged; with return_d2 also a uint16 plane of the same kind: 0 on labelled pixels, the squared distance
        to the nearest one where a label reached, 65535 elsewhere.  out: None, or where the grown labels go, an array or tensor
        like `labels`; it may be `labels` itself.  A negative label raises CellScreenError (CS_ERR_INVALID, `out` is then
        undefined); the expander stays usable."""
        params = expand_params(distance)
        if not isinstance(return_d2, (bool, np.bool_)):
            raise TypeError(f"return_d2 must be a bool, got {type(return_d2).__name__}")
        B, H, W = self._check(labels, out)
        on_dev = _is_tensor(labels)
        d2 = None
        if on_dev:
            import torch
            if out is None:
                out = torch.empty_like(labels)
            if return_d2:
                d2 = torch.empty((B, H, W), dtype=torch.uint16, device=labels.device)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, labels, out, d2)
        else:
            if out is None:
                out = np.empty((B, H, W), np.int32)
            if return_d2:
                d2 = np.empty((B, H, W), np.uint16)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_expand(self._handle, L._ptr(labels), B, H, W, kind, C.byref(params), L._ptr(out), L._ptr(d2), kind))
        return (out, d2) if return_d2 else out

    def last_timing(self):
        """Device milliseconds of the last expand_batch: expand_columns_ms (the column pass) and expand_rows_ms (the row pass)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.cs_label_expand_last_timing(self._handle, C.byref(a), C.byref(b)))
        return dict(expand_columns_ms=a.value, expand_rows_ms=b.value)
