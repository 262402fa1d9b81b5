"""Growing labels inside a mask by geodesic cost on the device (cs_label_propagate, include/cellscreen.h): whole cells
from a nuclear segmentation and a second stain, CellProfiler's IdentifySecondaryObjects "Propagation" / "Watershed - Image",
skimage.segmentation.watershed(guide, markers, mask=).

    cells = LabelPropagator().propagate_batch(nuclei, mask=body, guide=image, guide_channel=1, lam=4)
    cells, cost = LabelPropagator().propagate_batch(nuclei, mask=body, distance=16, return_cost=True)

All integers.  A seed pixel (label 1..2^20) is a source of cost 0; it keeps its label whatever the mask says and no path enters
it.  A path leaves a seed and moves through pixels that are no seed and whose mask is non-zero, to 4- or 8-neighbours; a step
q -> p costs lam * w + |g(p) - g(q)|, with w by the metric ("cityblock": 1, 4-neighbours; "chessboard": 1, 8-neighbours; "chamfer":
5 axial and 7 diagonal) and g the guide's channel (0 without a guide); a candidate above max_cost is not taken.  A pixel takes the
lexicographic minimum over the paths that reach it of (cost, label): the smallest cost, the smallest label among equals; a pixel
that nothing reaches keeps label 0 and cost -1.  tests/propagate_reference.py restates the rule.

Deliberate differences from CellProfiler's Propagation: the geometric and the intensity term add (there: under a square root), the
intensity term is the difference of two pixels (there: of 3 x 3 neighbourhoods), lam >= 1 (no pure-intensity limit), and a tie goes
to the smallest label.  3 x 3 neighbourhoods only, 2-D, isotropic spacing; the cost of a call grows with the winding of the mask,
one round per tile crossing."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_LABEL, MAX_SIDE, LabelTool, _is_tensor, check_label_plane, check_stack_shape  # noqa: F401

PIX_U8, PIX_U16 = 0, 1                  # cs_pixel_type
MAX_CHANNELS = 4
MAX_LAM = 255
NO_LIMIT = L.PROPAGATE_NO_LIMIT         # 2^40 - 2
MAX_KEY_BYTES = 1 << 30                 # of the device's key plane, 8 bytes per pixel
METRICS = {"cityblock": L.PROPAGATE_CITYBLOCK, "chessboard": L.PROPAGATE_CHESSBOARD, "chamfer": L.PROPAGATE_CHAMFER}
AXIAL = {"cityblock": 1, "chessboard": 1, "chamfer": 5}
COST_UNREACHED = -1


def _integer(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer in {lo}..{hi}, got {type(v).__name__}")
    if not lo <= int(v) <= hi:
        raise ValueError(f"{name} {v} outside {lo}..{hi}")
    return int(v)


def max_cost_of(distance, metric="chamfer", lam=1) -> int:
    """The max_cost that stands for a distance in pixels without a guide: floor(distance * lam * a), a the metric's axial weight
    (1, 1, 5), taken exactly of the number given.  A bool, NaN, inf and a result outside 1..2^40 - 2 raise."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    lam = _integer("lam", lam, 1, MAX_LAM)
    if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, float, np.integer, np.floating)):
        raise TypeError(f"distance must be a number of pixels, got {type(distance).__name__}")
    d = float(distance)
    if math.isnan(d) or math.isinf(d):
        raise ValueError(f"distance {distance} is not finite")
    n = math.floor(Fraction(int(distance) if isinstance(distance, (int, np.integer)) else d) * lam * AXIAL[metric])
    if not 1 <= n <= NO_LIMIT:
        raise ValueError(f"distance {distance}: max_cost {n} outside 1..{NO_LIMIT}")
    return n


def propagate_params(metric="chamfer", lam=1, guide_channel=0, max_cost=None) -> L.CSPropagateParams:
    """cs_propagate_params: metric "cityblock", "chessboard" or "chamfer"; lam an integer in 1..255; max_cost an integer in
    1..2^40 - 2, None: no limit.  Anything else raises before a handle exists."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    p = L.CSPropagateParams()
    p.metric = METRICS[metric]
    p.lam = _integer("lam", lam, 1, MAX_LAM)
    p.guide_channel = _integer("guide_channel", guide_channel, 0, MAX_CHANNELS - 1)
    p.reserved = 0
    p.max_cost = NO_LIMIT if max_cost is None else _integer("max_cost", max_cost, 1, NO_LIMIT)
    return p


class LabelPropagator(LabelTool):
    """cs_label_propagate on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that seeds and a mask a segmenter left on the device are read in stream order and the
    grown labels feed the measurers without leaving the device."""
    _noun = "the propagator"

    # ---- argument checks: everything is refused before the device is touched ---------------------------------------
    def _check_plane(self, name, a, on_dev, shape, dtypes):
        """a: [B,H,W] (guide: or [B,H,W,C]) of one of `dtypes` (names), numpy or tensor as the seeds are."""
        if not (_is_tensor(a) or isinstance(a, np.ndarray)):
            raise TypeError(f"unsupported input type {type(a)} for {name}")
        if _is_tensor(a) != on_dev:
            raise TypeError(f"seeds and {name} must both be numpy arrays or both be CUDA tensors")
        if on_dev:
            import torch
            if a.dtype not in tuple(getattr(torch, d) for d in dtypes):
                raise TypeError(f"{name} tensor dtype {a.dtype}: {' or '.join(dtypes)} expected")
            if not a.is_cuda:
                raise ValueError(f"{name} is a CPU tensor; pass numpy arrays or CUDA tensors")
            if a.device.index != self.device_id:
                raise ValueError(f"{name} is on {a.device}, {self._noun} on cuda:{self.device_id}")
            if not a.is_contiguous():
                raise ValueError(f"{name} is not contiguous")
        else:
            if a.dtype not in tuple(np.dtype(d.replace("bool", "bool_")) for d in dtypes):
                raise TypeError(f"{name} dtype {a.dtype}: {' or '.join(dtypes)} expected")
            if not a.flags.c_contiguous:
                raise ValueError(f"{name} must be C-contiguous")
        if name == "guide":
            if a.ndim not in (3, 4):
                raise ValueError(f"guide must be [B,H,W] or [B,H,W,C], got shape {tuple(a.shape)}")
        elif a.ndim != 3:
            raise ValueError(f"{name} must be [B,H,W], got shape {tuple(a.shape)}")
        if tuple(a.shape[:3]) != shape:
            raise ValueError(f"seeds {shape} and {name} {tuple(a.shape)} differ in batch or height x width")

    def _check(self, seeds, mask, guide, guide_channel, out):
        check_label_plane("seeds", seeds, self.device_id, self._noun)
        B, H, W = (int(x) for x in seeds.shape)
        check_stack_shape(B, H, W, seeds.shape)
        if B * H * W * 8 > MAX_KEY_BYTES:
            raise ValueError(f"batch {B} x {H} x {W}: the key plane takes {B * H * W * 8} bytes, above {MAX_KEY_BYTES}: split the batch")
        on_dev = _is_tensor(seeds)
        if mask is not None:
            self._check_plane("mask", mask, on_dev, (B, H, W), ("bool", "uint8"))
        nc, ptype = 1, PIX_U8
        if guide is not None:
            self._check_plane("guide", guide, on_dev, (B, H, W), ("uint8", "uint16", "int16") if on_dev else ("uint8", "uint16"))
            nc = int(guide.shape[3]) if guide.ndim == 4 else 1
            if nc < 1:
                raise ValueError(f"empty batch or image: shape {tuple(guide.shape)}")
            if nc > MAX_CHANNELS:
                raise ValueError(f"{nc} channels: the guide has at most {MAX_CHANNELS}")
            ptype = PIX_U8 if (guide.element_size() if on_dev else guide.itemsize) == 1 else PIX_U16
            if guide_channel >= nc:
                raise ValueError(f"guide_channel {guide_channel} outside 0..{nc - 1}")
        elif guide_channel != 0:
            raise ValueError(f"guide_channel {guide_channel} without a guide")
        if out is not None:
            check_label_plane("out", out, self.device_id, self._noun)
            if _is_tensor(out) != on_dev:
                raise TypeError("seeds and out must both be numpy arrays or both be CUDA tensors")
            if tuple(out.shape) != (B, H, W):
                raise ValueError(f"out {tuple(out.shape)} and seeds {tuple(seeds.shape)} differ in shape")
            if isinstance(out, np.ndarray) and not out.flags.writeable:
                raise ValueError("out is read-only")
        return B, H, W, nc, ptype, on_dev

    def propagate_batch(self, seeds, mask=None, guide=None, guide_channel=0, metric="chamfer", lam=1, distance=None, max_cost=None,
                        return_cost: bool = False, out=None):
        """seeds: int32 [B,H,W], a numpy array or a CUDA tensor of the propagator's device; 0 is background, labels 1..2^20.
        mask: None (everywhere), or bool / uint8 [B,H,W], non-zero where a label may grow.  guide: None, or uint8 / uint16 [B,H,W]
        or [B,H,W,C] with C <= 4 (uint16 tensors may come as int16 views), of which channel guide_channel is read.  All numpy
        arrays, or all CUDA tensors.  metric: "cityblock", "chessboard" or "chamfer"; lam: the weight of a geometric step against
        one grey level, an integer in 1..255.  max_cost: the largest cost a pixel may take, an integer in 1..2^40 - 2, None: no
        limit; distance: instead of max_cost and only without a guide, a number of pixels: max_cost_of(distance, metric, lam).
        Returns the grown labels, numpy for numpy input and a CUDA tensor for tensor input, ids unchanged; with return_cost also
        an int64 plane of the same kind: 0 on seeds, the cost where a path reached, -1 elsewhere.  out: None, or where the grown
        labels go, an array or tensor like `seeds`; it may be `seeds` itself.  A negative seed or one above 2^20 raises
        CellScreenError (CS_ERR_INVALID, `out` is then undefined); the propagator stays usable."""
        if distance is not None:
            if max_cost is not None:
                raise ValueError("distance and max_cost are two ways to say one thing: give one")
            if guide is not None:
                raise ValueError("distance needs a cost in pixels: with a guide give max_cost")
            max_cost = max_cost_of(distance, metric, lam)
        params = propagate_params(metric, lam, guide_channel, max_cost)
        if not isinstance(return_cost, (bool, np.bool_)):
            raise TypeError(f"return_cost must be a bool, got {type(return_cost).__name__}")
        B, H, W, nc, ptype, on_dev = self._check(seeds, mask, guide, params.guide_channel, out)
        cost = None
        if on_dev:
            import torch
            if mask is not None and mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)           # one byte per pixel, 0 or 1
            if out is None:
                out = torch.empty_like(seeds)
            if return_cost:
                cost = torch.empty((B, H, W), dtype=torch.int64, device=seeds.device)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, seeds, mask, guide, out, cost)
        else:
            if mask is not None and mask.dtype == np.bool_:
                mask = mask.view(np.uint8)
            if out is None:
                out = np.empty((B, H, W), np.int32)
            if return_cost:
                cost = np.empty((B, H, W), np.int64)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_propagate(self._handle, L._ptr(seeds), B, H, W, kind, L._ptr(mask), L._ptr(guide), nc, ptype,
                                             C.byref(params), L._ptr(out), L._ptr(cost), kind))
        return (out, cost) if return_cost else out

    def last_timing(self):
        """Device milliseconds of the last propagate_batch: propagate_init_ms (clearing and the key plane), propagate_relax_ms (the
        rounds) and propagate_finish_ms (the labels' pass); and propagate_rounds, the number of rounds, the closing quiet one
        included."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        L.check(self._lib.cs_label_propagate_last_timing(self._handle, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(propagate_init_ms=a.value, propagate_relax_ms=b.value, propagate_finish_ms=c.value, propagate_rounds=n.value)
