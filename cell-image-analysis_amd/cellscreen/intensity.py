"""Per-object intensities on the device (cs_label_intensity, include/cellscreen.h): how bright every object of a
label image is in every channel and where its centre of mass lies -- skimage.measure.regionprops with an intensity image,
scipy.ndimage.sum / mean / standard_deviation / minimum / maximum / center_of_mass over labels, CellProfiler's
MeasureObjectIntensity.

    t = IntensityMeasurer().measure_batch(image, labels)                     # image [B,H,W] or [B,H,W,C], C <= 4
    ring = IntensityMeasurer().measure_batch(image, grown, exclude=nuclei)  # the cytoplasm around each nucleus
    t.mean[:, 0] / ring.mean[:, 0]                                           # where both tables hold the same objects

An object is the set of pixels of one image with one label > 0, connected or not, less the pixels where `exclude` is non-zero.
The device returns exact integer sums (area, sum r, sum c; per channel sum v, sum v^2, sum v*r, sum v*c, min, max); the derived
values are taken from them here in Python ints and float64, so they do not depend on a summation order:

    mean = sum v / n        std = sqrt(n * sum v^2 - (sum v)^2) / n   (population, the numerator exact)
    centroid = (sum r, sum c) / n        weighted_centroid = (sum v*r, sum v*c) / sum v, NaN where sum v = 0

Median, quantiles and MAD need a selection per object and are QuantileMeasurer's (cellscreen/quantile.py); texture is
TextureMeasurer's (cellscreen/texture.py); the edge measures are RadialMeasurer's (cellscreen/radial.py).
2-D only, at most 4 channels per call."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_LABEL, MAX_SIDE, LabelTool, _is_tensor, check_stack_shape  # noqa: F401
from .preprocess import PIX_U8, PIX_U16

MAX_CHANNELS = 4
MAX_CELLS = 1 << 22                     # batch * max_label * channels


@dataclass
class ObjectTable:
    """The objects present in a batch, in (image, label) order; n objects, C channels.  All numpy arrays on the host."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    centroid: np.ndarray                # [n,2] float64: row, column
    integrated: np.ndarray              # [n,C] int64: sum v
    mean: np.ndarray                    # [n,C] float64
    std: np.ndarray                     # [n,C] float64, population
    min: np.ndarray                     # [n,C] int64
    max: np.ndarray                     # [n,C] int64
    weighted_centroid: np.ndarray       # [n,C,2] float64: row, column; NaN where sum v = 0
    geom: np.ndarray                    # [n,3] int64: area, sum r, sum c
    stats: np.ndarray                   # [n,C,6] int64: sum v, sum v^2, sum v*r, sum v*c, min, max

    def __len__(self):
        return int(self.label.shape[0])


def object_table(geom: np.ndarray, stats: np.ndarray) -> ObjectTable:
    """The table of the dense tables cs_label_intensity writes: geom [B,max_label,3] and stats [B,max_label,C,6], int64.  The
    rows of absent objects (area 0) are dropped."""
    geom, stats = np.asarray(geom), np.asarray(stats)
    if geom.dtype != np.int64 or stats.dtype != np.int64:
        raise TypeError("geom and stats must be int64")
    if geom.ndim != 3 or geom.shape[2] != 3 or stats.ndim != 4 or stats.shape[3] != 6 or stats.shape[:2] != geom.shape[:2]:
        raise ValueError(f"geom {geom.shape} and stats {stats.shape}: [B,max_label,3] and [B,max_label,C,6] expected")
    img, row = np.nonzero(geom[:, :, 0] > 0)
    g, s = geom[img, row], stats[img, row]              # [n,3], [n,C,6]
    n, nc = g.shape[0], s.shape[1]
    area = g[:, 0]
    centroid = g[:, 1:3] / area[:, None].astype(np.float64)     # both sides exact in float64: one rounding
    sv, sv2 = s[:, :, 0], s[:, :, 1]
    mean = sv / area[:, None].astype(np.float64)
    std = np.empty((n, nc), np.float64)
    for i in range(n):
        a = int(area[i])
        for c in range(nc):
            std[i, c] = math.sqrt(a * int(sv2[i, c]) - int(sv[i, c]) ** 2) / a      # Python ints: the numerator is exact
    with np.errstate(invalid="ignore", divide="ignore"):
        wc = np.where(sv[:, :, None] > 0, s[:, :, 2:4] / sv[:, :, None].astype(np.float64), np.nan)
    return ObjectTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), area=area.copy(), centroid=centroid,
                       integrated=sv.copy(), mean=mean, std=std, min=s[:, :, 4].copy(), max=s[:, :, 5].copy(), weighted_centroid=wc,
                       geom=g, stats=s)


class IntensityMeasurer(LabelTool):
    """cs_label_intensity on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read
    in stream order."""
    _noun = "the measurer"

    # ---- argument checks: everything is refused before the device is touched.  The planes are checked together, kind and shape
    # before dtype and device, so check_label_plane, which finishes one plane before the next, would answer in another order ----
    def _check(self, image, labels, exclude, max_label):
        planes = [("image", image), ("labels", labels)] + ([("exclude", exclude)] if exclude is not None else [])
        for name, a in planes:
            if not (_is_tensor(a) or isinstance(a, np.ndarray)):
                raise TypeError(f"unsupported input type {type(a)} for {name}")
        on_dev = _is_tensor(image)
        if any(_is_tensor(a) != on_dev for _, a in planes):
            raise TypeError("image, labels and exclude must all be numpy arrays or all be CUDA tensors")
        if image.ndim not in (3, 4):
            raise ValueError(f"image must be [B,H,W] or [B,H,W,C], got shape {tuple(image.shape)}")
        for name, a in planes[1:]:
            if a.ndim != 3:
                raise ValueError(f"{name} must be [B,H,W], got shape {tuple(a.shape)}")
            if tuple(a.shape) != tuple(image.shape[:3]):
                raise ValueError(f"image {tuple(image.shape)} and {name} {tuple(a.shape)} differ in batch or height x width")
        B, H, W = (int(x) for x in labels.shape)
        nc = int(image.shape[3]) if image.ndim == 4 else 1
        check_stack_shape(B, H, W, image.shape, nc)
        if nc > MAX_CHANNELS:
            raise ValueError(f"{nc} channels: at most {MAX_CHANNELS} are measured per call, split the stack")
        if on_dev:
            import torch
            if image.dtype == torch.uint8:
                ptype = PIX_U8
            elif image.dtype in (torch.uint16, torch.int16):
                ptype = PIX_U16
            else:
                raise TypeError(f"image tensor dtype {image.dtype}: uint8 or uint16 expected")
            for name, a in planes:
                if name != "image" and a.dtype != torch.int32:
                    raise TypeError(f"{name} tensor dtype {a.dtype}: int32 expected")
                if not a.is_cuda:
                    raise ValueError(f"{name} is a CPU tensor; pass numpy arrays or CUDA tensors")
                if a.device.index != self.device_id:
                    raise ValueError(f"{name} is on {a.device}, the measurer on cuda:{self.device_id}")
                if not a.is_contiguous():
                    raise ValueError(f"{name} is not contiguous")
        else:
            if image.dtype == np.uint8:
                ptype = PIX_U8
            elif image.dtype == np.uint16:
                ptype = PIX_U16
            else:
                raise TypeError(f"image dtype {image.dtype}: uint8 or uint16 expected")
            for name, a in planes:
                if name != "image" and a.dtype != np.int32:
                    raise TypeError(f"{name} dtype {a.dtype}: int32 expected")
                if not a.flags.c_contiguous:
                    raise ValueError(f"{name} must be C-contiguous")
        if max_label is not None:
            if isinstance(max_label, (bool, np.bool_)) or not isinstance(max_label, (int, np.integer)):
                raise TypeError(f"max_label must be an integer or None, got {type(max_label).__name__}")
            self._check_size(B, int(max_label), nc)
        return B, H, W, nc, ptype, on_dev

    @staticmethod
    def _check_size(B, max_label, nc):
        if max_label < 1:
            raise ValueError(f"max_label {max_label}: must be >= 1")
        if max_label > MAX_LABEL:
            raise ValueError(f"max_label {max_label} above {MAX_LABEL}: relabel sparse ids first")
        if B * max_label * nc > MAX_CELLS:
            raise ValueError(f"batch {B} x max_label {max_label} x channels {nc} above {MAX_CELLS}: measure fewer images per call")

    def measure_dense(self, image, labels, exclude=None, max_label=None):
        """The dense tables as the device writes them, numpy on the host: geom int64 [B,max_label,3] (area, sum r, sum c) and
        stats int64 [B,max_label,C,6] (sum v, sum v^2, sum v*r, sum v*c, min, max), row label - 1 for a label; the rows of an
        absent object are all zero.  Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev = self._check(image, labels, exclude, max_label)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc)
        max_label = int(max_label)
        geom = np.empty((B, max_label, 3), np.int64)
        stats = np.empty((B, max_label, nc, 6), np.int64)
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_intensity(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                             max_label, L._ptr(geom), L._ptr(stats), L.CS_MEM_HOST))
        return geom, stats

    def measure_batch(self, image, labels, exclude=None, max_label=None) -> ObjectTable:
        """image: [B,H,W] or [B,H,W,C] uint8 / uint16 with C <= 4, every channel is measured; labels: int32 [B,H,W], 0 is
        background; exclude: None, or int32 [B,H,W]: a pixel where it is non-zero belongs to no object.  All numpy arrays, or all
        CUDA tensors of the measurer's device (uint16 tensors may come as int16 views).  max_label: an upper bound of the labels
        (it sizes the device tables), None: their maximum.  Returns the ObjectTable of the objects present, in (image, label)
        order.  A negative label, or one above max_label, raises CellScreenError (CS_ERR_INVALID); the measurer stays usable."""
        return object_table(*self.measure_dense(image, labels, exclude, max_label))

    def last_timing(self):
        """Device milliseconds of the last measure_batch: intensity_clear_ms (clearing the tables) and intensity_pass_ms (the
        pass over the planes with its closing step)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.cs_label_intensity_last_timing(self._handle, C.byref(a), C.byref(b)))
        return dict(intensity_clear_ms=a.value, intensity_pass_ms=b.value)
