"""Spots and their count per object on the device (cs_spot_detect / cs_spot_fill, include/cellscreen.h): FISH dots,
DNA-damage foci, vesicles, P-bodies inside every cell -- skimage.feature.blob_dog / peak_local_max, TrackMate's DoG detector,
Big-FISH, CellProfiler's second IdentifyPrimaryObjects with RelateObjects.

    det = SpotDetector(extractor=seg)                                   # the segmenter's handle: its labels are read in place
    p = spot_params(sigma=1.0, min_distance=2)                          # DoG of sigma 1 and 1.6, no two spots within 2 px
    t = det.detect_batch(images, threshold=12.0, labels=cells, params=p)
    t.n_per_object, t.mean_response, t.subpixel                         # spot_table's derived values

The response is R = (A_a - A_b + 2^23) >> 24 in 1/256 counts, A the segmenter's exact 48-bit Gaussian sums under two integer
tables (smooth_weights; sigma=0: the image itself); a pixel is a spot iff R >= threshold and its key (R, -raster index) is the
greatest of its (2 min_distance + 1)^2 window.  All integers on the device, bit-identical run to run.

The threshold is the caller's, in counts of the response.  White pixel noise of standard deviation s appears in R / 256 with
standard deviation s * dog_noise_gain(params), so `threshold = k * s * dog_noise_gain(params)` is k sigmas of the noise, with s
from ThresholdSegmenter.noise_mesh_batch or the caller's own estimate: that step is the caller's, nothing here picks a threshold.

Deliberate differences from skimage: the response is a floor-rounded integer, ties go to the first pixel in raster order, and
the window is a square (Chebyshev distance), where peak_local_max prunes by Euclidean distance.  One channel and one scale per
call, no scale-space search and no blob radius estimate, 2-D, min_distance <= 8, table radii <= 64."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_LABEL, MAX_SIDE, LabelTool, _is_tensor, check_label_plane, check_stack_shape  # noqa: F401
from .preprocess import PIX_U8, PIX_U16
from .segment import smooth_weights

MAX_RADIUS = L.SMOOTH_MAX_RADIUS
MAX_DISTANCE = 8
MAX_ROWS = 1 << 22                      # batch * max_label
MAX_SPOTS = 1 << 22                     # per call
MAX_SCRATCH = 1 << 30                   # 12 bytes per pixel of the batch must stay under it
FIELDS, RECORD = 8, 6                   # the lengths of a list row and of an object's record
INT32_MIN = -(1 << 31)
SIGMA_MAX = (MAX_RADIUS + 0.49) / 4.0   # the largest sigma whose table has radius <= 64


def _number(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name} must be a number, got {type(v).__name__}")
    return float(v)


def _integer(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
    return int(v)


def _table(name, sigma):
    w = smooth_weights(sigma)
    if not 1 <= len(w) - 1 <= MAX_RADIUS:
        raise ValueError(f"{name} {sigma}: its table has radius {len(w) - 1}, outside 1..{MAX_RADIUS}")
    return w


def spot_params(sigma, sigma_ratio=1.6, sigma_coarse=None, min_distance=2, channel=0) -> L.CSSpotParams:
    """cs_spot_params of a difference of Gaussians: the fine table of `sigma` (0: the identity, the image itself), the coarse table
    of sigma_coarse, or of sigma * sigma_ratio where that is None (sigma = 0 needs sigma_coarse).  min_distance: the half-width m
    of the peak window, 1..8.  channel: which channel of an interleaved image.  Anything out of range raises here, before a
    handle exists."""
    sa = _number("sigma", sigma)
    if not 0.0 <= sa <= SIGMA_MAX:                      # NaN fails
        raise ValueError(f"sigma {sigma} outside 0..{SIGMA_MAX}")
    if sigma_coarse is None:
        ratio = _number("sigma_ratio", sigma_ratio)
        if not ratio > 1.0:
            raise ValueError(f"sigma_ratio {sigma_ratio}: must be above 1")
        if sa == 0.0:
            raise ValueError("sigma 0 (the identity) has no ratio: give sigma_coarse")
        sb = sa * ratio
    else:
        sb = _number("sigma_coarse", sigma_coarse)
    if not sa < sb <= SIGMA_MAX:
        raise ValueError(f"sigma_coarse {sb}: must be above sigma {sa} and at most {SIGMA_MAX}")
    m, ch = _integer("min_distance", min_distance), _integer("channel", channel)
    if not 1 <= m <= MAX_DISTANCE:
        raise ValueError(f"min_distance {m} outside 1..{MAX_DISTANCE}")
    if ch < 0:
        raise ValueError(f"channel {ch}: must be >= 0")
    wb = _table("sigma_coarse", sb)
    wa = [65536] if sa == 0.0 or len(smooth_weights(sa)) == 1 else _table("sigma", sa)
    if wa == wb:
        raise ValueError(f"sigma {sa} and sigma_coarse {sb} give the same table")
    p = L.CSSpotParams()
    p.radius_a, p.radius_b, p.min_distance, p.channel, p.reserved = len(wa) - 1, len(wb) - 1, m, ch, 0
    for k, v in enumerate(wa):
        p.weights_a[k] = v
    for k, v in enumerate(wb):
        p.weights_b[k] = v
    return p


def tables_of(params: L.CSSpotParams):
    """(w_a, w_b) of a cs_spot_params as lists of ints."""
    return list(params.weights_a[:params.radius_a + 1]), list(params.weights_b[:params.radius_b + 1])


def dog_noise_gain(params: L.CSSpotParams) -> float:
    """sqrt(sum (k_a - k_b)^2) over the 2-D kernels of the two integer tables, float64: white pixel noise of standard deviation s
    has standard deviation s * gain in R / 256 (away from the borders, where the reflection correlates it).  For the caller's
    threshold; see the module text."""
    wa, wb = tables_of(params)
    r = max(len(wa), len(wb)) - 1
    full = [np.array([(w[abs(k)] if abs(k) < len(w) else 0) for k in range(-r, r + 1)], np.float64) / 65536.0 for w in (wa, wb)]
    d = np.outer(full[0], full[0]) - np.outer(full[1], full[1])
    return float(math.sqrt(float((d * d).sum())))


def _ratio(num, den) -> float:
    return num / den if den else math.nan


def _parabola(lo: int, mid: int, hi: int) -> float:
    """The offset of the vertex of the parabola through (-1, lo), (0, mid), (1, hi); 0 where a neighbour is outside the image or
    the three lie on a line."""
    if lo == INT32_MIN or hi == INT32_MIN:
        return 0.0
    den = 2 * (lo - 2 * mid + hi)
    return (lo - hi) / den if den else 0.0


@dataclass
class SpotTable:
    """The spots of a batch and, with labels, the objects present, in (image, label) order.  All numpy arrays on the host."""
    counts: np.ndarray                  # [B,2] int64: the spots of the image, those on label 0
    offsets: np.ndarray                 # [B+1] int64: the spots of image b are rows offsets[b] .. offsets[b+1]
    spots: np.ndarray                   # [n,8] int32: r, c, label, R, R above, below, left, right (INT32_MIN outside the image)
    image: np.ndarray                   # [n] int32: the image of every spot
    response: np.ndarray                # [n] float64: R / 256, counts
    subpixel: np.ndarray                # [n,2] float64: row, column with the parabola's offsets
    geom: Optional[np.ndarray] = None   # [k,3] int64: area, sum r, sum c of the objects present
    records: Optional[np.ndarray] = None            # [k,6] int64: n, sum R, sum R^2, max R, sum r, sum c over the object's spots
    object_image: Optional[np.ndarray] = None       # [k] int32
    object_label: Optional[np.ndarray] = None       # [k] int32
    area: Optional[np.ndarray] = None               # [k] int64
    n_per_object: Optional[np.ndarray] = None       # [k] int64
    per_area: Optional[np.ndarray] = None           # [k] float64: spots per pixel
    mean_response: Optional[np.ndarray] = None      # [k] float64, counts; NaN without a spot
    max_response: Optional[np.ndarray] = None       # [k] float64, counts; NaN without a spot
    spot_centroid: Optional[np.ndarray] = None      # [k,2] float64: row, column; NaN without a spot
    plane: Optional[object] = None      # the response [B,H,W] int32 where it was asked for: numpy, or a tensor as the images

    def __len__(self):
        return int(self.spots.shape[0])


def spot_table(counts, offsets, spots, geom=None, records=None, plane=None) -> SpotTable:
    """The table of what cs_spot_detect and cs_spot_fill write: counts [B,2], offsets [B+1], spots [n,8] and, with labels, the dense
    geom [B,max_label,3] and records [B,max_label,6], whose rows of absent objects (area 0) are dropped.  Every quotient is one
    division of Python ints; NaN where its denominator is 0."""
    counts, offsets, spots = np.asarray(counts), np.asarray(offsets), np.asarray(spots)
    if counts.dtype != np.int64 or offsets.dtype != np.int64 or spots.dtype != np.int32:
        raise TypeError("counts and offsets must be int64, spots int32")
    if counts.ndim != 2 or counts.shape[1] != 2 or offsets.shape != (counts.shape[0] + 1,) or spots.ndim != 2 or spots.shape[1] != FIELDS:
        raise ValueError(f"counts {counts.shape}, offsets {offsets.shape}, spots {spots.shape}: [B,2], [B+1] and [n,{FIELDS}] expected")
    if int(offsets[-1]) != spots.shape[0]:
        raise ValueError(f"offsets end at {int(offsets[-1])}, the list has {spots.shape[0]} spots")
    n = spots.shape[0]
    image = np.repeat(np.arange(counts.shape[0], dtype=np.int32), np.diff(offsets))
    sub = np.empty((n, 2), np.float64)
    for i, (r, c, _, v, up, down, left, right) in enumerate(spots.tolist()):
        sub[i] = r + _parabola(up, v, down), c + _parabola(left, v, right)
    t = SpotTable(counts=counts, offsets=offsets, spots=spots, image=image, response=spots[:, 3] / 256.0, subpixel=sub, plane=plane)
    if (geom is None) != (records is None):
        raise ValueError("geom and records come together")
    if geom is not None:
        geom, records = np.asarray(geom), np.asarray(records)
        if geom.dtype != np.int64 or records.dtype != np.int64:
            raise TypeError("geom and records must be int64")
        if geom.ndim != 3 or geom.shape[2] != 3 or records.shape != geom.shape[:2] + (RECORD,) or geom.shape[0] != counts.shape[0]:
            raise ValueError(f"geom {geom.shape} and records {records.shape}: [B,max_label,3] and [B,max_label,{RECORD}] expected")
        img, row = np.nonzero(geom[:, :, 0] > 0)
        g, s = geom[img, row], records[img, row]
        k = len(g)
        per, mean, mx, cen = np.empty(k), np.empty(k), np.empty(k), np.empty((k, 2))
        for i, ((a, _, _), (ns, sr, _, top, rr, cc)) in enumerate(zip(g.tolist(), s.tolist())):
            per[i], mean[i], mx[i] = _ratio(ns, a), _ratio(sr, 256 * ns), _ratio(top, 256) if ns else math.nan
            cen[i] = _ratio(rr, ns), _ratio(cc, ns)
        t.geom, t.records, t.object_image, t.object_label = g, s, img.astype(np.int32), (row + 1).astype(np.int32)
        t.area, t.n_per_object, t.per_area, t.mean_response, t.max_response, t.spot_centroid = g[:, 0].copy(), s[:, 0].copy(), per, mean, mx, cen
    return t


class SpotDetector(LabelTool):
    """cs_spot_detect and cs_spot_fill on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a
    ThresholdSegmenter) whose handle and stream to share, so that labels a segmenter, a LabelExpander or a LabelPropagator on that
    handle left on the device are read in stream order."""
    _noun = "the detector"

    # ---- argument checks: everything is refused before the device is touched ----
    def _check(self, images, threshold, labels, exclude, max_label, params, return_response):
        if params is None:
            params = spot_params(1.0)
        if not isinstance(params, L.CSSpotParams):
            raise TypeError(f"params must come from spot_params, got {type(params).__name__}")
        if not isinstance(return_response, (bool, np.bool_)):
            raise TypeError(f"return_response must be a bool, got {type(return_response).__name__}")
        if exclude is not None and labels is None:
            raise ValueError("exclude needs labels")
        planes = [("images", images)] + [(n, a) for n, a in (("labels", labels), ("exclude", exclude)) if a is not None]
        for name, a in planes:
            if not (_is_tensor(a) or isinstance(a, np.ndarray)):
                raise TypeError(f"unsupported input type {type(a)} for {name}")
        on_dev = _is_tensor(images)
        if any(_is_tensor(a) != on_dev for _, a in planes):
            raise TypeError("images, labels and exclude must all be numpy arrays or all be CUDA tensors")
        if images.ndim not in (3, 4):
            raise ValueError(f"images must be [B,H,W] or [B,H,W,C], got shape {tuple(images.shape)}")
        for name, a in planes[1:]:
            if a.ndim != 3:
                raise ValueError(f"{name} must be [B,H,W], got shape {tuple(a.shape)}")
            if tuple(a.shape) != tuple(images.shape[:3]):
                raise ValueError(f"images {tuple(images.shape)} and {name} {tuple(a.shape)} differ in batch or height x width")
        B, H, W = (int(x) for x in images.shape[:3])
        nc = int(images.shape[3]) if images.ndim == 4 else 1
        check_stack_shape(B, H, W, images.shape, nc)
        if params.channel >= nc:
            raise ValueError(f"channel {params.channel}: the images have {nc}")
        if B * H * W * 12 >= MAX_SCRATCH:
            raise ValueError(f"batch {B} x {H} x {W}: 12 bytes of scratch per pixel must stay under {MAX_SCRATCH}, detect fewer images per call")
        if on_dev:
            import torch
            if images.dtype == torch.uint8:
                ptype = PIX_U8
            elif images.dtype in (torch.uint16, torch.int16):
                ptype = PIX_U16
            else:
                raise TypeError(f"images tensor dtype {images.dtype}: uint8 or uint16 expected")
            for name, a in planes:
                if name != "images" and a.dtype != torch.int32:
                    raise TypeError(f"{name} tensor dtype {a.dtype}: int32 expected")
                if not a.is_cuda:
                    raise ValueError(f"{name} is a CPU tensor; pass numpy arrays or CUDA tensors")
                if a.device.index != self.device_id:
                    raise ValueError(f"{name} is on {a.device}, the detector on cuda:{self.device_id}")
                if not a.is_contiguous():
                    raise ValueError(f"{name} is not contiguous")
        else:
            if images.dtype == np.uint8:
                ptype = PIX_U8
            elif images.dtype == np.uint16:
                ptype = PIX_U16
            else:
                raise TypeError(f"images dtype {images.dtype}: uint8 or uint16 expected")
            for name, a in planes:
                if name != "images" and a.dtype != np.int32:
                    raise TypeError(f"{name} dtype {a.dtype}: int32 expected")
                if not a.flags.c_contiguous:
                    raise ValueError(f"{name} must be C-contiguous")
        if isinstance(threshold, (str, bytes)):
            raise TypeError("threshold must be a number of counts or one per image")
        ts = list(threshold) if hasattr(threshold, "__len__") else [threshold] * B
        if len(ts) != B:
            raise ValueError(f"threshold has {len(ts)} values for {B} images")
        thr = np.empty(B, np.int32)
        for b, t in enumerate(ts):
            v = _number("threshold", t)
            if not math.isfinite(v) or int(round(v * 256)) < 1 or int(round(v * 256)) >= 1 << 31:
                raise ValueError(f"threshold {t}: int(round(256 t)) must be 1..2^31 - 1")
            thr[b] = int(round(v * 256))
        if max_label is not None:
            if labels is None:
                raise ValueError("max_label needs labels")
            self._check_size(B, _integer("max_label", max_label))
        return B, H, W, nc, ptype, on_dev, params, thr

    @staticmethod
    def _check_size(B, max_label):
        if max_label < 1:
            raise ValueError(f"max_label {max_label}: must be >= 1")
        if max_label > MAX_LABEL:
            raise ValueError(f"max_label {max_label} above {MAX_LABEL}: relabel sparse ids first")
        if B * max_label > MAX_ROWS:
            raise ValueError(f"batch {B} x max_label {max_label} above {MAX_ROWS}: detect fewer images per call")

    def detect_dense(self, images, threshold, labels=None, exclude=None, max_label=None, params=None, return_response=False):
        """What the device writes: (counts [B,2] int64, offsets [B+1] int64, spots [n,8] int32, geom [B,max_label,3] int64 or None,
        records [B,max_label,6] int64 or None, response or None).  The tables are numpy on the host; the response [B,H,W] int32 is
        numpy for numpy images and a tensor for tensors.  Arguments as detect_batch."""
        B, H, W, nc, ptype, on_dev, params, thr = self._check(images, threshold, labels, exclude, max_label, params, return_response)
        if labels is not None and max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label)
        counts = np.empty((B, 2), np.int64)
        geom = records = None
        if labels is not None:
            geom, records = np.empty((B, int(max_label), 3), np.int64), np.empty((B, int(max_label), RECORD), np.int64)
        handle = self._handle
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        plane = None
        if return_response:
            if on_dev:
                import torch
                plane = torch.empty((B, H, W), dtype=torch.int32, device=images.device)
            else:
                plane = np.empty((B, H, W), np.int32)
        if on_dev:
            import torch
            L.order_after_torch(self._lib.cs_preproc_wait_stream, handle, images, labels, exclude)
            # the tables go to the host whatever the images are: with device images out_kind is the device, for the response's sake
            d_counts = torch.empty((B, 2), dtype=torch.int64, device=images.device)
            d_geom = torch.empty(geom.shape, dtype=torch.int64, device=images.device) if labels is not None else None
            d_rec = torch.empty(records.shape, dtype=torch.int64, device=images.device) if labels is not None else None
            outs = (d_counts, d_geom, d_rec)
        else:
            outs = (counts, geom, records)
        n = C.c_int64(0)
        L.check(self._lib.cs_spot_detect(handle, L._ptr(images), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                         int(max_label) if labels is not None else 0, C.byref(params), L._ptr(thr), L._ptr(outs[0]),
                                         L._ptr(outs[1]), L._ptr(outs[2]), L._ptr(plane), kind, C.byref(n)))
        if on_dev:                                      # the call has synchronised: the tables are complete
            counts = outs[0].cpu().numpy()
            if labels is not None:
                geom, records = outs[1].cpu().numpy(), outs[2].cpu().numpy()
        spots = np.empty((n.value, FIELDS), np.int32)
        offsets = np.empty(B + 1, np.int64)
        L.check(self._lib.cs_spot_fill(handle, L._ptr(spots) if n.value else None, n.value, L._ptr(offsets), L.CS_MEM_HOST))
        return counts, offsets, spots, geom, records, plane

    def detect_batch(self, images, threshold, labels=None, exclude=None, max_label=None, params=None, return_response=False) -> SpotTable:
        """images: [B,H,W] or [B,H,W,C] uint8 / uint16, params.channel of them is read; labels: None, or int32 [B,H,W], 0 is
        background; exclude: None, or int32 [B,H,W]: a spot where it is non-zero has label 0 (the pixel still takes part in the
        response and in the windows).  All numpy arrays, or all CUDA tensors of the detector's device (uint16 tensors may come as
        int16 views).  threshold: counts of the response, one number or one per image; int(round(256 t)) >= 1.  max_label: an
        upper bound of the labels (it sizes the device tables), None: their maximum.  params: spot_params(...), None:
        spot_params(1.0).  return_response: the response plane too (SpotTable.plane).  A negative label, or one above max_label,
        raises CellScreenError (CS_ERR_INVALID); the detector stays usable."""
        return spot_table(*self.detect_dense(images, threshold, labels, exclude, max_label, params, return_response))

    def last_timing(self):
        """Device milliseconds of the last detect_batch: spot_response_ms (clearing and the two passes of the response),
        spot_peaks_ms (the peak pass, the rows' counts and their scan) and spot_records_ms (the objects' geometry, the list and the
        per-object records)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.check(self._lib.cs_spot_last_timing(self._handle, C.byref(a), C.byref(b), C.byref(c)))
        return dict(spot_response_ms=a.value, spot_peaks_ms=b.value, spot_records_ms=c.value)
