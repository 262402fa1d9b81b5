"""Image and per-object focus and saturation records on the device (cs_image_quality and cs_object_focus, include/cellscreen.h;
DESIGN 3zh): whether a field, a tile of it or a cell is worth measuring, before anything is measured -- CellProfiler's
MeasureImageQuality (FocusScore, LocalFocusScore, PercentMinimal / PercentMaximal), scipy.ndimage.laplace / sobel.

    q = ImageQualityMeasurer().measure_batch(image, tile=64)                  # image [B,H,W] or [B,H,W,C], C <= 4
    keep = (q.laplacian_variance[:, 0] > 50.0) & (q.percent_saturated[:, 0] < 1.0)
    f = ImageQualityMeasurer(extractor=seg).measure_objects(image, labels)    # the same focus values per object

A pixel is interior iff it has a full 3 x 3 neighbourhood inside the image; only interior pixels have focus values: the
4-neighbour Laplacian L, the Tenengrad G = gx^2 + gy^2 of the Sobel responses and Brenner's centred gradient Br.  The device
returns exact integer records; every derived value is taken from them here, once, as one correctly rounded quotient of Python
ints (NaN where the denominator is 0), so none depends on a summation order:

    mean = sum v / n        std = sqrt((n sum v^2 - (sum v)^2) / n^2)        focus_score = (n sum v^2 - (sum v)^2) / (n sum v)
    laplacian_variance = (n_int sum L^2 - (sum L)^2) / n_int^2    tenengrad = sum G / n_int    brenner = sum Br / n_int
    percent_minimal / percent_maximal / percent_saturated = 100 n_at_min / n, 100 n_at_max / n, 100 n_sat / n
    local_focus_score = var(nv) / median(nv) over the mesh tiles with sum v > 0, nv their focus_score (population variance,
                        numpy's median, in Fractions); 0 where the median is 0

All in counts of the pixel type: CellProfiler's 0..1 scale of focus_score is this divided by the dtype's top.  2-D only, at most
4 channels per call."""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_LABEL, MAX_SIDE, LabelTool, _is_tensor, check_stack_shape  # noqa: F401
from .intensity import IntensityMeasurer
from .preprocess import PIX_U8, PIX_U16

MAX_CHANNELS = 4
MAX_TILES = 1 << 20                     # batch * channels * mesh tiles
MIN_TILE, MAX_TILE = 16, 1024
RECORD, TILE, FOCUS = 13, 8, 5          # the lengths of an image record, a tile record and an object's focus record


def _ratio(num: int, den: int) -> float:
    """num / den of Python ints, correctly rounded (CPython's int / int is, whatever the sizes: it is what Fraction.__float__
    does); NaN where den is 0."""
    return num / den if den else math.nan


def _sqrt_ratio(num: int, den: int) -> float:
    """sqrt(num / den) of Python ints, num >= 0, den > 0, with ONE rounding: the integer root of num / den scaled by 4^s to at
    least 64 bits, its lowest bit set where anything was cut off (a sticky bit far below the 53 that survive), and then the
    int -> float conversion, which rounds to nearest even."""
    if den == 0:
        return math.nan
    if num == 0:
        return 0.0
    s = max(0, 64 - (num.bit_length() - den.bit_length()) // 2)
    scaled, cut = divmod(num << (2 * s), den)
    root = math.isqrt(scaled)
    if cut or root * root != scaled:
        root |= 1
    return math.ldexp(float(root), -s)


def _derive(n, sv, sv2, n_int, sl, sl2, sg, sbr):
    """mean, std, focus_score, laplacian_variance, tenengrad, brenner of one record of Python ints."""
    var_num = n * sv2 - sv * sv
    return (_ratio(sv, n), _sqrt_ratio(var_num, n * n), _ratio(var_num, n * sv),
            _ratio(n_int * sl2 - sl * sl, n_int * n_int), _ratio(sg, n_int), _ratio(sbr, n_int))


def _derive_array(rec):
    """rec [..., 8] int64 (n, sum v, sum v^2, n_int, sum L, sum L^2, sum G, sum Br) -> six float64 arrays of shape [...]."""
    lead = rec.shape[:-1]
    out = np.empty((6,) + (int(np.prod(lead, dtype=np.int64)),), np.float64)
    for i, row in enumerate(rec.reshape(-1, 8).tolist()):           # tolist: Python ints
        out[:, i] = _derive(*row)
    return tuple(a.reshape(lead) for a in out)


def _pair_sum(pairs):
    """The sum of the quotients (num, den), den > 0, as one unreduced (num, den): added in pairs, a level at a time, so that
    only the last few additions meet long integers and no gcd is ever taken."""
    while len(pairs) > 1:
        nxt = [(a * d + c * b, b * d) for (a, b), (c, d) in zip(pairs[0::2], pairs[1::2])]
        if len(pairs) & 1:
            nxt.append(pairs[-1])
        pairs = nxt
    return pairs[0]


def _cmp_quotients(x, y):
    """The order of two quotients (num, den), den > 0: by their correctly rounded floats, which never invert an order, and where
    those are equal by the cross products."""
    fx, fy = x[0] / x[1], y[0] / y[1]
    if fx != fy:
        return -1 if fx < fy else 1
    d = x[0] * y[1] - y[0] * x[1]
    return (d > 0) - (d < 0)


def _local_focus(tiles) -> float:
    """var(nv) / median(nv) of the tiles [m, 8] with sum v > 0, nv = (n sum v^2 - (sum v)^2) / (n sum v): exact, one rounding.
    Summing 1024 Fractions of unlike denominators one after the other runs a gcd on tens of thousands of bits at every step
    (seconds per image and channel); the pairwise sums of unreduced quotients take milliseconds."""
    nv = [(n * sv2 - sv * sv, n * sv) for n, sv, sv2 in (row[:3] for row in tiles.reshape(-1, 8).tolist()) if sv > 0]
    if not nv:
        return math.nan
    # the median: the floats are correctly rounded, so they order the quotients up to ties, which cross products settle
    nv.sort(key=functools.cmp_to_key(_cmp_quotients))
    k = len(nv)
    med = Fraction(*nv[k // 2]) if k % 2 else (Fraction(*nv[k // 2 - 1]) + Fraction(*nv[k // 2])) / 2
    if med == 0:
        return 0.0
    p1, q1 = _pair_sum(nv)
    p2, q2 = _pair_sum([(a * a, b * b) for a, b in nv])
    # (k sum t^2 - (sum t)^2) / k^2 / med
    return _ratio((k * p2 * q1 * q1 - p1 * p1 * q2) * med.denominator, k * k * q2 * q1 * q1 * med.numerator)


@dataclass
class ImageQualityTable:
    """The images of a batch, B of them with C channels; with a mesh, its m_r x m_c tiles.  All numpy arrays on the host."""
    n: np.ndarray                       # [B] int64: pixels
    n_interior: np.ndarray              # [B] int64: pixels with a full 3 x 3 neighbourhood
    mean: np.ndarray                    # [B,C] float64
    std: np.ndarray                     # [B,C] float64, population
    min: np.ndarray                     # [B,C] int64
    max: np.ndarray                     # [B,C] int64
    focus_score: np.ndarray             # [B,C] float64: variance / mean, NaN where sum v = 0
    laplacian_variance: np.ndarray      # [B,C] float64, NaN without an interior
    tenengrad: np.ndarray               # [B,C] float64
    brenner: np.ndarray                 # [B,C] float64
    percent_minimal: np.ndarray         # [B,C] float64: pixels at the image's own minimum
    percent_maximal: np.ndarray         # [B,C] float64
    percent_saturated: np.ndarray       # [B,C] float64: pixels >= sat_level
    records: np.ndarray                 # [B,C,13] int64, as the device wrote them
    tile: int = 0                       # the mesh's tile side, 0: no mesh
    mesh: Optional[np.ndarray] = None   # [B,C,m_r,m_c,8] int64
    tile_mean: Optional[np.ndarray] = None                # [B,C,m_r,m_c] float64, and so the five below
    tile_std: Optional[np.ndarray] = None
    tile_focus_score: Optional[np.ndarray] = None
    tile_laplacian_variance: Optional[np.ndarray] = None
    tile_tenengrad: Optional[np.ndarray] = None
    tile_brenner: Optional[np.ndarray] = None
    local_focus_score: Optional[np.ndarray] = None        # [B,C] float64

    def __len__(self):
        return int(self.records.shape[0])


def image_quality_table(records: np.ndarray, mesh: Optional[np.ndarray] = None, tile: int = 0) -> ImageQualityTable:
    """The table of what cs_image_quality writes: records [B,C,13] and, with a mesh, mesh [B,C,m_r,m_c,8], int64."""
    records = np.asarray(records)
    if records.dtype != np.int64 or (mesh is not None and np.asarray(mesh).dtype != np.int64):
        raise TypeError("records and mesh must be int64")
    if records.ndim != 3 or records.shape[2] != RECORD:
        raise ValueError(f"records {records.shape}: [B,C,{RECORD}] expected")
    if mesh is not None:
        mesh = np.asarray(mesh)
        if mesh.ndim != 5 or mesh.shape[4] != TILE or mesh.shape[:2] != records.shape[:2]:
            raise ValueError(f"mesh {mesh.shape}: [B,C,m_r,m_c,{TILE}] of records {records.shape} expected")
    mean, std, fs, lv, ten, br = _derive_array(records[:, :, [0, 1, 2, 8, 9, 10, 11, 12]])
    n = records[:, :, 0]
    pct = [np.array([[_ratio(100 * k, d) for k, d in zip(kr, dr)] for kr, dr in zip(records[:, :, j].tolist(), n.tolist())],
                    np.float64).reshape(n.shape) for j in (5, 6, 7)]
    t = ImageQualityTable(n=n[:, 0].copy(), n_interior=records[:, 0, 8].copy(), mean=mean, std=std, min=records[:, :, 3].copy(),
                          max=records[:, :, 4].copy(), focus_score=fs, laplacian_variance=lv, tenengrad=ten, brenner=br,
                          percent_minimal=pct[0], percent_maximal=pct[1], percent_saturated=pct[2], records=records, tile=int(tile))
    if mesh is not None:
        t.mesh = mesh
        (t.tile_mean, t.tile_std, t.tile_focus_score, t.tile_laplacian_variance, t.tile_tenengrad, t.tile_brenner) = _derive_array(mesh)
        t.local_focus_score = np.array([[_local_focus(mesh[b, c]) for c in range(mesh.shape[1])] for b in range(mesh.shape[0])],
                                       np.float64).reshape(mesh.shape[:2])
    return t


@dataclass
class ObjectFocusTable:
    """The objects present in a batch, in (image, label) order; n objects, C channels.  All numpy arrays on the host."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    n_interior: np.ndarray              # [n] int64: the object's pixels interior to the image
    laplacian_variance: np.ndarray      # [n,C] float64, NaN where n_interior = 0
    tenengrad: np.ndarray               # [n,C] float64
    brenner: np.ndarray                 # [n,C] float64
    geom: np.ndarray                    # [n,3] int64: area, sum r, sum c
    focus: np.ndarray                   # [n,C,5] int64: n_int, sum L, sum L^2, sum G, sum Br

    def __len__(self):
        return int(self.label.shape[0])


def object_focus_table(geom: np.ndarray, focus: np.ndarray) -> ObjectFocusTable:
    """The table of the dense tables cs_object_focus writes: geom [B,max_label,3] and focus [B,max_label,C,5], int64.  The rows of
    absent objects (area 0) are dropped."""
    geom, focus = np.asarray(geom), np.asarray(focus)
    if geom.dtype != np.int64 or focus.dtype != np.int64:
        raise TypeError("geom and focus must be int64")
    if geom.ndim != 3 or geom.shape[2] != 3 or focus.ndim != 4 or focus.shape[3] != FOCUS or focus.shape[:2] != geom.shape[:2]:
        raise ValueError(f"geom {geom.shape} and focus {focus.shape}: [B,max_label,3] and [B,max_label,C,{FOCUS}] expected")
    img, row = np.nonzero(geom[:, :, 0] > 0)
    g, f = geom[img, row], focus[img, row]              # [n,3], [n,C,5]
    lv, ten, br = (np.empty(f.shape[:2], np.float64) for _ in range(3))
    for i, obj in enumerate(f.tolist()):
        for c, (ni, sl, sl2, sg, sbr) in enumerate(obj):
            lv[i, c], ten[i, c], br[i, c] = _ratio(ni * sl2 - sl * sl, ni * ni), _ratio(sg, ni), _ratio(sbr, ni)
    n_int = f[:, 0, 0].copy() if f.shape[1] else np.zeros(len(g), np.int64)
    return ObjectFocusTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), area=g[:, 0].copy(), n_interior=n_int,
                            laplacian_variance=lv, tenengrad=ten, brenner=br, geom=g, focus=f)


class ImageQualityMeasurer(LabelTool):
    """cs_image_quality and cs_object_focus on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a
    ThresholdSegmenter) whose handle and stream to share, so that a batch the segmenter has on the device is gated in stream
    order."""
    _noun = "the measurer"
    _check_objects = IntensityMeasurer._check           # image, labels, exclude, max_label: the same planes, the same rules
    _check_size = staticmethod(IntensityMeasurer._check_size)

    # ---- argument checks: everything is refused before the device is touched ----
    def _check_image(self, image, tile, sat_level):
        if not (_is_tensor(image) or isinstance(image, np.ndarray)):
            raise TypeError(f"unsupported input type {type(image)} for image")
        on_dev = _is_tensor(image)
        if image.ndim not in (3, 4):
            raise ValueError(f"image must be [B,H,W] or [B,H,W,C], got shape {tuple(image.shape)}")
        B, H, W = (int(x) for x in image.shape[:3])
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
            if not image.is_cuda:
                raise ValueError("image is a CPU tensor; pass a numpy array or a CUDA tensor")
            if image.device.index != self.device_id:
                raise ValueError(f"image is on {image.device}, the measurer on cuda:{self.device_id}")
            if not image.is_contiguous():
                raise ValueError("image is not contiguous")
        else:
            if image.dtype == np.uint8:
                ptype = PIX_U8
            elif image.dtype == np.uint16:
                ptype = PIX_U16
            else:
                raise TypeError(f"image dtype {image.dtype}: uint8 or uint16 expected")
            if not image.flags.c_contiguous:
                raise ValueError("image must be C-contiguous")
        if isinstance(tile, (bool, np.bool_)) or not isinstance(tile, (int, np.integer)):
            raise TypeError(f"tile must be an integer, got {type(tile).__name__}")
        tile = int(tile)
        if tile != 0 and not MIN_TILE <= tile <= MAX_TILE:
            raise ValueError(f"tile {tile}: must be 0 (no mesh) or {MIN_TILE}..{MAX_TILE}")
        m_r, m_c = (-(-H // tile), -(-W // tile)) if tile else (1, 1)
        if B * nc * m_r * m_c > MAX_TILES:
            raise ValueError(f"batch {B} x channels {nc} x mesh {m_r} x {m_c} above {MAX_TILES} tiles: measure fewer images per call")
        sat = None
        if sat_level is not None:
            if isinstance(sat_level, (int, np.integer)) and not isinstance(sat_level, (bool, np.bool_)):
                sat_level = [sat_level] * nc
            if isinstance(sat_level, (str, bytes)) or not hasattr(sat_level, "__len__"):
                raise TypeError(f"sat_level must be None, an integer or one integer per channel, got {type(sat_level).__name__}")
            if len(sat_level) != nc:
                raise ValueError(f"sat_level has {len(sat_level)} levels for {nc} channels")
            for s in sat_level:
                if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)):
                    raise TypeError(f"sat_level holds a {type(s).__name__}: integers expected")
                if not 0 <= int(s) <= 65536:
                    raise ValueError(f"sat_level {int(s)}: must be 0..65536")
            sat = np.array([int(s) for s in sat_level], np.int32)
        return B, H, W, nc, ptype, on_dev, tile, m_r, m_c, sat

    def measure_batch_dense(self, image, tile=0, sat_level=None):
        """The tables as the device writes them, numpy on the host: records int64 [B,C,13] (n, sum v, sum v^2, min, max, n_at_min,
        n_at_max, n_sat, n_int, sum L, sum L^2, sum G, sum Br) and, with tile > 0, mesh int64 [B,C,m_r,m_c,8] (n, sum v, sum v^2,
        n_int, sum L, sum L^2, sum G, sum Br), else None.  Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev, tile, m_r, m_c, sat = self._check_image(image, tile, sat_level)
        records = np.empty((B, nc, RECORD), np.int64)
        mesh = np.empty((B, nc, m_r, m_c, TILE), np.int64) if tile else None
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_image_quality(self._handle, L._ptr(image), ptype, nc, B, H, W, kind, tile, L._ptr(sat), L._ptr(records),
                                           L._ptr(mesh), L.CS_MEM_HOST))
        return records, mesh

    def measure_batch(self, image, tile=0, sat_level=None) -> ImageQualityTable:
        """image: [B,H,W] or [B,H,W,C] uint8 / uint16 with C <= 4, every channel is measured; a numpy array or a CUDA tensor of the
        measurer's device (uint16 tensors may come as int16 views).  tile: 0, or the side 16..1024 of the tiles of a mesh of
        ceil(H / tile) x ceil(W / tile) tiles, pixel (r, c) in tile ((r m_r) // H, (c m_c) // W).  sat_level: None (the dtype's
        top), an integer, or one per channel: a pixel >= its level counts as saturated."""
        records, mesh = self.measure_batch_dense(image, tile, sat_level)
        return image_quality_table(records, mesh, tile)

    def measure_objects_dense(self, image, labels, exclude=None, max_label=None):
        """The dense tables as the device writes them, numpy on the host: geom int64 [B,max_label,3] (area, sum r, sum c) and focus
        int64 [B,max_label,C,5] (n_int, sum L, sum L^2, sum G, sum Br), row label - 1 for a label; the rows of an absent object
        are all zero.  Arguments as measure_objects."""
        B, H, W, nc, ptype, on_dev = self._check_objects(image, labels, exclude, max_label)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc)
        max_label = int(max_label)
        geom = np.empty((B, max_label, 3), np.int64)
        focus = np.empty((B, max_label, nc, FOCUS), np.int64)
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_object_focus(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                         max_label, L._ptr(geom), L._ptr(focus), L.CS_MEM_HOST))
        return geom, focus

    def measure_objects(self, image, labels, exclude=None, max_label=None) -> ObjectFocusTable:
        """image as measure_batch; labels: int32 [B,H,W], 0 is background; exclude: None, or int32 [B,H,W]: a pixel where it is
        non-zero belongs to no object.  All numpy arrays, or all CUDA tensors of the measurer's device.  max_label: an upper bound
        of the labels (it sizes the device tables), None: their maximum.  The stencil reads the image, not the labels.  A negative
        label, or one above max_label, raises CellScreenError (CS_ERR_INVALID); the measurer stays usable."""
        return object_focus_table(*self.measure_objects_dense(image, labels, exclude, max_label))

    def last_timing(self):
        """Device milliseconds of the last calls: quality_clear_ms / quality_pass_ms of measure_batch, focus_clear_ms /
        focus_pass_ms of measure_objects."""
        out = {}
        for name, fn in (("quality", self._lib.cs_image_quality_last_timing), ("focus", self._lib.cs_object_focus_last_timing)):
            a, b = C.c_double(), C.c_double()
            L.check(fn(self._handle, C.byref(a), C.byref(b)))
            out[f"{name}_clear_ms"], out[f"{name}_pass_ms"] = a.value, b.value
        return out
