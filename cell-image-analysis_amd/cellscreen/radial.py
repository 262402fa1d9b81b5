"""Per-object radial intensity distribution and edge intensities on the device (cs_label_radial, include/cellscreen.h; DESIGN
3za): whether a stain sits at the membrane, in the cytoplasm or around the centre of every object of a label image --
CellProfiler's MeasureObjectIntensityDistribution (FracAtD, MeanFrac, RadialCV per ring) and the Edge measures of
MeasureObjectIntensity.  The rule is this project's (tests/radial_reference.py restates it); it corresponds to those measurements
without a promise of bit equality with CellProfiler.

    t = RadialMeasurer().measure_batch(image, labels, bins=4)               # image [B,H,W] or [B,H,W,C], C <= 4
    t.frac_at_d[:, 3, 0], t.mean_frac[:, 3, 0], t.radial_cv[:, 3, 0]        # the outermost ring, channel 0
    t.edge_mean[:, 0]                                                       # the outline's mean intensity
    cells = RadialMeasurer().measure_batch(image, grown, centers=nuclear_centres)

An object is IntensityMeasurer's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  E2(p) is the exact squared Euclidean distance from an object pixel to the nearest position that is not the
object's (another label, background, an excluded pixel, outside the image): scipy.ndimage.distance_transform_edt(np.pad(labels
== l, 1)) ** 2, exact up to MAX_D2 = 127^2; a deeper object raises CellScreenError (CS_ERR_UNSUPPORTED).  The centre is the
deepest pixel, the smallest raster index among equals (scipy.ndimage.maximum_position), or the caller's; C2(p) is the squared
distance to it along the straight line -- CellProfiler propagates it inside the object, the one deliberate difference: the two
agree wherever the segment to the centre stays inside the object.  With B bins, ring(p) is the number of k in 1..B-1 with
(B - k)^2 C2 >= k^2 E2, that is floor(B dc / (dc + de)) without a root; wedge(p) = (r > rc) + 2 (c > cc) + 4 (|r - rc| > |c - cc|).
The device returns exact integer records; the floats are taken from them here in Python ints and Fractions:

    frac_at_d = sum v [ring] / sum v [object]           mean_frac = frac_at_d / (n [ring] / n [object])
    radial_cv = population std / mean of the wedge means sum v / n, over the wedges of the ring that have pixels
    edge_mean = sum v / n     edge_std = sqrt(n sum v^2 - (sum v)^2) / n     over the pixels with E2 == 1

NaN where a denominator is 0.  frac_at_d, mean_frac and edge_mean are one correctly rounded division of two integers;
radial_cv and edge_std are the root of one correctly rounded quotient of two integers: within 2 * 2^-53 relative of the exact
value.  No geodesic distance, no unscaled rings, no Zernike moments, 2-D only, at most 16 bins and 4 channels."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from . import _lib as L
from ._labels import LabelTool
from .intensity import MAX_CHANNELS, IntensityMeasurer

MAX_D2 = 127 * 127                      # CS_RADIAL_MAX_D2: the deepest E2 an object may hold
MAX_BINS = 16                           # CS_RADIAL_MAX_BINS
MAX_RING_BYTES = 1 << 30
WEDGES = 8


def radial_params(bins=4) -> "L.CSRadialParams":
    """cs_radial_params of a call: bins 1..16."""
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)):
        raise TypeError(f"bins must be an integer, got {type(bins).__name__}")
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins {bins}: must be in 1..{MAX_BINS}")
    p = L.CSRadialParams()
    p.bins = int(bins)
    return p


@dataclass
class RadialTable:
    """The objects present in a batch, in (image, label) order; n objects, R rings, C channels.  All numpy arrays on the host.
    The floats are NaN where a denominator is 0."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    center_rc: np.ndarray               # [n,2] int32: the centre's row and column
    max_d2: np.ndarray                  # [n] int32: E2 at the deepest pixel
    edge_count: np.ndarray              # [n] int64: the pixels with E2 == 1
    frac_at_d: np.ndarray               # [n,R,C] float64
    mean_frac: np.ndarray               # [n,R,C]
    radial_cv: np.ndarray               # [n,R,C]
    edge_integrated: np.ndarray         # [n,C] int64
    edge_mean: np.ndarray               # [n,C] float64
    edge_std: np.ndarray                # [n,C], population
    edge_min: np.ndarray                # [n,C] int64
    edge_max: np.ndarray                # [n,C] int64
    geom: np.ndarray                    # [n,3] int64: area, sum r, sum c
    center: np.ndarray                  # [n,4] int32: row, column, E2 at the deepest pixel, edge count
    ring: np.ndarray                    # [n,R,8,1+C] int64: per ring and wedge n, sum v
    edge: np.ndarray                    # [n,C,4] int64: sum v, sum v^2, min, max over the edge pixels

    def __len__(self):
        return int(self.label.shape[0])


def _ratio(a: int, b: int) -> float:
    return a / b if b != 0 else math.nan                # Python ints: correctly rounded


def _root_of_ratio(f: Fraction) -> float:
    return math.sqrt(f.numerator / f.denominator)       # one correctly rounded quotient of Python ints, then its root


def radial_cv_exact(n, sv):
    """(std / mean)^2 of the wedge means sv[w] / n[w] over the wedges with n[w] > 0, population, as a Fraction; None without such
    a wedge or where the mean is 0."""
    means = [Fraction(int(s), int(k)) for k, s in zip(n, sv) if k > 0]
    if not means:
        return None
    m = sum(means) / len(means)
    if m == 0:
        return None
    var = sum(x * x for x in means) / len(means) - m * m
    return var / (m * m)


def radial_table(geom, center, ring, edge) -> RadialTable:
    """The table of the dense tables cs_label_radial writes: geom [B,max_label,3] int64, center [B,max_label,4] int32, ring
    [B,max_label,R,8,1+C] int64 and edge [B,max_label,C,4] int64.  The rows of absent objects (area 0) are dropped."""
    geom, center, ring, edge = np.asarray(geom), np.asarray(center), np.asarray(ring), np.asarray(edge)
    if geom.dtype != np.int64 or ring.dtype != np.int64 or edge.dtype != np.int64 or center.dtype != np.int32:
        raise TypeError("geom, ring and edge must be int64, center int32")
    nc = edge.shape[2] if edge.ndim == 4 else 0
    if (geom.ndim != 3 or geom.shape[2] != 3 or center.shape != geom.shape[:2] + (4,) or edge.ndim != 4 or edge.shape[3] != 4 or
            edge.shape[:2] != geom.shape[:2] or not 1 <= nc <= MAX_CHANNELS or ring.ndim != 5 or ring.shape[:2] != geom.shape[:2] or
            not 1 <= ring.shape[2] <= MAX_BINS or ring.shape[3:] != (WEDGES, 1 + nc)):
        raise ValueError(f"geom {geom.shape}, center {center.shape}, ring {ring.shape}, edge {edge.shape}: [B,max_label,3], "
                         "[B,max_label,4], [B,max_label,R,8,1+C] and [B,max_label,C,4] expected")
    img, row = np.nonzero(geom[:, :, 0] > 0)
    g, ct, rg, ed = geom[img, row], center[img, row], ring[img, row], edge[img, row]
    n, nb = g.shape[0], ring.shape[2]
    frac = np.full((n, nb, nc), np.nan)
    mfrac = np.full((n, nb, nc), np.nan)
    cv = np.full((n, nb, nc), np.nan)
    emean = np.full((n, nc), np.nan)
    estd = np.full((n, nc), np.nan)
    for k in range(n):
        area, ne = int(g[k, 0]), int(ct[k, 3])
        for ch in range(nc):
            total = int(rg[k, :, :, 1 + ch].sum())
            for r in range(nb):
                nw = [int(x) for x in rg[k, r, :, 0]]
                sw = [int(x) for x in rg[k, r, :, 1 + ch]]
                nr, sr = sum(nw), sum(sw)
                frac[k, r, ch] = _ratio(sr, total)
                mfrac[k, r, ch] = _ratio(sr * area, total * nr)
                q = radial_cv_exact(nw, sw)
                if q is not None:
                    cv[k, r, ch] = _root_of_ratio(q)
            sv, sv2 = int(ed[k, ch, 0]), int(ed[k, ch, 1])
            emean[k, ch] = _ratio(sv, ne)
            if ne:
                estd[k, ch] = _root_of_ratio(Fraction(ne * sv2 - sv * sv, ne * ne))
    return RadialTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), area=g[:, 0].copy(), center_rc=ct[:, :2].copy(),
                       max_d2=ct[:, 2].copy(), edge_count=ct[:, 3].astype(np.int64), frac_at_d=frac, mean_frac=mfrac, radial_cv=cv,
                       edge_integrated=ed[:, :, 0].copy(), edge_mean=emean, edge_std=estd, edge_min=ed[:, :, 2].copy(),
                       edge_max=ed[:, :, 3].copy(), geom=g, center=ct, ring=rg, edge=ed)


class RadialMeasurer(LabelTool):
    """cs_label_radial on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read
    in stream order.  The argument checks of the planes are IntensityMeasurer's, in its order."""
    _noun = "the measurer"
    _check = IntensityMeasurer._check
    _check_size = staticmethod(IntensityMeasurer._check_size)
    MAX_D2 = MAX_D2                     # the deepest E2 an object may hold: 127 px
    MAX_BINS = MAX_BINS

    @staticmethod
    def _check_centers(centers, B, H, W, max_label):
        if centers is None:
            return None
        if not isinstance(centers, np.ndarray):
            raise TypeError(f"centers must be a numpy array on the host, got {type(centers).__name__}")
        if centers.dtype != np.int32:
            raise TypeError(f"centers dtype {centers.dtype}: int32 expected")
        if centers.shape != (B, max_label, 2):
            raise ValueError(f"centers {centers.shape}: [{B},{max_label},2] (batch, max_label, row and column) expected")
        if not centers.flags.c_contiguous:
            raise ValueError("centers must be C-contiguous")
        if centers.size and (centers.min() < 0 or centers[..., 0].max() >= H or centers[..., 1].max() >= W):
            raise ValueError(f"centers: every row must lie inside the image {H}x{W}")
        return centers

    def measure_dense(self, image, labels, exclude=None, max_label=None, bins=4, centers=None, want_d2=False):
        """The dense tables as the device writes them, numpy on the host: geom int64 [B,max_label,3], center int32
        [B,max_label,4], ring int64 [B,max_label,bins,8,1+C] and edge int64 [B,max_label,C,4] (RadialTable names the fields), row
        label - 1 for a label; the rows of an absent object are all zero.  With want_d2 a fifth: the depth plane uint16 [B,H,W].
        Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev = self._check(image, labels, exclude, max_label)
        prm = radial_params(bins)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc)
        max_label = int(max_label)
        if B * max_label * prm.bins * WEDGES * (1 + nc) * 8 > MAX_RING_BYTES:
            raise ValueError(f"batch {B} x max_label {max_label} x bins {prm.bins} x channels {nc}: the ring table would exceed "
                             f"{MAX_RING_BYTES} bytes, split the batch")
        centers = self._check_centers(centers, B, H, W, max_label)
        geom = np.empty((B, max_label, 3), np.int64)
        center = np.empty((B, max_label, 4), np.int32)
        ring = np.empty((B, max_label, prm.bins, WEDGES, 1 + nc), np.int64)
        edge = np.empty((B, max_label, nc, 4), np.int64)
        d2 = np.empty((B, H, W), np.uint16) if want_d2 else None
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_radial(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                          max_label, C.byref(prm), L._ptr(centers), L._ptr(geom), L._ptr(center), L._ptr(ring),
                                          L._ptr(edge), L._ptr(d2), L.CS_MEM_HOST))
        return (geom, center, ring, edge, d2) if want_d2 else (geom, center, ring, edge)

    def measure_batch(self, image, labels, exclude=None, max_label=None, bins=4, centers=None) -> RadialTable:
        """image: [B,H,W] or [B,H,W,C] uint8 / uint16 with C <= 4; labels, exclude, max_label: as
        IntensityMeasurer.measure_batch.  bins: the rings between centre and outline, 1..16.  centers: None (the deepest pixel of
        every object), or a numpy int32 [B,max_label,2] of rows and columns inside the image, one per table row.  Returns the
        RadialTable of the objects present, in (image, label) order.  A negative label, or one above max_label, raises
        CellScreenError (CS_ERR_INVALID), an object deeper than 127 px CellScreenError (CS_ERR_UNSUPPORTED); the measurer stays
        usable."""
        return radial_table(*self.measure_dense(image, labels, exclude, max_label, bins, centers))

    def last_timing(self):
        """Device milliseconds of the last measure_batch: radial_columns_ms (with the clearing), radial_rows_ms (with the
        centres) and radial_bins_ms."""
        v = [C.c_double() for _ in range(3)]
        L.check(self._lib.cs_label_radial_last_timing(self._handle, *(C.byref(x) for x in v)))
        return dict(zip(("radial_columns_ms", "radial_rows_ms", "radial_bins_ms"), (x.value for x in v)))
