"""Per-object size and shape on the device (cs_label_shape, include/cellscreen.h): what the geometry properties of
skimage.measure.regionprops and CellProfiler's MeasureObjectSizeShape report of every object of a label image.

    t = ShapeMeasurer().measure_batch(labels)                      # int32 [B,H,W], 0 = background
    t.area, t.perimeter, t.form_factor, t.major_axis_length, t.orientation, t.solidity, t.euler_number, t.hu
    ring = ShapeMeasurer().measure_batch(grown, exclude=nuclei)    # the cytoplasm around each nucleus: Euler number 0

The objects are IntensityMeasurer's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  No image is read.  The device returns exact integers per object: ten moments (n and the sums of r, c, r^2, rc, c^2,
r^3, r^2 c, r c^2, c^3 in image coordinates), the bounding box, the histogram of 2 x 2 bit quads over the plane padded by one
background pixel, the three classes of skimage.measure.perimeter(neighbourhood=4), and with hull=True the convex area and the two
Feret records.  Everything else follows here in Python ints and float64, the numerators exact and one rounding each where the value
is rational:

    centroid = (sum r, sum c) / n           extent = n / bbox_area          equivalent_diameter = sqrt(4 n / pi)
    mu       central moments (20, 11, 02, 30, 21, 12, 03; the first index is the row's): N20 / n with N20 = n sum r^2 - (sum r)^2,
             N30 / n^2 with N30 = n^2 sum r^3 - 3 n sum r sum r^2 + 2 (sum r)^3, and so on
    inertia  [[mu02, -mu11], [-mu11, mu20]] / n, its eigenvalues l1 >= l2 in the closed form of CellExtractor's eccentricity;
             major, minor axis = 4 sqrt(l1), 4 sqrt(l2); eccentricity = sqrt(1 - l2 / l1), taken as sqrt(2 rad / l1)
    orientation = atan2(2 N11, N20 - N02) / 2: the angle of the major axis from the row axis, in -pi/2 .. pi/2, regionprops'
             convention; where N20 = N02 that is pi/4 with the sign of N11, and 0 for N11 = 0
    hu       Hu's seven invariants of the normalised central moments, each one exact integer numerator over a power of n
    perimeter = n1 + n2 sqrt(2) + n3 (1 + sqrt(2)) / 2               form_factor = 4 pi n / perimeter^2, NaN where it is 0
    euler_number = (Q1 - Q3 - 2 QD) / 4 for 8-connectivity (regionprops' default), euler_number_4 = (Q1 - Q3 + 2 QD) / 4
    solidity = n / convex_area      feret_diameter_max = sqrt(feret_max2) / 2       feret_diameter_min = w / (2 sqrt(den))

The hull is that of the pixel-edge midpoints, CellExtractor's; convex_area counts the pixel centres inside or on it.  The Feret
diameters are the largest distance between two of its vertices and its smallest width over its edges.  scikit-image's
feret_diameter_max traces the contour of the convex image instead and is up to a pixel larger: a deliberate difference.

2-D only, one hull rule, no Zernike moments, no Crofton perimeter (the quads are in the table: a caller can derive one), no radial
distribution and no compactness measures."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from ._labels import MAX_LABEL, LabelTool, _is_tensor, check_label_plane, check_stack_shape

MAX_ROWS = 1 << 22                      # batch * max_label
SQRT2 = math.sqrt(2.0)
PERIMETER_WEIGHTS = (1.0, SQRT2, (1.0 + SQRT2) / 2.0)
Q1_CODES, Q3_CODES, QD_CODES = (1, 2, 4, 8), (7, 11, 13, 14), (6, 9)


@dataclass
class ShapeTable:
    """The objects present in a batch, in (image, label) order; n objects.  All numpy arrays on the host."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    bbox: np.ndarray                    # [n,4] int32: minr, minc, maxr, maxc, the max exclusive
    bbox_area: np.ndarray               # [n] int64
    extent: np.ndarray                  # [n] float64
    centroid: np.ndarray                # [n,2] float64: row, column
    equivalent_diameter: np.ndarray     # [n] float64
    mu: np.ndarray                      # [n,7] float64: central moments 20, 11, 02, 30, 21, 12, 03 (row index first)
    inertia_tensor: np.ndarray          # [n,2,2] float64
    inertia_eigvals: np.ndarray         # [n,2] float64: l1 >= l2 >= 0
    major_axis_length: np.ndarray       # [n] float64
    minor_axis_length: np.ndarray       # [n] float64
    eccentricity: np.ndarray            # [n] float64
    orientation: np.ndarray             # [n] float64, radians
    hu: np.ndarray                      # [n,7] float64
    perimeter: np.ndarray               # [n] float64
    form_factor: np.ndarray             # [n] float64, NaN where the perimeter is 0
    euler_number: np.ndarray            # [n] int64, 8-connectivity
    euler_number_4: np.ndarray          # [n] int64, 4-connectivity
    convex_area: Optional[np.ndarray]   # [n] int64; these four None without the hull
    solidity: Optional[np.ndarray]      # [n] float64
    feret_diameter_max: Optional[np.ndarray]    # [n] float64
    feret_diameter_min: Optional[np.ndarray]    # [n] float64
    moments: np.ndarray                 # [n,10] int64: the device's records of the objects
    quads: np.ndarray                   # [n,16] int32
    perim: np.ndarray                   # [n,3] int32
    hull: Optional[np.ndarray]          # [n,4] int64: convex_area, feret_max2, feret_min_num, feret_min_den

    def __len__(self):
        return int(self.label.shape[0])


def central_numerators(m):
    """(N20, N11, N02, N30, N21, N12, N03) of ten moments as Python ints: the central moments of order 2 are N / n, those of
    order 3 are N / n^2."""
    n, sr, sc, srr, src, scc, srrr, srrc, srcc, sccc = (int(x) for x in m)
    return (n * srr - sr * sr, n * src - sr * sc, n * scc - sc * sc,
            n * n * srrr - 3 * n * sr * srr + 2 * sr ** 3,
            n * n * srrc - n * sc * srr - 2 * n * sr * src + 2 * sr * sr * sc,
            n * n * srcc - n * sr * scc - 2 * n * sc * src + 2 * sc * sc * sr,
            n * n * sccc - 3 * n * sc * scc + 2 * sc ** 3)


def hu_numerators(N):
    """The integer numerators of Hu's seven invariants and the powers of n under them, of central_numerators' seven: with
    eta2 = N2 / n^3 and eta3 = N3 / n^4.5 every invariant is a polynomial of even degree in the eta3."""
    p, m, q, a, c, b, d = N                             # 20, 11, 02, 30, 21, 12, 03
    s, t, u, v = a + b, c + d, a - 3 * b, 3 * c - d
    return ((p + q, 3), ((p - q) ** 2 + 4 * m * m, 6), (u * u + v * v, 9), (s * s + t * t, 9),
            (u * s * (s * s - 3 * t * t) + v * t * (3 * s * s - t * t), 18),
            ((p - q) * (s * s - t * t) + 4 * m * s * t, 12),
            (v * s * (s * s - 3 * t * t) - u * t * (3 * s * s - t * t), 18))


def inertia(n, N20, N11, N02):
    """(trr, trc, tcc, l1, l2, eccentricity) in the float operations of csrc/extract.hip and tests/extract_reference.eccentricity"""
    n2 = float(n) * float(n)
    trr, tcc, trc = float(N20) / n2, float(N02) / n2, float(N11) / n2
    mean2 = (tcc + trr) * 0.5
    half = (tcc - trr) * 0.5
    rad = math.sqrt(half * half + trc * trc)
    l1, l2 = mean2 + rad, mean2 - rad
    ecc = 0.0 if l1 == 0.0 else 1.0 if l2 <= 0.0 else math.sqrt((2.0 * rad) / l1)
    return trr, trc, tcc, l1, max(l2, 0.0), ecc


def gray_counts(quads):
    """(Q1, Q3, QD) int64 [...] of quads [..., 16]"""
    q = np.asarray(quads).astype(np.int64)
    return q[..., list(Q1_CODES)].sum(axis=-1), q[..., list(Q3_CODES)].sum(axis=-1), q[..., list(QD_CODES)].sum(axis=-1)


def shape_table(moments, box, quads, perim, hull=None) -> ShapeTable:
    """The table of the dense records cs_label_shape writes: moments int64 [B,max_label,10], box int32 [B,max_label,4], quads int32
    [B,max_label,16], perim int32 [B,max_label,3] and hull int64 [B,max_label,4] or None.  The rows of absent objects (n = 0) are
    dropped."""
    moments, box, quads, perim = np.asarray(moments), np.asarray(box), np.asarray(quads), np.asarray(perim)
    hull = None if hull is None else np.asarray(hull)
    if moments.dtype != np.int64 or box.dtype != np.int32 or quads.dtype != np.int32 or perim.dtype != np.int32 or (
            hull is not None and hull.dtype != np.int64):
        raise TypeError("moments and hull must be int64, box, quads and perim int32")
    lead = moments.shape[:2]
    if (moments.ndim != 3 or moments.shape[2] != 10 or box.shape != lead + (4,) or quads.shape != lead + (16,) or perim.shape != lead + (3,)
            or (hull is not None and hull.shape != lead + (4,))):
        raise ValueError(f"moments {moments.shape}, box {box.shape}, quads {quads.shape}, perim {perim.shape}"
                         f"{'' if hull is None else f', hull {hull.shape}'}: [B,max_label,10], [B,max_label,4], [B,max_label,16], "
                         "[B,max_label,3] and [B,max_label,4] expected")
    img, row = np.nonzero(moments[:, :, 0] > 0)
    m, bx, qd, pm = moments[img, row], box[img, row], quads[img, row], perim[img, row]
    hl = None if hull is None else hull[img, row]
    n = m.shape[0]
    area = m[:, 0].copy()
    bbox_area = (bx[:, 2] - bx[:, 0]).astype(np.int64) * (bx[:, 3] - bx[:, 1]).astype(np.int64)
    areaf = area.astype(np.float64)
    centroid = m[:, 1:3] / areaf[:, None]               # both sides exact in float64: one rounding
    mu, hu = np.empty((n, 7), np.float64), np.empty((n, 7), np.float64)
    tensor, eig = np.empty((n, 2, 2), np.float64), np.empty((n, 2), np.float64)
    ecc, orient = np.empty(n, np.float64), np.empty(n, np.float64)
    for i in range(n):                                  # Python ints: every numerator is exact
        a = int(area[i])
        N = central_numerators(m[i])
        for k in range(7):
            mu[i, k] = N[k] / (a if k < 3 else a * a)
        trr, trc, tcc, l1, l2, ecc[i] = inertia(a, N[0], N[1], N[2])
        tensor[i] = (tcc, -trc), (-trc, trr)
        eig[i] = l1, l2
        orient[i] = 0.5 * math.atan2(float(2 * N[1]), float(N[0] - N[2]))
        for k, (num, power) in enumerate(hu_numerators(N)):
            hu[i, k] = num / a ** power
    perimeter = pm[:, 0] + pm[:, 1] * PERIMETER_WEIGHTS[1] + pm[:, 2] * PERIMETER_WEIGHTS[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        form = np.where(perimeter > 0, 4.0 * math.pi * areaf / (perimeter * perimeter), np.nan)
    q1, q3, qdg = gray_counts(qd)
    convex = solidity = fmax = fmin = None
    if hl is not None:
        convex = hl[:, 0].copy()
        solidity = areaf / convex.astype(np.float64)
        fmax = np.sqrt(hl[:, 1].astype(np.float64)) / 2.0
        fmin = hl[:, 2].astype(np.float64) / (2.0 * np.sqrt(hl[:, 3].astype(np.float64)))
    return ShapeTable(image=img.astype(np.int32), label=(row + 1).astype(np.int32), area=area, bbox=bx.copy(), bbox_area=bbox_area,
                      extent=areaf / bbox_area.astype(np.float64), centroid=centroid,
                      equivalent_diameter=np.sqrt(4.0 * areaf / math.pi), mu=mu, inertia_tensor=tensor, inertia_eigvals=eig,
                      major_axis_length=4.0 * np.sqrt(eig[:, 0]), minor_axis_length=4.0 * np.sqrt(eig[:, 1]), eccentricity=ecc,
                      orientation=orient, hu=hu, perimeter=perimeter, form_factor=form, euler_number=(q1 - q3 - 2 * qdg) // 4,
                      euler_number_4=(q1 - q3 + 2 * qdg) // 4, convex_area=convex, solidity=solidity, feret_diameter_max=fmax,
                      feret_diameter_min=fmin, moments=m, quads=qd, perim=pm, hull=hl)


class ShapeMeasurer(LabelTool):
    """cs_label_shape on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter) whose
    handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read in
    stream order."""
    _noun = "the measurer"

    # ---- argument checks: everything is refused before the device is touched ----
    def _check(self, labels, exclude, max_label):
        check_label_plane("labels", labels, self.device_id, self._noun)
        if exclude is not None:
            check_label_plane("exclude", exclude, self.device_id, self._noun)
            if _is_tensor(exclude) != _is_tensor(labels):
                raise TypeError("labels and exclude must both be numpy arrays or both be CUDA tensors")
            if tuple(exclude.shape) != tuple(labels.shape):
                raise ValueError(f"labels {tuple(labels.shape)} and exclude {tuple(exclude.shape)} differ in shape")
        B, H, W = (int(x) for x in labels.shape)
        check_stack_shape(B, H, W, labels.shape)
        if max_label is not None:
            if isinstance(max_label, (bool, np.bool_)) or not isinstance(max_label, (int, np.integer)):
                raise TypeError(f"max_label must be an integer or None, got {type(max_label).__name__}")
            self._check_size(B, int(max_label))
        return B, H, W, _is_tensor(labels)

    @staticmethod
    def _check_size(B, max_label):
        if max_label < 1:
            raise ValueError(f"max_label {max_label}: must be >= 1")
        if max_label > MAX_LABEL:
            raise ValueError(f"max_label {max_label} above {MAX_LABEL}: relabel sparse ids first")
        if B * max_label > MAX_ROWS:
            raise ValueError(f"batch {B} x max_label {max_label} above {MAX_ROWS}: measure fewer images per call")

    def measure_dense(self, labels, exclude=None, max_label=None, hull=True):
        """The dense records as the device writes them, numpy on the host: moments int64 [B,max_label,10], box int32
        [B,max_label,4], quads int32 [B,max_label,16], perim int32 [B,max_label,3] and hull int64 [B,max_label,4] (None with
        hull=False), row label - 1 for a label; the rows of an absent object are all zero.  Arguments as measure_batch."""
        B, H, W, on_dev = self._check(labels, exclude, max_label)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label)
        max_label = int(max_label)
        moments = np.empty((B, max_label, 10), np.int64)
        box = np.empty((B, max_label, 4), np.int32)
        quads = np.empty((B, max_label, 16), np.int32)
        perim = np.empty((B, max_label, 3), np.int32)
        hl = np.empty((B, max_label, 4), np.int64) if hull else None
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_shape(self._handle, L._ptr(labels), L._ptr(exclude), B, H, W, kind, max_label, 1 if hull else 0,
                                         L._ptr(moments), L._ptr(box), L._ptr(quads), L._ptr(perim), L._ptr(hl), L.CS_MEM_HOST))
        return moments, box, quads, perim, hl

    def measure_batch(self, labels, exclude=None, max_label=None, hull=True) -> ShapeTable:
        """labels: int32 [B,H,W], 0 is background; exclude: None, or int32 [B,H,W]: a pixel where it is non-zero belongs to no
        object.  Both numpy arrays, or both CUDA tensors of the measurer's device.  max_label: an upper bound of the labels (it
        sizes the device tables), None: their maximum.  hull: whether the convex area and the Feret diameters are taken too.
        Returns the ShapeTable of the objects present, in (image, label) order.  A negative label, or one above max_label, raises
        CellScreenError (CS_ERR_INVALID); the measurer stays usable."""
        return shape_table(*self.measure_dense(labels, exclude, max_label, hull))

    def last_timing(self):
        """Device milliseconds of the last measure_batch: shape_moments_ms (clearing, the moments and bounding boxes) and
        shape_outline_ms (the quads, the perimeter classes and the hull)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.cs_label_shape_last_timing(self._handle, C.byref(a), C.byref(b)))
        return dict(shape_moments_ms=a.value, shape_outline_ms=b.value)
