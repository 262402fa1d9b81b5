"""Per-object neighbours and contact on the device (cs_label_neighbors, include/cellscreen.h): what CellProfiler's
MeasureObjectNeighbors reports of every object of a label image.

    t = NeighborMeasurer().measure_batch(labels, distance=5)       # int32 [B,H,W], 0 = background
    t.number_of_neighbors, t.percent_touching, t.nearest_edge_label, t.first_closest_distance, t.angle_between_neighbors
    labels_i, d2_i, n_near_i = t.neighbors_of(i)                   # the neighbours of the table's object i

The objects are IntensityMeasurer's without an `exclude` plane: the pixels of one image with one label > 0, connected or not.  All
distances on the device are squared Euclidean distances between pixel centres, in integers; `distance` becomes max_d2 as
LabelExpander's does: the largest integer whose square root is <= distance (1 -> 1: 4-adjacent; 1.5 -> 2: 8-adjacent).  The device
returns exact integers: per object area, sum r, sum c, the number of its border pixels (a 4-neighbour is not the object's, outside the
image included), how many of them have a foreign label within max_d2, and its degree; per directed pair (a, b) with
D2(a, b) <= max_d2 the smallest squared distance D2 between their pixels and n_near, the number of a's border pixels whose nearest
foreign label (smallest d2, then smallest label) is b.  An object between two others does not hide them from each other: this is
CellProfiler's "dilate a by strel_disk(d) and collect the labels it meets" with max_d2 = d * d.  Everything else follows here in
float64:

    number_of_neighbors = degree                percent_touching = 100 touching / border
    nearest_edge_label, nearest_edge_distance   the neighbour at the smallest (D2, label) and sqrt(D2); 0 / NaN without neighbours
    first_closest_*, second_closest_*           over ALL objects of the image, neighbours or not, by the distance of the centroids
                                                (sum / area, d = sqrt(dr^2 + dc^2)), ordered by (d, label); 0 / NaN where the image
                                                has fewer than 2 or 3 objects
    angle_between_neighbors                     degrees, at this centroid between the first and the second closest; NaN without both
                                                or where one of them shares this centroid

2-D only, distances up to 32 px, Euclidean and not geodesic, no `exclude`, one label plane: no neighbours between two different sets
of objects."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._labels import MAX_LABEL, LabelTool, _is_tensor, check_label_plane, check_stack_shape
from .expand import expand_params

MAX_DISTANCE = 32
MAX_D2 = MAX_DISTANCE * MAX_DISTANCE
MAX_ROWS = 1 << 22                      # batch * max_label
TABLE_LOG2 = (10, 26)


def neighbor_params(distance, table_log2: int = 0) -> L.CSNeighborsParams:
    """cs_neighbors_params of a distance in pixels, a Python number in 1..32: max_d2 as expand_params takes it (1.5 -> 2, 2.9 -> 8,
    math.sqrt(n) -> n).  table_log2: 0, or 10..26, the first capacity of the device's pair table.  Everything else raises before a
    handle exists."""
    try:
        n = expand_params(distance).max_d2              # the types, NaN, inf, below 1
    except ValueError:
        raise ValueError(f"distance {distance} outside 1..{MAX_DISTANCE}") from None
    if n > MAX_D2 or float(distance) > MAX_DISTANCE:
        raise ValueError(f"distance {distance} outside 1..{MAX_DISTANCE}")
    if isinstance(table_log2, (bool, np.bool_)) or not isinstance(table_log2, (int, np.integer)):
        raise TypeError(f"table_log2 must be an integer, got {type(table_log2).__name__}")
    if table_log2 != 0 and not TABLE_LOG2[0] <= table_log2 <= TABLE_LOG2[1]:
        raise ValueError(f"table_log2 {table_log2}: 0 (automatic) or {TABLE_LOG2[0]}..{TABLE_LOG2[1]}")
    p = L.CSNeighborsParams()
    p.max_d2, p.table_log2, p.reserved = n, int(table_log2), 0
    return p


@dataclass
class NeighborTable:
    """The objects present in a batch, in (image, label) order; n objects.  All numpy arrays on the host."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    centroid: np.ndarray                # [n,2] float64: row, column
    border: np.ndarray                  # [n] int32: border pixels
    touching: np.ndarray                # [n] int32: those with a foreign label within the distance
    number_of_neighbors: np.ndarray     # [n] int32
    percent_touching: np.ndarray        # [n] float64
    nearest_edge_label: np.ndarray      # [n] int32, 0: no neighbour
    nearest_edge_distance: np.ndarray   # [n] float64, NaN: no neighbour
    first_closest_label: np.ndarray     # [n] int32, 0: the image has no other object
    first_closest_distance: np.ndarray  # [n] float64
    second_closest_label: np.ndarray    # [n] int32
    second_closest_distance: np.ndarray  # [n] float64
    angle_between_neighbors: np.ndarray  # [n] float64, degrees
    geom: np.ndarray                    # [n,3] int64: the device's records of the objects
    objects: np.ndarray                 # [n,3] int32
    row_start: np.ndarray               # [n] int64: the object's row is pairs[row_start : row_end]
    row_end: np.ndarray                 # [n] int64
    pairs: np.ndarray                   # [n_pairs,3] int32: neighbour label, D2, n_near; every row sorted by label

    def __len__(self):
        return int(self.label.shape[0])

    def neighbors_of(self, i):
        """(labels, d2, n_near) of the table's object i, int32 arrays sorted by label; the neighbours are objects of its image."""
        row = self.pairs[int(self.row_start[i]):int(self.row_end[i])]
        return row[:, 0].copy(), row[:, 1].copy(), row[:, 2].copy()


def _closest_two(centroid):
    """(first label index, first d, second label index, second d, angle) among the n objects of one image, indices -1 where there is
    none; ordered by (d, index), the indices in label order."""
    n = centroid.shape[0]
    i1, i2 = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    d1, d2, ang = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    if n < 2:
        return i1, d1, i2, d2, ang
    step = max(1, (1 << 22) // n)                       # rows of the distance matrix at a time
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        me = np.arange(lo, hi)
        dr = centroid[None, :, 0] - centroid[lo:hi, None, 0]
        dc = centroid[None, :, 1] - centroid[lo:hi, None, 1]
        d = np.sqrt(dr * dr + dc * dc)
        d[me - lo, me] = np.inf
        a = np.argmin(d, axis=1)                        # the first of equal distances: the smaller label
        i1[lo:hi], d1[lo:hi] = a, d[me - lo, a]
        if n < 3:
            continue
        d[me - lo, a] = np.inf
        b = np.argmin(d, axis=1)
        i2[lo:hi], d2[lo:hi] = b, d[me - lo, b]
        dot = dr[me - lo, a] * dr[me - lo, b] + dc[me - lo, a] * dc[me - lo, b]
        norm = d1[lo:hi] * d2[lo:hi]
        with np.errstate(divide="ignore", invalid="ignore"):
            cosv = np.clip(dot / norm, -1.0, 1.0)
        ang[lo:hi] = np.where(norm > 0.0, np.degrees(np.arccos(cosv)), np.nan)
    return i1, d1, i2, d2, ang


def neighbor_table(geom, objects, offsets, pairs) -> NeighborTable:
    """The table of the dense records cs_label_neighbors writes: geom int64 [B,max_label,3], objects int32 [B,max_label,3], offsets
    int64 [B * max_label + 1] and pairs int32 [n_pairs,3].  The rows of absent objects (area 0) are dropped; they have no pairs."""
    geom, objects, offsets, pairs = np.asarray(geom), np.asarray(objects), np.asarray(offsets), np.asarray(pairs)
    if geom.dtype != np.int64 or objects.dtype != np.int32 or offsets.dtype != np.int64 or pairs.dtype != np.int32:
        raise TypeError("geom and offsets must be int64, objects and pairs int32")
    if (geom.ndim != 3 or geom.shape[2] != 3 or objects.shape != geom.shape or offsets.shape != (geom.shape[0] * geom.shape[1] + 1,)
            or pairs.ndim != 2 or pairs.shape[1] != 3 or pairs.shape[0] != int(offsets[-1])):
        raise ValueError(f"geom {geom.shape}, objects {objects.shape}, offsets {offsets.shape}, pairs {pairs.shape}: [B,max_label,3], "
                         "[B,max_label,3], [B * max_label + 1] and [offsets[-1],3] expected")
    M = geom.shape[1]
    img, row = np.nonzero(geom[:, :, 0] > 0)
    g, ob = geom[img, row], objects[img, row]
    n = g.shape[0]
    area = g[:, 0].copy()
    centroid = g[:, 1:3] / area.astype(np.float64)[:, None]             # both sides exact in float64: one rounding
    flat = img.astype(np.int64) * M + row
    start, end = offsets[flat], offsets[flat + 1]
    near_label, near_d = np.zeros(n, np.int32), np.full(n, np.nan)
    has = np.flatnonzero(end > start)
    if has.size:                                        # a row's smallest (D2, label); rows without pairs hold none of the list
        key = (pairs[:, 1].astype(np.int64) << 21) | pairs[:, 0].astype(np.int64)
        best = np.minimum.reduceat(key, start[has])
        near_label[has] = (best & ((1 << 21) - 1)).astype(np.int32)
        near_d[has] = np.sqrt((best >> 21).astype(np.float64))
    l1, l2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    d1, d2, ang = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    label = (row + 1).astype(np.int32)
    bounds = np.flatnonzero(np.r_[True, img[1:] != img[:-1], True]) if n else np.zeros(1, np.int64)
    for s, e in zip(bounds[:-1], bounds[1:]):           # image by image
        i1, d1[s:e], i2, d2[s:e], ang[s:e] = _closest_two(centroid[s:e])
        l1[s:e] = np.where(i1 >= 0, label[s:e][np.maximum(i1, 0)], 0)
        l2[s:e] = np.where(i2 >= 0, label[s:e][np.maximum(i2, 0)], 0)
    return NeighborTable(image=img.astype(np.int32), label=label, area=area, centroid=centroid, border=ob[:, 0].copy(),
                         touching=ob[:, 1].copy(), number_of_neighbors=ob[:, 2].copy(),
                         percent_touching=100.0 * ob[:, 1].astype(np.float64) / ob[:, 0].astype(np.float64),
                         nearest_edge_label=near_label, nearest_edge_distance=near_d, first_closest_label=l1, first_closest_distance=d1,
                         second_closest_label=l2, second_closest_distance=d2, angle_between_neighbors=ang, geom=g, objects=ob,
                         row_start=start.copy(), row_end=end.copy(), pairs=pairs)


class NeighborMeasurer(LabelTool):
    """cs_label_neighbors on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter) whose
    handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read in stream
    order."""
    _noun = "the measurer"

    # ---- argument checks: everything is refused before the device is touched ----
    def _check(self, labels, max_label):
        check_label_plane("labels", labels, self.device_id, self._noun)
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

    def measure_dense(self, labels, distance, max_label=None, table_log2: int = 0):
        """The records as the device writes them, numpy on the host: geom int64 [B,max_label,3], objects int32 [B,max_label,3]
        (border, touching, degree), offsets int64 [B * max_label + 1] and pairs int32 [n_pairs,3] (neighbour label, D2, n_near), row
        b * max_label + label - 1 for a label of image b; the rows of an absent object are all zero and its CSR row is empty.
        Arguments as measure_batch; table_log2 as neighbor_params."""
        params = neighbor_params(distance, table_log2)
        B, H, W, on_dev = self._check(labels, max_label)
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label)
        max_label = int(max_label)
        geom = np.empty((B, max_label, 3), np.int64)
        objects = np.empty((B, max_label, 3), np.int32)
        offsets = np.empty(B * max_label + 1, np.int64)
        n = C.c_int64(0)
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, labels)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_neighbors(self._handle, L._ptr(labels), B, H, W, kind, max_label, C.byref(params), L._ptr(geom),
                                             L._ptr(objects), L._ptr(offsets), L.CS_MEM_HOST, C.byref(n)))
        pairs = np.empty((n.value, 3), np.int32)
        if n.value:
            L.check(self._lib.cs_label_neighbors_pairs(self._handle, L._ptr(pairs), n.value, L.CS_MEM_HOST))
        return geom, objects, offsets, pairs

    def measure_batch(self, labels, distance, max_label=None) -> NeighborTable:
        """labels: int32 [B,H,W], 0 is background; a numpy array or a CUDA tensor of the measurer's device.  distance: a number of
        pixels in 1..32 (neighbor_params).  max_label: an upper bound of the labels (it sizes the device tables), None: their
        maximum.  Returns the NeighborTable of the objects present, in (image, label) order.  A negative label, or one above
        max_label, raises CellScreenError (CS_ERR_INVALID); the measurer stays usable."""
        return neighbor_table(*self.measure_dense(labels, distance, max_label))

    def last_timing(self):
        """Device milliseconds of the last measure_batch: neighbors_scan_ms (clearing and the scan of the disks) and neighbors_rows_ms
        (degrees, offsets, scatter and the sort of the rows)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.cs_label_neighbors_last_timing(self._handle, C.byref(a), C.byref(b)))
        return dict(neighbors_scan_ms=a.value, neighbors_rows_ms=b.value)

    def last_table(self):
        """(table_log2, grows) of the last measure_batch: the capacity its pair table ended with, and how often it was doubled."""
        a, b = C.c_int32(), C.c_int32()
        L.check(self._lib.cs_label_neighbors_last_table(self._handle, C.byref(a), C.byref(b)))
        return a.value, b.value
