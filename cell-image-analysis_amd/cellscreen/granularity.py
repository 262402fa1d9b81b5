"""Per-object granularity spectrum on the device (cs_label_granularity, include/cellscreen.h): the size spectrum of
the bright structures -- speckles, vesicles, foci -- inside every object of a label image, CellProfiler's MeasureGranularity.  The
rule is this project's (tests/granularity_reference.py restates it); it corresponds to that measurement without a promise of bit
equality with CellProfiler.

    t = GranularityMeasurer().measure_batch(image, labels, steps=16)         # image [B,H,W] or [B,H,W,C], C <= 4
    t.spectrum[:, 1, 0]                                                      # step 2 of channel 0: structures about 3 px wide
    t.image_spectrum[:, :, 0]                                                # the same per image, CellProfiler's Granularity_k

An object is IntensityMeasurer's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
is non-zero.  Per channel the working plane P is the image (subsample 1) or its rounded s x s block means, P[R][C] = (2 sum v +
n) // (2 n) over the block's n in-image pixels; with masked=True a pixel off the objects counts as 0 in it.  For k = 1..steps, E_k
is the erosion of E_(k-1) by the 3 x 3 cross (E_0 = P, neighbours outside the plane ignored) and R_k the reconstruction by
dilation of E_k under P with the same cross; R_0 = P.  The device returns exact integer records, S_k = the sum over the object's
full-resolution pixels (r, c) of R_k[r // s][c // s], and per image the sum of R_k over the working plane; the floats are taken
from them here in Python ints, each one correctly rounded division:

    spectrum[k-1] = 100 (S_(k-1) - S_k) / S_0          start_mean = S_0 / area

NaN where S_0 = 0 (CellProfiler clamps the start mean to eps and reports 0 there).  Deliberate differences from CellProfiler: the
subsampling is an integer block mean read back by the nearest block, not bilinear; there is no background removal (pass a plane
corrected by ThresholdSegmenter.correct_batch); the reconstruction is image-wide, so a bright structure shared by two touching
objects is held up for both, as in CellProfiler.  2-D only, the cross only, at most 4 channels and 64 steps."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._labels import LabelTool
from .intensity import MAX_CHANNELS, IntensityMeasurer

MAX_STEPS = 64                          # CS_GRANULARITY_MAX_STEPS
SUBSAMPLES = (1, 2, 4, 8)
MAX_TABLE_BYTES = 1 << 30               # of the sums table and of the planes stack


def granularity_params(steps=16, subsample=1, masked=False) -> "L.CSGranularityParams":
    """cs_granularity_params of a call: steps 1..64, subsample 1, 2, 4 or 8, masked a bool."""
    for name, v in (("steps", steps), ("subsample", subsample)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
    if not isinstance(masked, (bool, np.bool_)):
        raise TypeError(f"masked must be a bool, got {type(masked).__name__}")
    if not 1 <= int(steps) <= MAX_STEPS:
        raise ValueError(f"steps {steps}: must be in 1..{MAX_STEPS}")
    if int(subsample) not in SUBSAMPLES:
        raise ValueError(f"subsample {subsample}: must be one of {SUBSAMPLES}")
    p = L.CSGranularityParams()
    p.steps, p.subsample, p.masked, p.reserved = int(steps), int(subsample), int(bool(masked)), 0
    return p


@dataclass
class GranularityTable:
    """The objects present in a batch, in (image, label) order; n objects, K steps, C channels, B images.  All numpy arrays on the
    host.  The floats are NaN where S_0 = 0."""
    image: np.ndarray                   # [n] int32: the image of the batch
    label: np.ndarray                   # [n] int32
    area: np.ndarray                    # [n] int64
    start_mean: np.ndarray              # [n,C] float64: S_0 / area
    spectrum: np.ndarray                # [n,K,C] float64: 100 (S_(k-1) - S_k) / S_0
    image_spectrum: np.ndarray          # [B,K,C] float64: the same of the working plane's sums
    geom: np.ndarray                    # [n,3] int64: area, sum r, sum c
    sums: np.ndarray                    # [n,K+1,C] int64: S_0 .. S_K
    image_sums: np.ndarray              # [B,K+1,C] int64

    def __len__(self):
        return int(self.label.shape[0])


def _spectrum(s) -> np.ndarray:
    """s: int64 [m, K+1, C] -> float64 [m, K, C], Python ints in between."""
    m, k1, nc = s.shape
    out = np.full((m, k1 - 1, nc), np.nan)
    for i in range(m):
        for ch in range(nc):
            v = [int(x) for x in s[i, :, ch]]
            if v[0] != 0:
                for k in range(1, k1):
                    out[i, k - 1, ch] = (100 * (v[k - 1] - v[k])) / v[0]       # Python ints: correctly rounded
    return out


def derive(geom, sums, image_sums) -> dict:
    """The values a GranularityTable reports, from the dense tables cs_label_granularity writes: geom [B,max_label,3], sums
    [B,max_label,K+1,C] and image_sums [B,K+1,C], int64.  The rows of absent objects (area 0) are dropped.  A pure host function."""
    geom, sums, image_sums = np.asarray(geom), np.asarray(sums), np.asarray(image_sums)
    if geom.dtype != np.int64 or sums.dtype != np.int64 or image_sums.dtype != np.int64:
        raise TypeError("geom, sums and image_sums must be int64")
    if (geom.ndim != 3 or geom.shape[2] != 3 or sums.ndim != 4 or sums.shape[:2] != geom.shape[:2] or not 2 <= sums.shape[2] <= MAX_STEPS + 1 or
            not 1 <= sums.shape[3] <= MAX_CHANNELS or image_sums.shape != (geom.shape[0],) + sums.shape[2:]):
        raise ValueError(f"geom {geom.shape}, sums {sums.shape}, image_sums {image_sums.shape}: [B,max_label,3], [B,max_label,K+1,C] and "
                         "[B,K+1,C] expected")
    img, row = np.nonzero(geom[:, :, 0] > 0)
    g, s = geom[img, row], sums[img, row]
    n, nc = g.shape[0], sums.shape[3]
    start = np.full((n, nc), np.nan)
    for i in range(n):
        for ch in range(nc):
            if int(s[i, 0, ch]) != 0:
                start[i, ch] = int(s[i, 0, ch]) / int(g[i, 0])
    return dict(image=img.astype(np.int32), label=(row + 1).astype(np.int32), area=g[:, 0].copy(), start_mean=start, spectrum=_spectrum(s),
                image_spectrum=_spectrum(image_sums), geom=g, sums=s, image_sums=image_sums.copy())


def granularity_table(geom, sums, image_sums) -> GranularityTable:
    """The table of the dense tables cs_label_granularity writes (derive names them)."""
    return GranularityTable(**derive(geom, sums, image_sums))


class GranularityMeasurer(LabelTool):
    """cs_label_granularity on one preprocess handle (one GPU, one stream).  extractor: a CellExtractor (or a ThresholdSegmenter)
    whose handle and stream to share, so that labels a segmenter or a LabelExpander on that handle left on the device are read
    in stream order.  The argument checks of the planes are IntensityMeasurer's, in its order."""
    _noun = "the measurer"
    _check = IntensityMeasurer._check
    _check_size = staticmethod(IntensityMeasurer._check_size)
    MAX_STEPS = MAX_STEPS

    def measure_dense(self, image, labels, exclude=None, steps=16, subsample=1, masked=False, max_label=None, want_planes=False):
        """The dense tables as the device writes them, numpy on the host: geom int64 [B,max_label,3], sums int64
        [B,max_label,steps+1,C] and image_sums int64 [B,steps+1,C], row label - 1 for a label; the rows of an absent object are all
        zero.  With want_planes a fourth: the planes R_0..R_steps, uint16 [B,steps+1,C,Hs,Ws].  Arguments as measure_batch."""
        B, H, W, nc, ptype, on_dev = self._check(image, labels, exclude, max_label)
        prm = granularity_params(steps, subsample, masked)
        if not isinstance(want_planes, (bool, np.bool_)):
            raise TypeError(f"want_planes must be a bool, got {type(want_planes).__name__}")
        if max_label is None:
            max_label = max(1, int(labels.max()))       # a batch without objects still runs: it reports a negative label
            self._check_size(B, max_label, nc)
        max_label = int(max_label)
        k1, s = prm.steps + 1, prm.subsample
        hs, ws = -(-H // s), -(-W // s)
        if B * max_label * k1 * nc * 8 > MAX_TABLE_BYTES:
            raise ValueError(f"batch {B} x max_label {max_label} x steps {prm.steps} x channels {nc}: the sums table would exceed "
                             f"{MAX_TABLE_BYTES} bytes, split the batch")
        if want_planes and B * k1 * nc * hs * ws * 2 > MAX_TABLE_BYTES:
            raise ValueError(f"batch {B} x steps {prm.steps} x channels {nc} x {hs} x {ws}: the planes stack would exceed "
                             f"{MAX_TABLE_BYTES} bytes, split the batch")
        geom = np.empty((B, max_label, 3), np.int64)
        sums = np.empty((B, max_label, k1, nc), np.int64)
        image_sums = np.empty((B, k1, nc), np.int64)
        planes = np.empty((B, k1, nc, hs, ws), np.uint16) if want_planes else None
        if on_dev:
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, image, labels, exclude)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(self._lib.cs_label_granularity(self._handle, L._ptr(image), ptype, nc, L._ptr(labels), L._ptr(exclude), B, H, W, kind,
                                               max_label, C.byref(prm), L._ptr(geom), L._ptr(sums), L._ptr(image_sums), L._ptr(planes),
                                               L.CS_MEM_HOST))
        return (geom, sums, image_sums, planes) if want_planes else (geom, sums, image_sums)

    def measure_batch(self, image, labels, exclude=None, steps=16, subsample=1, masked=False, max_label=None) -> GranularityTable:
        """image: [B,H,W] or [B,H,W,C] uint8 / uint16 with C <= 4; labels, exclude, max_label: as
        IntensityMeasurer.measure_batch.  steps: the length of the spectrum, 1..64.  subsample: 1, 2, 4 or 8, the side of the blocks
        whose means make the working plane.  masked: pixels off the objects count as 0 in the working plane.  Returns the
        GranularityTable of the objects present, in (image, label) order.  A negative label, or one above max_label, raises
        CellScreenError (CS_ERR_INVALID); the measurer stays usable."""
        return granularity_table(*self.measure_dense(image, labels, exclude, steps, subsample, masked, max_label))

    def last_timing(self):
        """Device milliseconds of the last measure_batch: granularity_prepare_ms (with the clearing), granularity_steps_ms (the
        erosions with their reconstructions) and granularity_sums_ms (the steps + 1 sums passes)."""
        v = [C.c_double() for _ in range(3)]
        L.check(self._lib.cs_label_granularity_last_timing(self._handle, *(C.byref(x) for x in v)))
        return dict(zip(("granularity_prepare_ms", "granularity_steps_ms", "granularity_sums_ms"), (x.value for x in v)))

    def last_rounds(self):
        """(rounds, reads) of the last measure_batch: the reconstruction rounds of all steps together, and the reads of the control
        word (one host synchronisation each)."""
        a, b = C.c_int32(), C.c_int32()
        L.check(self._lib.cs_label_granularity_last_rounds(self._handle, C.byref(a), C.byref(b)))
        return a.value, b.value
