"""The built-in segmenter on the GPU (csrc/segment.hip): a global threshold (Otsu's, or a fixed one), optional hole filling
and connected-component labelling, from the segmentation channel of an image stack to int32 label images that
cellscreen.extract reads without a copy through the host.

It is NOT StarDist and does not try to be: it is a classical segmenter for bright cells on a dark background.  By default
cells that touch come out as one region, which the extraction's area and eccentricity rules then judge like any other region.
With split_touching=True such regions are cut at their necks by an exact integer distance-transform watershed
(cs_segment_split; tests/split_reference.py restates it): seeds are the maxima of the distance to the background that stand
split_h half pixels above their saddles.  Cells that overlap without a neck, and cores deeper than 127 px, stay whole under
that rule (it sees the mask alone); with connectivity 2 the cut between two equal cells is skewed, so connectivity 1 stays the
default.
split_by="intensity" (with split_touching=True) is for the cells without a neck: the same watershed on heights taken from the
image (cs_segment_split_intensity; tests/split_intensity_reference.py restates it).  Each component's own range of the plane
the threshold saw (after smooth_sigma and background_radius) is stretched to 254 levels, Hq = 1 + (G - lo) * 254 // max(hi - lo,
split_contrast, 1), and two bright cores are cut apart along the valley between them when it lies split_depth levels below the
lower core.  The scale is per component, so a dim cell beside a bright field keeps its own 254 levels and nothing depends on
the rest of the batch; a component flatter than split_contrast counts is not stretched, the guard against splitting on noise.
It needs a smoothed plane: pass smooth_sigma (1.5 on the scene it was specified on), because on a noisy plane every noise peak
deeper than split_depth is a seed and a cell shatters into dozens of regions.  And cells that overlap in projection add up,
so the lens between two cores can be the brightest spot and come out as a third region.
What it computes is exact: the threshold is scikit-image 0.18.3's threshold_otsu of the channel (an integer), the mask is
`channel > threshold` (after scipy.ndimage.binary_fill_holes with fill_holes), and the labels are scipy.ndimage.label's
(= skimage.measure.label's) ids, as restated in tests/segment_reference.py; neither library is a dependency.

One global threshold needs a flat background.  Where the illumination is uneven (vignetting, a tilted coverslip, haze: a
background slope larger than the cells' own contrast) pass background_radius=r: the channel is first corrected on the device by
a white top-hat with the flat square of side 2r + 1 (cs_segment_background; scipy.ndimage.white_tophat bit for bit, restated in
tests/background_reference.py), after an optional 3 x 3 median (denoise=True), and the threshold, the labels and the split see
the corrected plane.  r must exceed half the width of the widest cell (r >= 51 for cells up to the extraction's 8000 px area
limit); a smaller r eats the cores of the cells.  Off by default, and only the segmentation channel is corrected: the
extraction's intensity rules and crops read the raw analysis channel.

One global threshold also needs cells of one brightness.  Where bright and dim cells share a field, Otsu's threshold settles
between the background and the bright ones and the dim cells are never found.  threshold="local" with local_radius=r cuts every
pixel against the mean of its own (2r + 1)^2 neighbourhood instead (cs_segment_local; tests/local_reference.py restates it):
foreground is  n * x - S - n * local_delta > 0  and  x > local_floor, S the window's sum with the image reflected about its
edges, n = (2r + 1)^2.  That is x > skimage.filters.threshold_local(x, 2r + 1, method='mean', offset=-local_delta) decided in
integers; the one difference is an exact tie, n * (x - local_delta) = S, which is background here while the library's float64
mean may fall on either side.  The window must be wider than the widest cell, as the top-hat's square, or a cell's core sits
near its own mean and drops out.  Noise on empty background passes a small local_delta as speckle: hundreds of regions of a
few pixels per field, each labelled, numbered and measured before the extraction's area rule drops it, and the label count
rises towards the extraction's limit (batch * max_label <= 2^22).  min_area (below) removes them before the labelling;
denoise=True and a local_delta of a few noise sigmas make fewer of them.  The mask feeds the same hole filling, labelling and
split; with background_radius the local rule runs on the corrected plane.

Hysteresis threshold, in the place of the plain cut or of the local rule (cs_segment_hysteresis; tests/hysteresis_reference.py
restates it), off by default.  One number per pixel leaves a choice between two evils: set low, noise passes as speckle, and
min_area, which goes by size, takes a small real object with it; set high, the speckle is gone and so is every cell's dim rim,
and the regions the extraction measures are smaller than the cells.  Two numbers end it: a pixel is foreground if it passes the
weak rule and is connected, through pixels that pass it too, to a pixel that passes the strong rule, which is
skimage.filters.apply_hysteresis_threshold decided in integers.  The strong rule is the one the segmenter has anyway.  The weak
one has the same form with a lower number: weak_threshold as an int is in counts, low = min(weak_threshold, t); as a float
strictly between 0 and 1 it is a fraction of the strong threshold, low = (t * q) >> 16 with q = int(f * 65536 + 0.5), the form
for Otsu, whose t is not known in advance; with threshold="local" weak_delta stands in local_delta's place (same window, floor
and tie rule).  Components are taken under the segmenter's connectivity; speckle has no strong pixel and goes whatever its
size, a cell keeps its whole weak extent.  The hole filling, the cleanup, the labels and the split see the resulting 0 / 1
plane; the thresholds reported stay the strong rule's.  The low number is never chosen automatically.

Noise-adaptive threshold, threshold="noise", in the place of all of the above rules (cs_segment_noise; tests/noise_reference.py
restates it).  Every other rule takes its numbers in counts, which do not travel between exposures, cameras, bit depths or even
the fields of one plate; the one unit that does is the image's own background noise.  The background level and the noise are
estimated on a mesh of noise_tile x noise_tile tiles with robust statistics (the median, and 1.4826 times the median absolute
deviation, not below noise_floor counts), each map is median-filtered over 3 x 3 tiles (a tile that a cell fills is rejected)
and interpolated bilinearly to every pixel, and foreground is  x > background + noise_k * sigma, decided in 64-bit integers
with noise_k in 1/256 (an exact tie is background), as SExtractor and photutils' Background2D cut.  It follows a sloping
background without the top-hat, and weak_k (not above noise_k) is the weak rule of the hysteresis threshold above: noise_k=6,
weak_k=3 keeps whole cells and no speckle.  The tile must stay well above a cell's width; a slope inside a tile inflates the
sigma, and a field so crowded that most tiles are mostly cell biases both maps upward.  The thresholds reported are -1.

Mask cleanup, between the hole filling and the labels (cs_segment_clean; tests/clean_reference.py restates it), off by default:
open_radius=r (1..15) opens the mask, r erosions then r dilations by the 3 x 3 square (open_connectivity=2, the default) or
cross (1), which is scipy.ndimage.binary_opening(mask, generate_binary_structure(2, k), iterations=r) bit for bit: speckle and
bridges thinner than 2r + 1 pixels go, and the square rounds a disk's diagonal edge by about 0.4 * r px.  min_area=a then turns
components (under the segmenter's connectivity) of fewer than a pixels into background, as
skimage.morphology.remove_small_objects(mask, min_size=a) does.  The labels, the split and the distances see the cleaned mask.

Smoothing, before everything else (cs_segment_smooth; tests/smooth_reference.py restates it), off by default: smooth_sigma=s
(0.25..15.875) replaces the channel by its Gaussian, for noisy fields where the threshold shatters a faint cell into fragments
that no cleanup of the mask puts together again.  Integers only: a separable kernel of radius int(4 s + 0.5) with 16-bit
fixed-point weights that sum to 2^16 (smooth_weights), the image reflected about its edges, one rounding to nearest at the very
end.  That is scipy.ndimage.gaussian_filter(x, s, mode='reflect', truncate=4.0) in float64 to within 0.5 + top * (2 eps + eps^2),
eps the summed quantisation error of the taps; the library's own integer output truncates and is not reproduced bit for bit.
denoise=True then runs the 3 x 3 median before the Gaussian (hot pixels go before they are smeared) and nowhere else; the
correction, the threshold, the cleanup, the labels and the split see the smoothed plane, the extraction the raw channel.

    seg = ThresholdSegmenter()
    labels, n_labels, thresholds = seg.segment_batch(images)          # numpy in, numpy out; CUDA tensors in, CUDA tensor out
    seg = ThresholdSegmenter(split_touching=True)                      # the same, touching cells apart
    seg = ThresholdSegmenter(split_touching=True, split_by="intensity", smooth_sigma=1.5)     # ... cells without a neck too
    seg = ThresholdSegmenter(background_radius=51)                     # uneven illumination flattened before the threshold
    seg = ThresholdSegmenter(threshold="local", local_radius=25, local_delta=60)      # bright and dim cells in one field
    seg = ThresholdSegmenter(threshold="local", local_radius=25, local_delta=40, min_area=50)         # ... without the speckle
    seg = ThresholdSegmenter(smooth_sigma=2)                           # faint cells in noise: Gaussian first
    seg = ThresholdSegmenter(threshold="local", local_radius=25, local_delta=200, weak_delta=40)      # no speckle, whole cells
    seg = ThresholdSegmenter(weak_threshold=0.2)                       # Otsu's threshold for the cores, a fifth of it for the rims
    seg = ThresholdSegmenter(threshold="noise")                        # 5 sigmas above the local background, no number in counts
    seg = ThresholdSegmenter(threshold="noise", noise_k=6, weak_k=3)   # ... cores at 6 sigmas, rims down to 3, no speckle
    stats, labels, n_labels = seg.score_batch(images, truth)           # how good any of these is against true labels: score.py
    seg = ThresholdSegmenter(expand_distance=6)                        # a nuclear stain segmented, the labels grown 6 px: expand.py

    screening = ProductionMutantScreening(model_dir, cell_extractor=threshold_cell_extractor())
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _lib as L
from ._labels import MAX_BATCH, MAX_SIDE, _is_tensor, check_label_plane, check_stack_shape  # noqa: F401
from .extract import IMAGE_NO_CELLS, IMAGE_OK, CellExtractor, qc_params, read_image, region_stats, split_channels
from .preprocess import OUT_SIDE, PIX_U8, PIX_U16, Preprocessor, check_out_hw
from .expand import LabelExpander, expand_params
from .score import THRESHOLDS as SCORE_THRESHOLDS, LabelMatcher, check_thresholds


def segment_params(threshold="otsu", connectivity: int = 1, fill_holes: bool = True) -> L.CSSegmentParams:
    """cs_segment_params from the Python arguments; anything out of range raises before a handle exists."""
    p = L.CSSegmentParams()
    if isinstance(threshold, str):
        if threshold != "otsu":
            raise ValueError(f"threshold must be 'otsu' or an integer, got {threshold!r}")
        p.threshold_mode, p.threshold = L.THRESH_OTSU, 0
    else:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)):
            raise TypeError(f"threshold must be 'otsu' or an integer, got {type(threshold).__name__}")
        if not 0 <= int(threshold) <= 65535:
            raise ValueError(f"threshold {threshold} outside 0..65535")
        p.threshold_mode, p.threshold = L.THRESH_FIXED, int(threshold)
    if isinstance(connectivity, bool) or connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (4 neighbours) or 2 (8 neighbours), got {connectivity!r}")
    p.connectivity = int(connectivity)
    p.fill_holes = 1 if fill_holes else 0
    return p


def split_params(split_touching: bool = False, split_h: int = 3) -> Optional[L.CSSplitParams]:
    """cs_split_params from the Python arguments, None without split_touching; anything out of range raises before a handle
    exists (also without split_touching: a bad split_h is a mistake either way)."""
    if not isinstance(split_touching, (bool, np.bool_)):
        raise TypeError(f"split_touching must be a bool, got {type(split_touching).__name__}")
    if isinstance(split_h, bool) or not isinstance(split_h, (int, np.integer)):
        raise TypeError(f"split_h must be an integer (half pixels), got {type(split_h).__name__}")
    if not 1 <= int(split_h) <= 255:
        raise ValueError(f"split_h {split_h} outside 1..255")
    if not split_touching:
        return None
    p = L.CSSplitParams()
    p.h = int(split_h)
    return p


SPLIT_DEPTH, SPLIT_CONTRAST = 16, 0                       # the defaults of split_by="intensity"


def split_intensity_params(split_touching: bool = False, split_by="distance", split_h: int = 3, split_depth: int = SPLIT_DEPTH,
                           split_contrast: int = SPLIT_CONTRAST) -> Optional[L.CSSplitIntensityParams]:
    """cs_split_intensity_params from the Python arguments, None with split_by="distance"; anything out of range raises before
    a handle exists.  split_depth and split_contrast belong to "intensity" alone, split_h to "distance" alone, and "intensity"
    needs split_touching=True: it is a way of splitting, not a switch of its own."""
    if not isinstance(split_by, str):
        raise TypeError(f"split_by must be 'distance' or 'intensity', got {type(split_by).__name__}")
    if split_by not in ("distance", "intensity"):
        raise ValueError(f"split_by must be 'distance' or 'intensity', got {split_by!r}")
    for name, v in (("split_depth", split_depth), ("split_contrast", split_contrast)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
    if not 1 <= int(split_depth) <= 254:
        raise ValueError(f"split_depth {split_depth} outside 1..254")
    if not 0 <= int(split_contrast) <= 65535:
        raise ValueError(f"split_contrast {split_contrast} outside 0..65535")
    if split_by == "distance":
        if int(split_depth) != SPLIT_DEPTH or int(split_contrast) != SPLIT_CONTRAST:
            raise ValueError("split_depth and split_contrast belong to split_by='intensity'")
        return None
    if not split_touching:
        raise ValueError("split_by='intensity' needs split_touching=True")
    if split_h != 3:
        raise ValueError("split_h belongs to split_by='distance'; the intensity split takes split_depth")
    p = L.CSSplitIntensityParams()
    p.depth, p.min_contrast = int(split_depth), int(split_contrast)
    return p


def background_params(background_radius=None, denoise: bool = False) -> Optional[L.CSBackgroundParams]:
    """cs_background_params from the Python arguments, None without a radius (no correction); anything out of range raises
    before a handle exists.  denoise (the 3 x 3 median) is part of the correction: without a radius it is an error."""
    if not isinstance(denoise, (bool, np.bool_)):
        raise TypeError(f"denoise must be a bool, got {type(denoise).__name__}")
    if background_radius is None:
        if denoise:
            raise ValueError("denoise=True needs background_radius: the median is a step of the background correction")
        return None
    if isinstance(background_radius, bool) or not isinstance(background_radius, (int, np.integer)):
        raise TypeError(f"background_radius must be None or an integer (pixels), got {type(background_radius).__name__}")
    if not 1 <= int(background_radius) <= 255:
        raise ValueError(f"background_radius {background_radius} outside 1..255")
    p = L.CSBackgroundParams()
    p.radius, p.median = int(background_radius), 1 if denoise else 0
    return p


def local_params(local_radius=None, local_delta: int = 0, local_floor: int = -1, denoise: bool = False) -> L.CSLocalParams:
    """cs_local_params from the Python arguments of threshold="local"; anything out of range (a missing radius among them)
    raises before a handle exists.  denoise: the 3 x 3 median before the sums."""
    if not isinstance(denoise, (bool, np.bool_)):
        raise TypeError(f"denoise must be a bool, got {type(denoise).__name__}")
    if local_radius is None:
        raise ValueError("threshold='local' needs local_radius: the window has side 2 * local_radius + 1")
    for name, v in (("local_radius", local_radius), ("local_delta", local_delta), ("local_floor", local_floor)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
    if not 1 <= int(local_radius) <= 255:
        raise ValueError(f"local_radius {local_radius} outside 1..255")
    if not -65535 <= int(local_delta) <= 65535:
        raise ValueError(f"local_delta {local_delta} outside -65535..65535")
    if not -1 <= int(local_floor) <= 65535:
        raise ValueError(f"local_floor {local_floor} outside -1..65535 (-1: off)")
    p = L.CSLocalParams()
    p.radius, p.delta, p.floor, p.median = int(local_radius), int(local_delta), int(local_floor), 1 if denoise else 0
    return p


MAX_OPEN_RADIUS, MAX_MIN_AREA = 15, 1 << 24


def clean_params(open_radius=None, open_connectivity: int = 2, min_area=None) -> Optional[L.CSCleanParams]:
    """cs_clean_params from the Python arguments, None with neither step (no cleanup); anything out of range raises before a
    handle exists.  open_connectivity is checked also without open_radius: alone it is a default, not a request."""
    for name, v in (("open_radius", open_radius), ("min_area", min_area)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise TypeError(f"{name} must be None or an integer, got {type(v).__name__}")
    if isinstance(open_connectivity, bool) or not isinstance(open_connectivity, (int, np.integer)):
        raise TypeError(f"open_connectivity must be 1 (cross) or 2 (square), got {type(open_connectivity).__name__}")
    if open_connectivity not in (1, 2):
        raise ValueError(f"open_connectivity must be 1 (cross) or 2 (square), got {open_connectivity!r}")
    if open_radius is not None and not 1 <= int(open_radius) <= MAX_OPEN_RADIUS:
        raise ValueError(f"open_radius {open_radius} outside 1..{MAX_OPEN_RADIUS}")
    if min_area is not None and not 1 <= int(min_area) <= MAX_MIN_AREA:
        raise ValueError(f"min_area {min_area} outside 1..{MAX_MIN_AREA}")
    if open_radius is None and min_area is None:
        return None
    p = L.CSCleanParams()
    p.open_radius, p.open_connectivity, p.min_area = int(open_radius or 0), int(open_connectivity), int(min_area or 0)
    return p


def hysteresis_params(threshold="otsu", weak_threshold=None, weak_delta=None, local_delta: int = 0) -> Optional[L.CSHysteresisParams]:
    """cs_hysteresis_params from the Python arguments, None with neither option (no hysteresis); anything out of range or in
    the wrong combination raises before a handle exists.  weak_threshold belongs to the global rules: an int in 0..65535 is
    absolute (with a fixed threshold not above it), a float strictly between 0 and 1 a fraction of the strong threshold, kept as
    q = int(f * 65536 + 0.5) in 1..65535.  weak_delta belongs to threshold="local": an int in -65535..65535, not above
    local_delta."""
    local = isinstance(threshold, str) and threshold == "local"
    if weak_threshold is None and weak_delta is None:
        return None
    if weak_threshold is not None and weak_delta is not None:
        raise ValueError("weak_threshold and weak_delta exclude each other: one weak rule")
    p = L.CSHysteresisParams()
    if weak_delta is not None:
        if isinstance(weak_delta, (bool, np.bool_)) or not isinstance(weak_delta, (int, np.integer)):
            raise TypeError(f"weak_delta must be None or an integer, got {type(weak_delta).__name__}")
        if not local:
            raise ValueError("weak_delta belongs to threshold='local'; the global rules take weak_threshold")
        if not -65535 <= int(weak_delta) <= 65535:
            raise ValueError(f"weak_delta {weak_delta} outside -65535..65535")
        if int(weak_delta) > int(local_delta):
            raise ValueError(f"weak_delta {weak_delta} above local_delta {local_delta}: the weak rule is the lower one")
        p.mode, p.weak = L.WEAK_LOCAL, int(weak_delta)
        return p
    if isinstance(weak_threshold, (bool, np.bool_)) or not isinstance(weak_threshold, (int, float, np.integer, np.floating)):
        raise TypeError(f"weak_threshold must be None, an integer (counts) or a float (fraction), got {type(weak_threshold).__name__}")
    if local:
        raise ValueError("weak_threshold belongs to the global rules; threshold='local' takes weak_delta")
    if isinstance(weak_threshold, (int, np.integer)):
        if not 0 <= int(weak_threshold) <= 65535:
            raise ValueError(f"weak_threshold {weak_threshold} outside 0..65535")
        if not isinstance(threshold, str) and int(weak_threshold) > int(threshold):
            raise ValueError(f"weak_threshold {weak_threshold} above threshold {threshold}: the weak rule is the lower one")
        p.mode, p.weak = L.WEAK_ABSOLUTE, int(weak_threshold)
        return p
    f = float(weak_threshold)
    if not 0.0 < f < 1.0:                                                       # NaN fails both
        raise ValueError(f"weak_threshold {weak_threshold}: a fraction lies strictly between 0 and 1")
    q = int(f * 65536 + 0.5)
    if not 1 <= q <= 65535:
        raise ValueError(f"weak_threshold {weak_threshold} rounds to {q} / 65536, outside 1..65535")
    p.mode, p.weak = L.WEAK_FRACTION, q
    return p


NOISE_K, NOISE_TILE, NOISE_FLOOR = 5.0, 64, 1.0           # the defaults of threshold="noise"
NOISE_TILES = (16, 32, 64, 128, 256)
NOISE_K8_MAX, NOISE_FLOOR_MAX = 16383, 4095


def noise_params(noise_k=NOISE_K, noise_tile: int = NOISE_TILE, noise_floor=NOISE_FLOOR, weak_k=None,
                 connectivity: int = 1) -> L.CSNoiseParams:
    """cs_noise_params from the Python arguments of threshold="noise"; anything out of range raises before a handle exists.
    noise_k and weak_k are kept in 1/256, k8 = int(k * 256 + 0.5) in 1..16383 with weak_k8 not above k8; noise_floor (counts,
    0..4095) as floor8 = int(f * 256 + 0.5); noise_tile is a power of two in 16..256."""
    def number(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{name} must be a number, got {type(v).__name__}")
        if math.isnan(float(v)) or math.isinf(float(v)):
            raise ValueError(f"{name} {v} is not a finite number")
        return float(v)

    k = number("noise_k", noise_k)
    f = number("noise_floor", noise_floor)
    if isinstance(noise_tile, (bool, np.bool_)) or not isinstance(noise_tile, (int, np.integer)):
        raise TypeError(f"noise_tile must be an integer, got {type(noise_tile).__name__}")
    if int(noise_tile) not in NOISE_TILES:
        raise ValueError(f"noise_tile {noise_tile}: a power of two in 16..256")
    k8 = int(k * 256 + 0.5) if 0.0 < k < 1e6 else 0
    if not 1 <= k8 <= NOISE_K8_MAX:
        raise ValueError(f"noise_k {noise_k} is {k8} / 256, outside 1..{NOISE_K8_MAX} / 256")
    if not 0.0 <= f <= NOISE_FLOOR_MAX:
        raise ValueError(f"noise_floor {noise_floor} outside 0..{NOISE_FLOOR_MAX}")
    weak8 = -1
    if weak_k is not None:
        w = number("weak_k", weak_k)
        weak8 = int(w * 256 + 0.5) if 0.0 < w < 1e6 else 0
        if not 1 <= weak8 <= k8:
            raise ValueError(f"weak_k {weak_k} is {weak8} / 256, outside 1..{k8} / 256 (noise_k): the weak rule is the lower one")
    if isinstance(connectivity, bool) or connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (4 neighbours) or 2 (8 neighbours), got {connectivity!r}")
    p = L.CSNoiseParams()
    p.tile, p.k8, p.weak_k8, p.floor8, p.connectivity = int(noise_tile), k8, weak8, int(f * 256 + 0.5), int(connectivity)
    return p


def _noise_mode(threshold, connectivity=1, noise_k=NOISE_K, noise_tile=NOISE_TILE, noise_floor=NOISE_FLOOR, weak_k=None,
                weak_threshold=None, weak_delta=None) -> Optional[L.CSNoiseParams]:
    """cs_noise_params of a segmenter's arguments, None without threshold="noise".  noise_k, noise_tile, noise_floor and weak_k
    belong to "noise" alone; with it the weak rule is weak_k, and weak_threshold and weak_delta are refused."""
    if not (isinstance(threshold, str) and threshold == "noise"):
        noise_params(noise_k, noise_tile, noise_floor, weak_k)                  # a bad value is a mistake either way
        if float(noise_k) != NOISE_K or int(noise_tile) != NOISE_TILE or float(noise_floor) != NOISE_FLOOR or weak_k is not None:
            raise ValueError("noise_k, noise_tile, noise_floor and weak_k belong to threshold='noise'")
        return None
    if weak_threshold is not None or weak_delta is not None:
        raise ValueError("weak_threshold and weak_delta belong to the other rules; threshold='noise' takes weak_k")
    return noise_params(noise_k, noise_tile, noise_floor, weak_k, connectivity)


SMOOTH_SIGMA_MIN, SMOOTH_SIGMA_MAX = 0.25, 15.875         # radius int(4 sigma + 0.5) = 1..64


def smooth_weights(sigma: float, truncate: float = 4.0):
    """The fixed-point Gaussian table w[0..r] of cs_smooth_params, r = int(truncate * sigma + 0.5): w_k = floor(e_k) with
    e_k = 65536 * g_k / (g_0 + 2 * sum g_k), g_k = exp(-k^2 / (2 sigma^2)) in float64; the deficit 65536 - w_0 - 2 * sum w_k
    is handed out by largest remainder over k >= 1 (ties to the smaller k; +1 each, which costs 2) and the centre takes the
    last 0 or 1.  w_0 + 2 * sum_{k >= 1} w_k == 65536, non-increasing from the centre.  tests/smooth_reference.py has an
    identical copy."""
    r = int(truncate * sigma + 0.5)
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(r + 1)]
    norm = g[0] + 2.0 * sum(g[1:])
    e = [65536.0 * gk / norm for gk in g]
    w = [int(math.floor(ek)) for ek in e]
    deficit = 65536 - w[0] - 2 * sum(w[1:])
    for k in sorted(range(1, r + 1), key=lambda k: (-(e[k] - w[k]), k)):
        if deficit < 2:
            break
        w[k] += 1
        deficit -= 2
    w[0] += deficit
    return w


def smooth_params(smooth_sigma=None, denoise: bool = False) -> Optional[L.CSSmoothParams]:
    """cs_smooth_params from the Python arguments, None without a sigma (no smoothing); anything out of range raises before a
    handle exists.  denoise: the 3 x 3 median before the Gaussian."""
    if not isinstance(denoise, (bool, np.bool_)):
        raise TypeError(f"denoise must be a bool, got {type(denoise).__name__}")
    if smooth_sigma is None:
        return None
    if isinstance(smooth_sigma, (bool, np.bool_)) or not isinstance(smooth_sigma, (int, float, np.integer, np.floating)):
        raise TypeError(f"smooth_sigma must be None or a number (pixels), got {type(smooth_sigma).__name__}")
    if not SMOOTH_SIGMA_MIN <= float(smooth_sigma) <= SMOOTH_SIGMA_MAX:                  # NaN fails both
        raise ValueError(f"smooth_sigma {smooth_sigma} outside {SMOOTH_SIGMA_MIN}..{SMOOTH_SIGMA_MAX}")
    w = smooth_weights(float(smooth_sigma))
    p = L.CSSmoothParams()
    p.radius, p.median, p.reserved = len(w) - 1, 1 if denoise else 0, 0
    for k, v in enumerate(w):
        p.weights[k] = v
    return p


def _threshold_mode(threshold, connectivity, fill_holes, local_radius, local_delta, local_floor, background_radius, denoise,
                    smooth_sigma=None):
    """(cs_segment_params, cs_local_params or None, cs_background_params or None) of a segmenter's arguments.  In local mode the
    labelling sees a 0 / 1 plane, so its parameters are a fixed threshold of 0; the median runs once, inside the first stage
    that exists: the smoothing (smooth_params has it then, and the stages here get none), else the correction, else the local
    rule."""
    if smooth_params(smooth_sigma, denoise) is not None:
        denoise = False
    if isinstance(threshold, str) and threshold == "noise":
        # cs_segment_noise makes a 0 / 1 plane, as the local rule: the fixed threshold 0 for what follows
        if local_radius is not None or local_delta != 0 or local_floor != -1:
            raise ValueError("local_radius, local_delta and local_floor belong to threshold='local'")
        return segment_params(0, connectivity, fill_holes), None, background_params(background_radius, denoise)
    if isinstance(threshold, str) and threshold == "local":
        if not isinstance(denoise, (bool, np.bool_)):
            raise TypeError(f"denoise must be a bool, got {type(denoise).__name__}")
        background = background_params(background_radius, bool(denoise) and background_radius is not None)
        local = local_params(local_radius, local_delta, local_floor, bool(denoise) and background is None)
        return segment_params(0, connectivity, fill_holes), local, background
    if local_radius is not None or local_delta != 0 or local_floor != -1:
        raise ValueError("local_radius, local_delta and local_floor belong to threshold='local'")
    return segment_params(threshold, connectivity, fill_holes), None, background_params(background_radius, denoise)


class ThresholdSegmenter:
    """Threshold + connected components on one preprocess handle (one GPU, one stream).  threshold: "otsu" (per image) or an
    integer; foreground is pixel > threshold.  connectivity: 1 (4 neighbours) or 2 (8).  fill_holes: background enclosed
    by foreground becomes foreground before labelling.  extractor: a CellExtractor whose handle and stream to share, so
    that labels left on the device feed its extract_batch in stream order.  split_touching: cut touching cells apart
    (cs_segment_split, see the module text); split_h: the depth in half pixels (1..255) a saddle needs below the lower of
    its two peaks to separate them.  split_by: "distance" (that rule) or "intensity" (split_touching=True still switches the
    split on): the heights come from the plane the threshold saw, see the module text; split_depth (1..254 of a component's 254
    levels, default 16: on the specifying scene 8 to 20 give the same regions) is how far below the lower core a valley must lie,
    split_contrast (0..65535 counts) the range below which a component is not stretched.  These two belong to "intensity" alone
    and split_h to "distance" alone.  background_radius: None, or the radius r (1..255) of the white top-hat that flattens the
    channel before the threshold (see the module text); denoise: a 3 x 3 median before the top-hat.  With numpy input the
    corrected plane makes one extra round trip through the host; CUDA tensors are the fast path.
    threshold="local": the local mean threshold of the module text in the global one's place, with local_radius (1..255,
    required), local_delta (counts above the local mean, -65535..65535) and local_floor (pixel > local_floor as well; -1:
    off); these three belong to "local" alone.  denoise then needs no background_radius: the median runs before the sums.  The
    thresholds it reports are -1: there is no single number.  With numpy input the mask makes one more round trip.
    open_radius (None or 1..15), open_connectivity (1 cross, 2 square) and min_area (None or 1..2^24): the mask cleanup of the
    module text, after the hole filling; the labels and the split then see the cleaned mask.  With numpy input the cleaned
    mask makes one more round trip.
    smooth_sigma (None or 0.25..15.875): the Gaussian smoothing of the module text, before everything else; denoise then runs
    the median before the Gaussian and needs no background_radius.  With numpy input the smoothed plane makes one more round
    trip.
    weak_threshold (None, an int in 0..65535: counts, or a float strictly between 0 and 1: a fraction of the strong threshold)
    and, with threshold="local", weak_delta (None or an int in -65535..65535, not above local_delta): the hysteresis threshold
    of the module text, in the place of the plain cut or of the local rule; the threshold (or local_delta) stays the strong
    rule and is what `thresholds` reports.  The hole filling and every later stage see its 0 / 1 plane.  With numpy input that
    plane makes one more round trip through the host, as the other stages' planes do.
    threshold="noise": the noise-adaptive threshold of the module text in the place of all these rules, with noise_k (sigmas
    above the local background, kept in 1/256, default 5), noise_tile (the mesh tile's side, a power of two in 16..256, default
    64), noise_floor (the least sigma in counts, 0..4095, default 1) and weak_k (None, or the weak rule's k, not above noise_k);
    these four belong to "noise" alone, and local_*, weak_threshold and weak_delta are refused with it.  The thresholds it
    reports are -1.  With numpy input its plane makes one more round trip through the host.
    expand_distance (None, or a number of pixels in 1..127): the labels, after the split where there is one, are grown in place
    by that distance on the same handle (cs_label_expand, cellscreen/expand.py): every region spreads outwards and stops halfway
    to its neighbours, as skimage.segmentation.expand_labels does.  For a channel that stains a part of the cell, the nucleus
    say, while the other channel is measured over the whole cell.  n_labels, thresholds and return_distance are what they are
    without it; score_batch scores the grown labels.  With numpy input the labels make one more round trip through the host."""

    def __init__(self, device_id: int = 0, threshold="otsu", connectivity: int = 1, fill_holes: bool = True,
                 extractor: Optional[CellExtractor] = None, split_touching: bool = False, split_h: int = 3,
                 background_radius: Optional[int] = None, denoise: bool = False, local_radius: Optional[int] = None,
                 local_delta: int = 0, local_floor: int = -1, open_radius: Optional[int] = None, open_connectivity: int = 2,
                 min_area: Optional[int] = None, smooth_sigma: Optional[float] = None, split_by: str = "distance",
                 split_depth: int = SPLIT_DEPTH, split_contrast: int = SPLIT_CONTRAST, weak_threshold=None,
                 weak_delta: Optional[int] = None, noise_k: float = NOISE_K, noise_tile: int = NOISE_TILE,
                 noise_floor: float = NOISE_FLOOR, weak_k: Optional[float] = None, expand_distance=None):
        self._expand = None if expand_distance is None else expand_params(expand_distance)
        self.expand_distance = expand_distance
        self._params, self._local, self._background = _threshold_mode(threshold, connectivity, fill_holes, local_radius, local_delta,
                                                                      local_floor, background_radius, denoise, smooth_sigma)
        self._noise = _noise_mode(threshold, connectivity, noise_k, noise_tile, noise_floor, weak_k, weak_threshold, weak_delta)
        self.noise_k, self.noise_tile, self.noise_floor = float(noise_k), int(noise_tile), float(noise_floor)
        self.weak_k = None if weak_k is None else float(weak_k)
        self._hysteresis = None if self._noise is not None else hysteresis_params(threshold, weak_threshold, weak_delta, local_delta)
        # what takes the hysteresis stage's 0 / 1 plane: the fixed threshold 0, and the hole filling as requested
        self._after_hysteresis = segment_params(0, connectivity, fill_holes)
        self.weak_threshold, self.weak_delta = weak_threshold, (None if weak_delta is None else int(weak_delta))
        self._smooth = smooth_params(smooth_sigma, denoise)
        self.smooth_sigma = None if smooth_sigma is None else float(smooth_sigma)
        self._split = split_params(split_touching, split_h)
        self._split_intensity = split_intensity_params(split_touching, split_by, split_h, split_depth, split_contrast)
        self.split_by, self.split_depth, self.split_contrast = split_by, int(split_depth), int(split_contrast)
        self._clean = clean_params(open_radius, open_connectivity, min_area)
        # what labels the cleaned 0 / 1 plane: the fixed threshold 0 and no second hole filling
        self._after_clean = segment_params(0, connectivity, False)
        self.open_radius, self.open_connectivity, self.min_area = (None if open_radius is None else int(open_radius)), \
            int(open_connectivity), (None if min_area is None else int(min_area))
        self.local_radius, self.local_delta, self.local_floor = (None if local_radius is None else int(local_radius)), int(local_delta), \
            int(local_floor)
        self.background_radius, self.denoise = (None if background_radius is None else int(background_radius)), bool(denoise)
        self.split_touching, self.split_h = bool(split_touching), int(split_h)
        if extractor is not None and extractor.device_id != device_id:
            raise ValueError(f"extractor is on device {extractor.device_id}, the segmenter on {device_id}")
        self.threshold, self.connectivity, self.fill_holes = threshold, int(connectivity), bool(fill_holes)
        self._lib = L.load_library()
        self.device_id = device_id
        self._ext = extractor
        self._pre: Optional[Preprocessor] = None        # own handle: created by the first call, after its argument checks
        self._matcher = LabelMatcher(device_id, extractor=self)     # score_batch: cs_label_match on this segmenter's handle
        self._scored = False                            # the last call was a score_batch: last_timing reports the match
        self._expander = LabelExpander(device_id, extractor=self)   # expand_distance: cs_label_expand on this segmenter's handle

    @property
    def _handle(self):
        if self._ext is not None:
            return self._ext._handle
        if self._pre is None:
            self._pre = Preprocessor(self.device_id)
        return self._pre._h

    def close(self):
        """Frees the segmenter's own handle (a shared extractor's handle stays the extractor's); a later call makes a new one."""
        if self._pre is not None:
            self._pre.close()
            self._pre = None

    # ---- argument checks: everything is refused before the device is touched ---------------------------------------
    def _check(self, images, channel):
        on_dev = _is_tensor(images)
        if not on_dev and not isinstance(images, np.ndarray):
            raise TypeError(f"unsupported input type {type(images)}")
        if images.ndim not in (3, 4):
            raise ValueError(f"images must be [B,H,W] or [B,H,W,C], got shape {tuple(images.shape)}")
        B, H, W = (int(x) for x in images.shape[:3])
        Cn = int(images.shape[3]) if images.ndim == 4 else 1
        check_stack_shape(B, H, W, images.shape, Cn)
        if channel is None:
            if Cn == 1:
                channel = 0
            elif Cn >= 3:
                channel = 2                                         # the segmentation channel, improved_detection.py:55
            else:
                raise ValueError(f"{Cn} channels: pass channel= explicitly")
        if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or not 0 <= channel < Cn:
            raise ValueError(f"channel {channel!r} outside [0, {Cn})")
        if on_dev:
            import torch
            if images.dtype == torch.uint8:
                ptype = PIX_U8
            elif images.dtype in (torch.uint16, torch.int16):
                ptype = PIX_U16
            else:
                raise TypeError(f"image tensor dtype {images.dtype}: uint8 or uint16 expected")
            if not images.is_cuda:
                raise ValueError("images is a CPU tensor; pass numpy arrays or CUDA tensors")
            if images.device.index != self.device_id:
                raise ValueError(f"images is on {images.device}, the segmenter on cuda:{self.device_id}")
            if not images.is_contiguous():
                raise ValueError("images is not contiguous")
        else:
            if images.dtype == np.uint8:
                ptype = PIX_U8
            elif images.dtype == np.uint16:
                ptype = PIX_U16
            else:
                raise TypeError(f"image dtype {images.dtype}: uint8 or uint16 expected")
            if not images.flags.c_contiguous:
                raise ValueError("images must be C-contiguous")
        return B, H, W, Cn, int(channel), ptype, on_dev

    def _plane(self, src, dtype, fn, *params, after=()):
        """The source with the plane that `fn`, a cs_segment_* entry point that makes one, makes of it in the channel's place:
        [B,H,W] of `dtype` (None: the images' own), allocated where the images are; a device plane is complete in the handle's
        stream order only.  params: what the entry point takes between the image and the plane, after: what follows the plane."""
        images, B, H, W, Cn, channel, ptype, on_dev = src
        if on_dev:
            import torch
            plane = torch.empty((B, H, W), dtype=images.dtype if dtype is None else torch.uint8, device=images.device)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, images, plane)
        else:
            plane = np.empty((B, H, W), images.dtype if dtype is None else dtype)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        L.check(fn(self._handle, L._ptr(images), ptype, Cn, channel, B, H, W, kind, *params, L._ptr(plane), kind, *after))
        return plane, B, H, W, 1, 0, (ptype if dtype is None else PIX_U8), on_dev

    def _front(self, src, upto, report=False):
        """The front of the pipeline on a checked source (images, B, H, W, Cn, channel, ptype, on_dev), up to and including the
        stage `upto`: "smooth", "background", "local" (the local rule, whatever else is set), "threshold" (the stage in the plain
        cut's place: the noise rule, else hysteresis, else the local rule) or "clean"; a stage that is off is passed over, and each stage takes the
        plane of the one before in the channel's place.  Returns (src, params, reported, guide): the current plane as a source,
        the cs_segment_params that cut it, with report the int32 [B] thresholds of the strong rule where a stage here had to
        read them (else None), and the source the thresholding stage saw."""
        last = ("smooth", "background", "local", "threshold", "clean").index(upto)
        lib, B = self._lib, src[1]
        if self._smooth is not None:
            src = self._plane(src, None, lib.cs_segment_smooth, C.byref(self._smooth))
        if last >= 1 and self._background is not None:
            # the library's final synchronisation comes after everything that reads the plane
            src = self._plane(src, None, lib.cs_segment_background, C.byref(self._background))
        # what split_by="intensity" takes its heights from: the plane the threshold stage sees, never a 0 / 1 plane
        guide = src
        params, reported = self._params, None
        otsu = self._params.threshold_mode == L.THRESH_OTSU

        def strong():
            """Where a stage writes the strong thresholds: Otsu's are computed there, which costs a device plane its one wait; a
            fixed one and local mode's -1 need no reading."""
            reported = np.zeros(B, np.int32)
            if otsu:
                return reported, reported.ctypes.data
            reported[:] = self._params.threshold
            return reported, None

        if last >= 2 and self._noise is not None:
            # the 0 / 1 plane in the channel's place, cut at the fixed threshold 0
            src = self._plane(src, np.uint8, lib.cs_segment_noise, C.byref(self._noise), after=(None,))
        elif last >= 2 and self._hysteresis is not None and upto != "local":
            # the 0 / 1 plane in the channel's place, cut at the fixed threshold 0
            reported, thr = strong() if report else (None, None)
            src = self._plane(src, np.uint8, lib.cs_segment_hysteresis, C.byref(self._params),
                              None if self._local is None else C.byref(self._local), C.byref(self._hysteresis), after=(thr,))
            params = self._after_hysteresis
        elif last >= 2 and self._local is not None:
            # the 0 / 1 plane in the channel's place, cut at the fixed threshold 0: hole filling, labels and the split as they are
            src = self._plane(src, np.uint8, lib.cs_segment_local, C.byref(self._local))
        if last >= 4 and self._clean is not None:
            # the cleaned 0 / 1 plane in the channel's place, cut at the fixed threshold 0 and not filled again; the thresholds
            # are the cleanup's unless the hysteresis stage has reported them already
            thr = None
            if report and reported is None:
                reported, thr = strong()
            src = self._plane(src, np.uint8, lib.cs_segment_clean, C.byref(params), C.byref(self._clean), after=(thr,))
            params = self._after_clean
        return src, params, reported, guide

    def _times(self, fn, n):
        """The n device milliseconds that a cs_segment_*_last_timing reports; for a plane left on the device it waits for it."""
        v = [C.c_double() for _ in range(n)]
        L.check(fn(self._handle, *(C.byref(x) for x in v)))
        return tuple(x.value for x in v)

    def _smooth_timing(self):
        a, b = self._times(self._lib.cs_segment_smooth_last_timing, 2)
        t = {"smooth_ms": b}
        if self._smooth.median:
            t["smooth_median_ms"] = a
        return t

    def smooth_batch(self, images, channel: Optional[int] = None):
        """The smoothed plane of `channel` that every later stage starts from: [B,H,W] of the images' dtype, numpy for numpy
        input, a CUDA tensor for tensor input (complete when this returns).  Needs smooth_sigma."""
        src = (images, *self._check(images, channel))
        if self._smooth is None:
            raise ValueError("smooth_batch needs smooth_sigma: this segmenter smooths nothing")
        src = self._front(src, "smooth")[0]
        if src[-1]:
            self._smooth_timing()                                   # reads the times, which waits for the plane: torch may use it
        return src[0]

    def _background_timing(self):
        return dict(zip(("median_ms", "background_ms"), self._times(self._lib.cs_segment_background_last_timing, 2)))

    def correct_batch(self, images, channel: Optional[int] = None):
        """The background-corrected plane of `channel` that segment_batch thresholds: [B,H,W] of the images' dtype, numpy for
        numpy input, a CUDA tensor for tensor input (complete when this returns).  Needs background_radius."""
        src = (images, *self._check(images, channel))
        if self._background is None:
            raise ValueError("correct_batch needs background_radius: this segmenter corrects nothing")
        src = self._front(src, "background")[0]
        if src[-1]:
            self._background_timing()                               # reads the times, which waits for the plane: torch may use it
        return src[0]

    def _local_timing(self):
        return dict(zip(("local_median_ms", "local_ms"), self._times(self._lib.cs_segment_local_last_timing, 2)))

    def local_mask_batch(self, images, channel: Optional[int] = None):
        """The mask of the local mean threshold that segment_batch fills and labels: [B,H,W] uint8, 1 = foreground, numpy for
        numpy input, a CUDA tensor for tensor input (complete when this returns).  Needs threshold="local"; with
        background_radius it is the mask of the corrected plane."""
        src = (images, *self._check(images, channel))
        if self._local is None:
            raise ValueError("local_mask_batch needs threshold='local'")
        src = self._front(src, "local")[0]
        if src[-1]:
            self._local_timing()                                    # reads the times, which waits for the plane: torch may use it
        return src[0]

    def _hysteresis_timing(self):
        return dict(zip(("hysteresis_level_ms", "hysteresis_link_ms"), self._times(self._lib.cs_segment_hysteresis_last_timing, 2)))

    def hysteresis_mask_batch(self, images, channel: Optional[int] = None):
        """The mask of the hysteresis threshold, before the hole filling: [B,H,W] uint8, 1 = foreground, numpy for numpy input,
        a CUDA tensor for tensor input (complete when this returns).  Needs weak_threshold or weak_delta; with smooth_sigma and
        background_radius it is the mask of what they make."""
        src = (images, *self._check(images, channel))
        if self._hysteresis is None:
            raise ValueError("hysteresis_mask_batch needs weak_threshold or weak_delta: this segmenter has one rule")
        src = self._front(src, "threshold")[0]
        if src[-1]:
            self._hysteresis_timing()                               # reads the times, which waits for the plane: torch may use it
        return src[0]

    def _noise_timing(self):
        return dict(zip(("noise_mesh_ms", "noise_cut_ms", "noise_link_ms"), self._times(self._lib.cs_segment_noise_last_timing, 3)))

    def noise_mask_batch(self, images, channel: Optional[int] = None):
        """The mask of the noise-adaptive threshold, before the hole filling: [B,H,W] uint8, 1 = foreground, numpy for numpy
        input, a CUDA tensor for tensor input (complete when this returns).  Needs threshold="noise"; with smooth_sigma and
        background_radius it is the mask of what they make."""
        src = (images, *self._check(images, channel))
        if self._noise is None:
            raise ValueError("noise_mask_batch needs threshold='noise'")
        src = self._front(src, "threshold")[0]
        if src[-1]:
            self._noise_timing()                                    # reads the times, which waits for the plane: torch may use it
        return src[0]

    def noise_mesh_batch(self, images, channel: Optional[int] = None):
        """The mesh of the noise-adaptive threshold after its 3 x 3 filter: int32 numpy [B, 2, my, mx], the background B8 then
        the noise S8, both in 1/256 counts, my = max(1, H // noise_tile) tiles down and mx across.  Needs threshold="noise"."""
        src = (images, *self._check(images, channel))
        if self._noise is None:
            raise ValueError("noise_mesh_batch needs threshold='noise'")
        src = self._front(src, "background")[0]
        B, H, W = src[1:4]
        mesh = np.zeros((B, 2, max(1, H // self.noise_tile), max(1, W // self.noise_tile)), np.int32)
        self._plane(src, np.uint8, self._lib.cs_segment_noise, C.byref(self._noise), after=(mesh.ctypes.data,))
        return mesh

    def _clean_timing(self):
        return dict(zip(("open_ms", "min_area_ms"), self._times(self._lib.cs_segment_clean_last_timing, 3)[1:]))

    def clean_mask_batch(self, images, channel: Optional[int] = None):
        """The cleaned mask that segment_batch labels: [B,H,W] uint8, 1 = foreground, numpy for numpy input, a CUDA tensor for
        tensor input (complete when this returns).  Needs open_radius or min_area; with background_radius and threshold="local"
        it is the cleaned mask of what they make."""
        src = (images, *self._check(images, channel))
        if self._clean is None:
            raise ValueError("clean_mask_batch needs open_radius or min_area: this segmenter cleans nothing")
        src = self._front(src, "clean")[0]
        if src[-1]:
            self._clean_timing()                                    # reads the times, which waits for the plane: torch may use it
        return src[0]

    def segment_batch(self, images, channel: Optional[int] = None, return_distance: bool = False):
        """images: [B,H,W] or [B,H,W,C] uint8 / uint16, numpy or CUDA tensors of the segmenter's device; the channel that is
        segmented is `channel` (default 2 of >= 3 channels as improved_detection.py:55, 0 of one).
        Returns (labels, n_labels, thresholds): labels int32 [B,H,W] (0 = background, ids 1.. in raster order of each
        component's first pixel), numpy for numpy input and a CUDA tensor for tensor input; n_labels and thresholds int32
        numpy [B].  return_distance (split_touching only): a fourth result, uint8 [B,H,W] where the labels are: the distance
        to the background in half pixels, capped at 255; with split_by="intensity" the heights Hq the split used instead."""
        src = (images, *self._check(images, channel))
        if return_distance and self._split is None:
            raise ValueError("return_distance needs split_touching=True: the plain segmenter computes no distances")
        self._scored = False
        # every stage takes the plane of the one before in the channel's place; threshold, label and split what they leave
        (images, B, H, W, Cn, channel, ptype, on_dev), params, reported, guide = self._front(src, "clean", report=True)
        n_labels = np.zeros(B, np.int32)
        thresholds = np.zeros(B, np.int32)
        if on_dev:
            import torch
            labels = torch.empty((B, H, W), dtype=torch.int32, device=images.device)
            L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, images, labels)
        else:
            labels = np.empty((B, H, W), np.int32)
        kind = L.CS_MEM_DEVICE if on_dev else L.CS_MEM_HOST
        if self._split is None:
            L.check(self._lib.cs_segment_threshold(self._handle, L._ptr(images), ptype, Cn, channel, B, H, W, kind,
                                                   C.byref(params), L._ptr(labels), kind, n_labels.ctypes.data,
                                                   thresholds.ctypes.data))
            if reported is not None:
                thresholds = reported
            if self._local is not None or self._noise is not None:
                thresholds[:] = -1                                  # no single number
            self._grow(labels)
            return labels, n_labels, thresholds
        dist = None
        if return_distance:
            if on_dev:
                dist = torch.empty((B, H, W), dtype=torch.uint8, device=images.device)
                L.order_after_torch(self._lib.cs_preproc_wait_stream, self._handle, dist)
            else:
                dist = np.empty((B, H, W), np.uint8)
        if self._split_intensity is not None:
            L.check(self._lib.cs_segment_split_intensity(self._handle, L._ptr(images), ptype, Cn, channel, B, H, W, kind,
                                                         C.byref(params), C.byref(self._split_intensity), L._ptr(guide[0]), guide[6],
                                                         guide[4], guide[5], L._ptr(labels), kind, n_labels.ctypes.data,
                                                         thresholds.ctypes.data, L._ptr(dist)))
        else:
            L.check(self._lib.cs_segment_split(self._handle, L._ptr(images), ptype, Cn, channel, B, H, W, kind, C.byref(params),
                                               C.byref(self._split), L._ptr(labels), kind, n_labels.ctypes.data,
                                               thresholds.ctypes.data, L._ptr(dist)))
        if reported is not None:
            thresholds = reported
        if self._local is not None or self._noise is not None:
            thresholds[:] = -1
        self._grow(labels)
        return (labels, n_labels, thresholds, dist) if return_distance else (labels, n_labels, thresholds)

    def _grow(self, labels):
        """expand_distance: the labels of segment_batch grown where they are."""
        if self._expand is not None:
            self._expander.expand_batch(labels, self.expand_distance, out=labels)

    def score_batch(self, images, truth, channel: Optional[int] = None, thresholds=SCORE_THRESHOLDS, max_truth: Optional[int] = None):
        """segment_batch, then the labels scored where they are against `truth` (int32 [B,H,W], numpy or a CUDA tensor, 0 =
        background) on the same handle: cellscreen/score.py.  Returns (stats, labels, n_labels): LabelMatch.stats(thresholds) of
        the batch, and segment_batch's labels and counts.  max_truth: the largest label `truth` may hold (None: its maximum).
        The thresholds, `truth` and the images are checked before the device is touched."""
        check_thresholds(thresholds)
        B, H, W = self._check(images, channel)[:3]
        check_label_plane("truth", truth, self.device_id, self._matcher._noun)
        if tuple(truth.shape) != (B, H, W):
            raise ValueError(f"truth {tuple(truth.shape)} and images {tuple(images.shape)} differ in batch or height x width")
        labels, n_labels, _ = self.segment_batch(images, channel)
        m = self._matcher.match_batch(labels, truth, max_pred=max(1, int(n_labels.max())), max_truth=max_truth)
        self._scored = True
        return m.stats(thresholds), labels, n_labels

    def last_timing(self):
        """Device milliseconds of the last call's stages; with split_touching the stages of cs_segment_split (with
        split_by="intensity" those of cs_segment_split_intensity: height_ms where the other has distance_ms); with
        background_radius also median_ms and background_ms (the top-hat) of the last correction; with threshold="local" also
        local_median_ms and local_ms (the sums and the comparison) of the last mask; with open_radius or min_area also open_ms
        and min_area_ms of the last cleanup (0 for a step that is off), and threshold_ms is then the labelling call's cut of the
        cleaned plane; with smooth_sigma also smooth_ms (the two passes) of the last smoothing, and smooth_median_ms when the
        median ran there; with weak_threshold or weak_delta also hysteresis_level_ms (thresholds or sums, and the level plane)
        and hysteresis_link_ms (weak components, flags, the kept plane) of the last hysteresis stage, which then stands in the
        local rule's place: local_ms is not reported; with threshold="noise" noise_mesh_ms (tile statistics and the mesh filter),
        noise_cut_ms (the cut or the level plane) and noise_link_ms (with weak_k: weak components, flags, the kept plane; else 0)
        of the last noise stage; after score_batch also match_count_ms (clearing and cs_label_match's one pass over the two label
        planes) and match_reduce_ms (its reduction into the tables); with expand_distance also expand_columns_ms and expand_rows_ms,
        the two passes of the last cs_label_expand."""
        extra = self._smooth_timing() if self._smooth is not None else {}
        if self._background is not None:
            extra.update(self._background_timing())
        if self._noise is not None:
            extra.update(self._noise_timing())
        elif self._hysteresis is not None:
            extra.update(self._hysteresis_timing())
        elif self._local is not None:
            extra.update(self._local_timing())
        if self._clean is not None:
            extra.update(self._clean_timing())
        if self._scored:
            extra.update(self._matcher.last_timing())
        if self._expand is not None:
            extra.update(self._expander.last_timing())
        if self._split is None:
            return dict(zip(("threshold_ms", "label_ms"), self._times(self._lib.cs_segment_last_timing, 2)), **extra)
        if self._split_intensity is not None:
            return dict(zip(("threshold_ms", "height_ms", "seed_ms", "flood_ms"),
                            self._times(self._lib.cs_segment_split_intensity_last_timing, 4)), **extra)
        return dict(zip(("threshold_ms", "distance_ms", "seed_ms", "flood_ms"), self._times(self._lib.cs_segment_split_last_timing, 4)),
                    **extra)


    def last_host_syncs(self) -> int:
        """Host synchronisations of the last split_touching call (either split_by): the reads of the control word between
        groups of reconstruction and flood rounds, and the final one."""
        if self._split is None:
            raise ValueError("last_host_syncs needs split_touching=True: the plain segmenter synchronises once")
        a, b = C.c_int32(), C.c_int32()
        L.check(self._lib.cs_segment_split_last_syncs(self._handle, C.byref(a), C.byref(b)))
        return a.value + b.value + 1


def threshold_cell_extractor(device_id: int = 0, out_hw=(OUT_SIDE, OUT_SIDE), threshold="otsu", connectivity: int = 1,
                             fill_holes: bool = True, split_touching: bool = False, split_h: int = 3,
                             background_radius: Optional[int] = None, denoise: bool = False, local_radius: Optional[int] = None,
                             local_delta: int = 0, local_floor: int = -1, open_radius: Optional[int] = None,
                             open_connectivity: int = 2, mask_min_area: Optional[int] = None,
                             smooth_sigma: Optional[float] = None, split_by: str = "distance", split_depth: int = SPLIT_DEPTH,
                             split_contrast: int = SPLIT_CONTRAST, weak_threshold=None, weak_delta: Optional[int] = None,
                             noise_k: float = NOISE_K, noise_tile: int = NOISE_TILE, noise_floor: float = NOISE_FLOOR,
                             weak_k: Optional[float] = None, expand_distance=None, **qc):
    """The `cell_extractor(image_path) -> (cells, stats)` that ProductionMutantScreening and create_training_dataset accept,
    with the built-in segmenter in StarDist's place: the file is read (extract.read_image / split_channels), uploaded once,
    segmented and extracted on one handle, and the labels never leave the device.  Not StarDist: see the module text.
    Errors raise as label_cell_extractor's do; the screening driver's try turns them into the reference's "Error processing"
    line and ([], []).  out_hw and **qc as for label_cell_extractor; split_touching, split_h, background_radius and denoise as
    for ThresholdSegmenter, and threshold="local" with local_radius, local_delta and local_floor too: with background_radius the segmentation channel is corrected before the threshold, while the
    extraction still reads the raw analysis channel, so the intensity rules and the crops are what they are without it.
    open_radius and open_connectivity as for ThresholdSegmenter, and mask_min_area for its min_area: the mask cleanup before
    the labels.  The name differs here because min_area is, and stays, the extraction's own area rule among **qc.
    smooth_sigma as for ThresholdSegmenter: the segmentation channel is smoothed first, the extraction reads the raw one.
    split_by, split_depth and split_contrast as for ThresholdSegmenter; split_by="intensity" wants smooth_sigma.
    weak_threshold and weak_delta as for ThresholdSegmenter: the hysteresis threshold in the plain cut's place.
    threshold="noise" with noise_k, noise_tile, noise_floor and weak_k as for ThresholdSegmenter: the noise-adaptive threshold.
    expand_distance as for ThresholdSegmenter: the labels are grown by that many pixels before the extraction, for a
    segmentation channel that stains the nucleus alone.  The QC numbers among **qc stay the caller's: a grown region is judged
    by the same min_area and max_area (and border, eccentricity and intensity rules) unless they are changed to fit it."""
    out_hw = check_out_hw(out_hw)
    if expand_distance is not None:
        expand_params(expand_distance)
    _threshold_mode(threshold, connectivity, fill_holes, local_radius, local_delta, local_floor, background_radius, denoise,
                    smooth_sigma)
    split_params(split_touching, split_h)
    split_intensity_params(split_touching, split_by, split_h, split_depth, split_contrast)
    clean_params(open_radius, open_connectivity, mask_min_area)
    if _noise_mode(threshold, connectivity, noise_k, noise_tile, noise_floor, weak_k, weak_threshold, weak_delta) is None:
        hysteresis_params(threshold, weak_threshold, weak_delta, local_delta)
    qc_params(**qc)
    st = {}

    def cell_extractor(image_path: str):
        import torch
        image = read_image(image_path)
        _, img, ch = split_channels(image)
        seg_ch = 2 if img.ndim == 3 else 0
        if img.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"image dtype {img.dtype}: uint8 or uint16 expected")
        if "x" not in st:
            st["x"] = CellExtractor(device_id, out_hw, **qc)
            st["s"] = ThresholdSegmenter(device_id, threshold, connectivity, fill_holes, extractor=st["x"],
                                         split_touching=split_touching, split_h=split_h, background_radius=background_radius,
                                         denoise=denoise, local_radius=local_radius, local_delta=local_delta,
                                         local_floor=local_floor, open_radius=open_radius, open_connectivity=open_connectivity,
                                         min_area=mask_min_area, smooth_sigma=smooth_sigma, split_by=split_by,
                                         split_depth=split_depth, split_contrast=split_contrast, weak_threshold=weak_threshold,
                                         weak_delta=weak_delta, noise_k=noise_k, noise_tile=noise_tile, noise_floor=noise_floor,
                                         weak_k=weak_k, expand_distance=expand_distance)
        host = np.ascontiguousarray(img)[None]
        dev = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(torch.device("cuda", device_id))
        labels, _, _ = st["s"].segment_batch(dev, channel=seg_ch)
        r = st["x"].extract_batch(dev, labels, channel=ch)
        status = int(r.status[0])
        if status != IMAGE_OK:
            raise ValueError("a passing region has a bounding-box side below 8 px (equalize_adapthist raises)"
                             if status == IMAGE_NO_CELLS else st["x"]._unsupported_text() + " (beyond the preprocess kernel)")
        return list(r.cells.cpu().numpy()), region_stats(r.regions)

    return cell_extractor
