"""CPU restatement of the segmenter's split_by="intensity" option (cs_segment_split_intensity of csrc/segment.hip):
the watershed of tests/split_reference.py on a height plane made from the image instead of from the mask, with numpy and
scipy.ndimage only.  A function of the mask and the guide plane alone, all integers.

  heights       Hq: per component c of the mask (under the connectivity), lo_c / hi_c the smallest and largest guide value
                over its pixels, span_c = max(hi_c - lo_c, min_contrast, 1), Hq = 1 + ((G - lo_c) * 254) // span_c on the mask
                (a byte in 1..255), 0 on background.  scipy.ndimage.label / minimum / maximum; the golden pins it to SciPy.
  split_intensity   reconstruct / seeds / flood / renumber of split_reference with Hq in Dq's place and depth in h's.
  segment_batch the restatement of ThresholdSegmenter(split_touching=True, split_by="intensity", ...).segment_batch(...,
                return_distance=True) with the stage options the tests use: the guide is the plane the threshold stage saw (after
                the smoothing and the correction), never the 0 / 1 plane of local mode or of the cleanup.
  scene         the 170 x 260 field of 11 Gaussian cells the option was specified on."""
import numpy as np
from scipy import ndimage

import background_reference as BR
import clean_reference as CR
import local_reference as LR
import smooth_reference as MR
from segment_reference import STRUCTURES, otsu
from split_reference import flood, reconstruct, renumber, seeds

CELLS = [(40, 40, 16, 3000), (40, 62, 16, 3000), (110, 45, 18, 1500), (110, 70, 18, 3500), (45, 150, 14, 2500), (40, 210, 10, 2500),
         (40, 224, 12, 2800), (110, 150, 15, 2500), (128, 165, 15, 2500), (106, 176, 15, 2500), (126, 190, 14, 2200)]
SCENE_SHAPE, SCENE_BACKGROUND = (170, 260), 300


def heights(mask: np.ndarray, guide: np.ndarray, connectivity: int = 1, min_contrast: int = 0) -> np.ndarray:
    """Hq uint8 of one boolean mask and one 2-D uint8 / uint16 guide plane."""
    mask = np.asarray(mask, bool)
    if guide.shape != mask.shape or guide.dtype not in (np.uint8, np.uint16):
        raise TypeError("a uint8 / uint16 guide of the mask's shape expected")
    if not 0 <= int(min_contrast) <= 65535:
        raise ValueError("min_contrast outside 0..65535")
    lab, n = ndimage.label(mask, structure=STRUCTURES[connectivity])
    out = np.zeros(mask.shape, np.uint8)
    if n == 0:
        return out
    idx = np.arange(1, n + 1)
    g = guide.astype(np.int64)
    lo = np.asarray(ndimage.minimum(g, lab, idx), np.int64)
    hi = np.asarray(ndimage.maximum(g, lab, idx), np.int64)
    span = np.maximum(np.maximum(hi - lo, int(min_contrast)), 1)
    c = lab[mask] - 1
    out[mask] = 1 + ((g[mask] - lo[c]) * 254) // span[c]
    return out


def split_intensity(mask: np.ndarray, guide: np.ndarray, connectivity: int = 1, depth: int = 16, min_contrast: int = 0):
    """(labels int32, n_labels, Hq uint8) of one boolean mask and its guide plane."""
    if not 1 <= int(depth) <= 254:
        raise ValueError("depth outside 1..254")
    mask = np.asarray(mask, bool)
    Hq = heights(mask, guide, connectivity, min_contrast)
    s, _ = seeds(reconstruct(Hq, int(depth), connectivity), mask, connectivity)
    lab, n = renumber(flood(s, Hq, mask, connectivity))
    return lab.astype(np.int32), n, Hq


def split_intensity_batch(masks: np.ndarray, guides: np.ndarray, connectivity: int = 1, depth: int = 16, min_contrast: int = 0):
    """(labels [B,H,W], n_labels [B], Hq [B,H,W]) of a stack of masks and guides, image by image."""
    out = [split_intensity(m, g, connectivity, depth, min_contrast) for m, g in zip(masks, guides)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.stack([o[2] for o in out])


def segment_batch(images: np.ndarray, channel=None, threshold="otsu", connectivity: int = 1, fill_holes: bool = True, depth: int = 16,
                  min_contrast: int = 0, smooth_sigma=None, denoise: bool = False, background_radius=None, local_radius=None,
                  local_delta: int = 0, local_floor: int = -1, open_radius=None, open_connectivity: int = 2, min_area=None,
                  raw_guide: bool = False):
    """(labels, n_labels, thresholds, Hq, guides) of a [B,H,W] / [B,H,W,C] stack.  The median runs once, inside the first stage
    that exists (the smoothing, else the correction, else the local rule), as in cellscreen.segment.  raw_guide: the raw
    channel as the guide, which the segmenter never does: for tests that show the guide matters."""
    if images.ndim == 3:
        chan = images
    else:
        chan = images[..., channel if channel is not None else (2 if images.shape[3] >= 3 else 0)]
    labs, ns, thrs, hqs, guides = [], [], [], [], []
    for raw in chan:
        x = np.ascontiguousarray(raw)
        med = bool(denoise)
        if smooth_sigma is not None:
            x, med = MR.smooth_sigma(x, float(smooth_sigma), med), False
        if background_radius is not None:
            x, med = BR.correct(x, int(background_radius), med), False
        if isinstance(threshold, str) and threshold == "local":
            m, t = LR.local_mask(x, int(local_radius), local_delta, local_floor, med) > 0, -1
        else:
            t = otsu(x) if threshold == "otsu" else int(threshold)
            m = x > t
        if fill_holes:
            m = ndimage.binary_fill_holes(m)
        if open_radius is not None or min_area is not None:
            m = CR.clean(m.astype(np.uint8), open_radius, open_connectivity, min_area, connectivity) > 0
        g = np.ascontiguousarray(raw) if raw_guide else x
        lab, n, Hq = split_intensity(m, g, connectivity, depth, min_contrast)
        labs.append(lab), ns.append(n), thrs.append(t), hqs.append(Hq), guides.append(g)
    return np.stack(labs), np.array(ns, np.int32), np.array(thrs, np.int32), np.stack(hqs), np.stack(guides)


def scene(noise: float = 60.0, seed: int = 0, dtype=np.uint16) -> np.ndarray:
    """[170, 260] of `dtype`: 11 Gaussian cells a * exp(-d^2 / (2 (0.5 r)^2)), summed, on a background of 300 counts, plus
    Gaussian noise of `noise` counts.  They overlap in pairs, a bright + dim pair and a group of four, without a neck between
    them: the mask has 5 components.  uint8: the uint16 scene divided by 16."""
    yy, xx = np.mgrid[0:SCENE_SHAPE[0], 0:SCENE_SHAPE[1]]
    f = np.full(SCENE_SHAPE, float(SCENE_BACKGROUND))
    for cy, cx, r, a in CELLS:
        f += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.5 * r) ** 2))
    if noise:
        f += np.random.default_rng(seed).normal(0.0, noise, SCENE_SHAPE)
    u16 = np.rint(np.clip(f, 0, 65535)).astype(np.uint16)
    return u16 if np.dtype(dtype) == np.uint16 else (u16 // 16).clip(0, 255).astype(np.uint8)
