"""CPU restatement of the segmenter's hysteresis threshold (cs_segment_hysteresis in csrc/segment.hip,
ThresholdSegmenter(weak_threshold=..., weak_delta=...)): what the device kernels are compared against, with numpy and
scipy.ndimage.label only.

  weak_of        the low threshold of the global rules from the strong one: min(weak, t) for an int (counts),
                 (t * q) >> 16 with q = int(f * 65536 + 0.5) in 1..65535 for a float strictly between 0 and 1
  levels_global  0 background, 1 where x > low only, 2 where x > t (low <= t: every strong pixel is a weak pixel)
  levels_local   the same under the local rule: margin = n * x - S - n * delta of tests/local_reference.py, 2 where it is
                 positive under delta, 1 where only under weak_delta (<= delta), and x > floor for both; a tie is background
  hysteresis     the pixels of those components of levels > 0 (connectivity 1: 4 neighbours, 2: 8) that hold a pixel of level 2
  segment        hysteresis, then tests/segment_reference.py's hole filling and labels; the threshold reported is the strong one
This is skimage.filters.apply_hysteresis_threshold with integer rules.  tests/golden/golden_hysteresis.npz
(tools/make_golden_hysteresis.py) pins `hysteresis` to SciPy 1.15.3 in the form of that function's body."""
import numpy as np

import background_reference as BR
import local_reference as LR
import segment_reference as R


def weak_of(t: int, weak_threshold) -> int:
    """low_b of one image whose strong threshold is t."""
    if isinstance(weak_threshold, (bool, np.bool_)):
        raise TypeError("weak_threshold: an int (counts) or a float (fraction)")
    if isinstance(weak_threshold, (int, np.integer)):
        if not 0 <= int(weak_threshold) <= 65535:
            raise ValueError("weak_threshold outside 0..65535")
        return min(int(weak_threshold), int(t))
    f = float(weak_threshold)
    if not 0.0 < f < 1.0:
        raise ValueError("a fraction lies strictly between 0 and 1")
    q = int(f * 65536 + 0.5)
    if not 1 <= q <= 65535:
        raise ValueError("the fraction rounds to q outside 1..65535")
    return (int(t) * q) >> 16


def levels_global(channel: np.ndarray, t: int, low: int) -> np.ndarray:
    if low > t:
        raise ValueError("low above the strong threshold")
    x = channel.astype(np.int64)
    return (x > low).astype(np.uint8) + (x > t).astype(np.uint8)


def levels_local(x: np.ndarray, r: int, delta: int, weak_delta: int, floor: int = -1, median: bool = False) -> np.ndarray:
    LR._check(x, r, delta, floor)
    if not -65535 <= weak_delta <= delta:
        raise ValueError("weak_delta outside -65535..delta")
    if median:
        x = BR.median3(x)
    sums = LR.window_sum(x, r)
    above = x.astype(np.int64) > floor
    weak = (LR.margin(x, r, weak_delta, sums) > 0) & above
    strong = (LR.margin(x, r, delta, sums) > 0) & above
    return weak.astype(np.uint8) + strong.astype(np.uint8)


def hysteresis(levels: np.ndarray, connectivity: int = 1) -> np.ndarray:
    """uint8 0 / 1 plane of one 2-D level plane."""
    if levels.ndim != 2:
        raise TypeError("2-D level plane expected")
    lab, n = R.label_mask(levels > 0, connectivity)
    keep = np.zeros(n + 1, bool)
    keep[lab[levels == 2]] = True
    keep[0] = False
    return keep[lab].astype(np.uint8)


def hysteresis_global(channel: np.ndarray, threshold="otsu", weak_threshold=0.5, connectivity: int = 1):
    """(plane, t) of one 2-D integer image under the global rules."""
    t = R.otsu(channel) if isinstance(threshold, str) else int(threshold)
    return hysteresis(levels_global(channel, t, weak_of(t, weak_threshold)), connectivity), t


def _channel(images, channel):
    if images.ndim == 3:
        return images
    return images[..., channel if channel is not None else (2 if images.shape[3] >= 3 else 0)]


def hysteresis_batch(images: np.ndarray, threshold="otsu", weak_threshold=0.5, connectivity: int = 1, channel=None):
    """(planes uint8 [B,H,W], thresholds int32 [B]) of a [B,H,W] / [B,H,W,C] stack under the global rules."""
    out = [hysteresis_global(np.ascontiguousarray(c), threshold, weak_threshold, connectivity) for c in _channel(images, channel)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def hysteresis_local_batch(images: np.ndarray, r: int, delta: int, weak_delta: int, floor: int = -1, median: bool = False,
                           connectivity: int = 1, channel=None) -> np.ndarray:
    return np.stack([hysteresis(levels_local(np.ascontiguousarray(c), r, delta, weak_delta, floor, median), connectivity)
                     for c in _channel(images, channel)])


def segment(channel: np.ndarray, threshold="otsu", weak_threshold=0.5, connectivity: int = 1, fill_holes: bool = True):
    """(labels, n_labels, t) of one 2-D image: the plane, then what the segmenter does with a mask."""
    plane, t = hysteresis_global(channel, threshold, weak_threshold, connectivity)
    lab, n, _ = LR.label_plane(plane, connectivity, fill_holes)
    return lab, n, t


def segment_local(channel: np.ndarray, r: int, delta: int, weak_delta: int, floor: int = -1, median: bool = False,
                  connectivity: int = 1, fill_holes: bool = True):
    return LR.label_plane(hysteresis(levels_local(channel, r, delta, weak_delta, floor, median), connectivity), connectivity,
                          fill_holes)


def segment_batch(images: np.ndarray, channel=None, **kw):
    out = [segment(np.ascontiguousarray(c), **kw) for c in _channel(images, channel)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def level_inputs(shape, seed=0):
    """(name, uint8 level plane) of one shape: noise at two densities with a few strong pixels, blobs joined by bridges with
    every other blob strong at its centre, an all-weak plane with its one strong pixel at each corner in turn and at its root
    (the first pixel in raster order, which is corner 0), the same without a strong pixel, a plane without a weak pixel, and a
    checkerboard of weak pixels with strong ones on a few squares of one colour, where the connectivities differ."""
    H, W = shape
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    named = []
    for name, dens in (("noise35", 0.35), ("noise60", 0.6)):
        lv = (rng.random(shape) < dens).astype(np.uint8)
        lv[(rng.random(shape) < 0.02) & (lv > 0)] = 2
        named.append((name, lv))
    rad = max(2, min(H, W, 64) // 4)
    pitch = 3 * rad
    cy, cx = yy // pitch * pitch + pitch // 2, xx // pitch * pitch + pitch // 2
    blobs = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
    blobs |= (yy % pitch == pitch // 2) & (xx // pitch % 2 == 0)                # every other pair of blobs joined by a bridge
    lv = blobs.astype(np.uint8)
    lv[(yy == cy) & (xx == cx) & ((yy // pitch + xx // pitch) % 3 == 0)] = 2
    named.append(("bridged", lv))
    for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        lv = np.ones(shape, np.uint8)
        lv[y, x] = 2
        named.append((f"corner{k}", lv))
    named.append(("weak_only", np.ones(shape, np.uint8)))
    named.append(("empty", np.zeros(shape, np.uint8)))
    lv = ((yy + xx) % 2 == 0).astype(np.uint8)
    lv[(yy % 5 == 0) & (xx % 7 == 0) & (lv > 0)] = 2
    named.append(("checker", lv))
    return named


def image_of(levels: np.ndarray, dtype, t: int, low: int) -> np.ndarray:
    """An image whose level plane under (t, low) is `levels`; low < t below the type's top.  Level 1 and level 2 sit ON the
    first value that passes (low + 1, t + 1) on even pixels and well above on odd ones, level 0 ON low itself or at 0."""
    if not 0 <= low < t < int(np.iinfo(dtype).max):
        raise ValueError("need 0 <= low < t < top")
    yy, xx = np.mgrid[0:levels.shape[0], 0:levels.shape[1]]
    odd = (yy + xx) % 2 == 1
    top = int(np.iinfo(dtype).max)
    img = np.where(odd, 0, low)
    img = np.where(levels == 1, np.where(odd, t, low + 1), img)
    img = np.where(levels == 2, np.where(odd, top, t + 1), img)
    return img.astype(dtype)
