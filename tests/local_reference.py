"""CPU restatement of the segmenter's local mean threshold (cs_segment_local in csrc/segment.hip,
ThresholdSegmenter(threshold="local", ...)): what the device kernels are compared against, with numpy only.

  window_sum         S(i, j): the int64 sum of x over [i - r, i + r] x [j - r, j + r], indices outside the image reflected about
                     the edge (d c b a | a b c d: numpy.pad's 'symmetric', scipy's mode='reflect'; period 2 * side, so r may
                     exceed a side), from a summed-area table
  window_sum_direct  the same straight from the definition: every window summed on its own, folded indices, O(w^2) per pixel
  local_mask         n * x - S - n * delta > 0 and x > floor, n = (2r + 1)^2; with median the plane of
                     background_reference.median3 stands on both sides of the comparison
  segment            the mask, then tests/segment_reference.py's hole filling and labels (threshold reported as -1)
This is x > skimage.filters.threshold_local(x, 2r + 1, method='mean', offset=-delta) decided in integers.  The one deliberate
difference: an exact tie, n * (x - delta) = S, is background here, while the library's float64 mean may fall on either side.
tests/golden/golden_local.npz (tools/make_golden_local.py) pins the rest to scikit-image 0.18.3 on inputs that cannot tie."""
import numpy as np
from scipy import ndimage

import background_reference as BR
import segment_reference as R


def _check(x, r, delta, floor):
    if x.ndim != 2 or x.dtype not in (np.uint8, np.uint16):
        raise TypeError("2-D uint8 / uint16 image expected")
    if not 1 <= r <= 255:
        raise ValueError("radius outside 1..255")
    if not -65535 <= delta <= 65535:
        raise ValueError("delta outside -65535..65535")
    if not -1 <= floor <= 65535:
        raise ValueError("floor outside -1..65535")


def fold(i, n):
    """Index i of a line of n reflected about its edges (any integer i, arrays too)."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def window_sum(x: np.ndarray, r: int) -> np.ndarray:
    w = 2 * r + 1
    p = np.pad(x.astype(np.int64), r, mode="symmetric")
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), axis=0), axis=1)
    return c[w:, w:] - c[:-w, w:] - c[w:, :-w] + c[:-w, :-w]


def window_sum_direct(x: np.ndarray, r: int) -> np.ndarray:
    H, W = x.shape
    x64 = x.astype(np.int64)
    out = np.zeros((H, W), np.int64)
    for i in range(H):
        rows = fold(np.arange(i - r, i + r + 1), H)
        for j in range(W):
            cols = fold(np.arange(j - r, j + r + 1), W)
            out[i, j] = x64[np.ix_(rows, cols)].sum()
    return out


def margin(x: np.ndarray, r: int, delta: int, sums=None) -> np.ndarray:
    """n * x - S - n * delta, int64: foreground needs it positive; zero is the tie."""
    n = (2 * r + 1) ** 2
    return n * x.astype(np.int64) - (window_sum(x, r) if sums is None else sums) - n * int(delta)


def local_mask(x: np.ndarray, r: int, delta: int = 0, floor: int = -1, median: bool = False, sums=None) -> np.ndarray:
    """The uint8 plane (1 = foreground) of one 2-D image.  sums: window_sum of the (median's) plane, if the caller has it."""
    _check(x, r, delta, floor)
    if median:
        x = BR.median3(x)
    return ((margin(x, r, delta, sums) > 0) & (x.astype(np.int64) > floor)).astype(np.uint8)


def local_mask_batch(images: np.ndarray, r: int, delta: int = 0, floor: int = -1, median: bool = False, channel=None) -> np.ndarray:
    if images.ndim == 3:
        chan = images
    else:
        ch = channel if channel is not None else (2 if images.shape[3] >= 3 else 0)
        chan = images[..., ch]
    return np.stack([local_mask(np.ascontiguousarray(c), r, delta, floor, median) for c in chan])


def label_plane(mask: np.ndarray, connectivity: int = 1, fill_holes: bool = True):
    """(labels, n_labels, -1) of a 0 / 1 plane: what the segmenter does with the mask."""
    m = mask > 0
    lab, n = R.label_mask(ndimage.binary_fill_holes(m) if fill_holes else m, connectivity)
    return lab, n, -1


def segment(channel: np.ndarray, r: int, delta: int = 0, floor: int = -1, median: bool = False, connectivity: int = 1,
            fill_holes: bool = True):
    return label_plane(local_mask(channel, r, delta, floor, median), connectivity, fill_holes)
