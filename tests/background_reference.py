"""CPU restatement of the segmenter's background correction (cs_segment_background in csrc/segment.hip,
ThresholdSegmenter(background_radius=...)): what the device kernels are compared against, with numpy only.

  window_min / window_max   the minimum / maximum over the window [i - r, i + r] x [j - r, j + r] clipped to the image
                            (window_*_direct: the same straight from the definition, O(r) per pixel)
  median3                   the 3 x 3 median with the edge pixel repeated: scipy.ndimage.median_filter(x, size=3), default mode
  white_tophat              x - window_max(window_min(x, r), r): scipy.ndimage.white_tophat(x, size=(2r + 1, 2r + 1))
  correct                   the optional median, then the top-hat: the plane the segmenter thresholds
  segment                   correct, then tests/segment_reference.py's segment on the plane
tests/test_background_cpu.py holds both restatements against SciPy bit for bit.  All arithmetic stays in the pixel type."""
import numpy as np

import segment_reference as R


def _window_direct(x: np.ndarray, r: int, axis: int, op, ident) -> np.ndarray:
    """The definition: op over [i - r, i + r] along `axis`, clipped -- padding with op's identity is what clipping means.
    O(r) per pixel."""
    widths = [(0, 0), (0, 0)]
    widths[axis] = (r, r)
    p = np.pad(x, widths, mode="constant", constant_values=ident)
    return op.reduce(np.lib.stride_tricks.sliding_window_view(p, 2 * r + 1, axis=axis), axis=-1)


def _window(x: np.ndarray, r: int, axis: int, op, ident) -> np.ndarray:
    """The same in O(log r) per pixel, so that the device tests stay quick: after step j an element holds op over the 2^j
    elements from itself on, and a window of w = 2r + 1 is two overlapping spans of 2^k <= w."""
    x = np.moveaxis(x, axis, -1)
    n, w, k = x.shape[-1], 2 * r + 1, 0
    while (2 << k) <= w:
        k += 1
    fill = lambda m: np.full(x.shape[:-1] + (m,), ident, x.dtype)
    p = np.concatenate([fill(r), x, fill(r + (1 << k))], axis=-1)
    for j in range(k):
        p = op(p, np.concatenate([p[..., 1 << j:], fill(1 << j)], axis=-1))
    off = w - (1 << k)
    return np.moveaxis(op(p[..., :n], p[..., off:off + n]), -1, axis)


def _check(x, r):
    if x.ndim != 2 or x.dtype not in (np.uint8, np.uint16):
        raise TypeError("2-D uint8 / uint16 image expected")
    if not 1 <= r <= 255:
        raise ValueError("radius outside 1..255")


def window_min(x: np.ndarray, r: int, window=_window) -> np.ndarray:
    _check(x, r)
    top = np.iinfo(x.dtype).max
    return window(window(x, r, 1, np.minimum, top), r, 0, np.minimum, top)


def window_max(x: np.ndarray, r: int, window=_window) -> np.ndarray:
    _check(x, r)
    return window(window(x, r, 1, np.maximum, 0), r, 0, np.maximum, 0)


def window_min_direct(x: np.ndarray, r: int) -> np.ndarray:
    return window_min(x, r, _window_direct)


def window_max_direct(x: np.ndarray, r: int) -> np.ndarray:
    return window_max(x, r, _window_direct)


def median3(x: np.ndarray) -> np.ndarray:
    p = np.pad(x, 1, mode="edge")
    H, W = x.shape
    nine = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return np.sort(nine, axis=0)[4]


def white_tophat(x: np.ndarray, r: int) -> np.ndarray:
    opened = window_max(window_min(x, r), r)
    assert (opened <= x).all()                          # an opening is never above the image: no wrap
    return x - opened


def correct(channel: np.ndarray, radius: int, denoise: bool = False) -> np.ndarray:
    """The corrected plane of one 2-D uint8 / uint16 image."""
    _check(channel, radius)
    return white_tophat(median3(channel) if denoise else channel, radius)


def correct_batch(images: np.ndarray, radius: int, denoise: bool = False, channel=None) -> np.ndarray:
    if images.ndim == 3:
        chan = images
    else:
        ch = channel if channel is not None else (2 if images.shape[3] >= 3 else 0)
        chan = images[..., ch]
    return np.stack([correct(np.ascontiguousarray(c), radius, denoise) for c in chan])


def segment(channel: np.ndarray, radius: int, denoise: bool = False, threshold="otsu", connectivity: int = 1, fill_holes: bool = True):
    """(labels, n_labels, threshold) of the corrected plane: ThresholdSegmenter(background_radius=radius, denoise=denoise)."""
    return R.segment(correct(channel, radius, denoise), threshold, connectivity, fill_holes)


def segment_batch(images: np.ndarray, radius: int, denoise: bool = False, channel=None, **kw):
    planes = correct_batch(images, radius, denoise, channel)
    out = [R.segment(p, **kw) for p in planes]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32))
