"""CPU restatement of the built-in segmenter (csrc/segment.hip, cellscreen.segment): what the device kernels are compared
against, with numpy and scipy.ndimage only.

  otsu          scikit-image 0.18.3's threshold_otsu on an integer image (filters/thresholding.py:282-350 with
                exposure.histogram's integer branch: one bin per integer of [min, max]); tests/golden/golden_segment.npz pins
                it to the library.  A constant image returns its value, as 0.18.3 does.
  fill_holes    scipy.ndimage.binary_fill_holes, default structure.
  label         scipy.ndimage.label with the 4- or 8-neighbour structure: ids 1.. in raster order of each component's first
                pixel, which is skimage.measure.label's numbering too (the golden records the latter).
Foreground is pixel > threshold."""
import numpy as np
from scipy import ndimage

STRUCTURES = {1: ndimage.generate_binary_structure(2, 1), 2: ndimage.generate_binary_structure(2, 2)}


def otsu(channel: np.ndarray) -> int:
    if not np.issubdtype(channel.dtype, np.integer):
        raise TypeError("integer image expected")
    lo, hi = int(channel.min()), int(channel.max())
    if lo == hi:
        return lo
    counts = np.bincount(channel.ravel().astype(np.int64) - lo, minlength=hi - lo + 1).astype(np.float64)
    centers = np.arange(lo, hi + 1).astype(np.float64)
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    m1 = np.cumsum(counts * centers) / w1
    m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
    var = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return lo + int(np.argmax(var))


def mask_of(channel: np.ndarray, threshold: int, fill_holes: bool) -> np.ndarray:
    m = channel > threshold
    return ndimage.binary_fill_holes(m) if fill_holes else m


def label_mask(mask: np.ndarray, connectivity: int = 1):
    lab, n = ndimage.label(mask, structure=STRUCTURES[connectivity])
    return lab.astype(np.int32), int(n)


def segment(channel: np.ndarray, threshold="otsu", connectivity: int = 1, fill_holes: bool = True):
    """(labels int32 [H,W], n_labels, threshold) of one 2-D integer image."""
    t = otsu(channel) if threshold == "otsu" else int(threshold)
    lab, n = label_mask(mask_of(channel, t, fill_holes), connectivity)
    return lab, n, t


def segment_batch(images: np.ndarray, channel=None, **kw):
    """The restatement of ThresholdSegmenter.segment_batch for [B,H,W] / [B,H,W,C] stacks."""
    if images.ndim == 3:
        chan = images
    else:
        ch = channel if channel is not None else (2 if images.shape[3] >= 3 else 0)
        chan = images[..., ch]
    out = [segment(c, **kw) for c in chan]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32))


def first_pixels(labels: np.ndarray) -> np.ndarray:
    """Minimum linear index of each label 1..n, in label order."""
    flat = labels.ravel()
    n = int(flat.max()) if flat.size else 0
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return first[1:]
