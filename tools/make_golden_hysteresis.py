"""Generates tests/golden/golden_hysteresis.npz: small level planes and SciPy's answer to the linking step of the segmenter's
hysteresis threshold (cs_segment_hysteresis, tests/hysteresis_reference.py).

    python tools/make_golden_hysteresis.py       # SciPy 1.15.3

Per plane i (tests/hysteresis_reference.py's level_inputs over SHAPES):
    lo_i, hi_i       numpy.packbits of the weak mask (level > 0) and of the strong mask (level == 2); shape_i its shape
    h_{c}_i          numpy.packbits of the answer under connectivity c, computed in the very form of the body of
                     skimage.filters.apply_hysteresis_threshold:
                         labels_low, num_labels = ndimage.label(mask_low)
                         sums = ndimage.sum(mask_high, labels_low, numpy.arange(num_labels + 1))
                         connected_to_high = sums > 0
                         thresholded = connected_to_high[labels_low]
                     with the 8-neighbour structure passed to ndimage.label for c = 2 (the library's function has connectivity
                     1 only).  scikit-image itself is not on the machine this file was made on and is not used: the body is
                     three SciPy calls, and they are what is pinned.
The tool also asserts what the restatement relies on: the strong mask is a subset of the weak one in every input."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hysteresis_reference as HR                                              # noqa: E402

SHAPES = [(1, 1), (1, 9), (9, 1), (37, 53), (17, 65), (40, 70), (130, 200)]


def apply_hysteresis(mask_low, mask_high, connectivity):
    labels_low, num_labels = ndimage.label(mask_low, structure=ndimage.generate_binary_structure(2, connectivity))
    sums = ndimage.sum(mask_high, labels_low, np.arange(num_labels + 1))
    connected_to_high = sums > 0
    return connected_to_high[labels_low]


def main():
    out = {}
    planes = [lv for shape in SHAPES for _, lv in HR.level_inputs(shape)]
    out["n"] = np.int64(len(planes))
    for i, lv in enumerate(planes):
        lo, hi = lv > 0, lv == 2
        assert not (hi & ~lo).any()
        out[f"lo_{i}"] = np.packbits(lo)
        out[f"hi_{i}"] = np.packbits(hi)
        out[f"shape_{i}"] = np.array(lv.shape, np.int64)
        for c in (1, 2):
            out[f"h_{c}_{i}"] = np.packbits(apply_hysteresis(lo, hi, c))
    out["versions"] = np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_hysteresis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(planes), "planes")


if __name__ == "__main__":
    main()
