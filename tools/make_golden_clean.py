"""Generates tests/golden/golden_clean.npz: small masks and SciPy's answers to the two steps of the segmenter's mask cleanup
(cs_segment_clean, tests/clean_reference.py).

    python tools/make_golden_clean.py            # SciPy 1.15.3

Per mask i (tests/clean_reference.py's mask_inputs over SHAPES: noise, bridged blobs, full, empty, checkerboard, frames):
    x_i              numpy.packbits of the mask; shape_i its shape
    o_{r}_{k}_i      numpy.packbits of scipy.ndimage.binary_opening(x, generate_binary_structure(2, k), iterations=r)
    d_{a}_{c}_i      numpy.packbits of the mask without its components (scipy.ndimage.label, connectivity c) of fewer than a
                     pixels (numpy.bincount of the labels): skimage.morphology.remove_small_objects(x, a, c) by its definition;
                     scikit-image itself is not used
The tool also asserts what the restatement relies on: r iterations equal one opening by scipy.ndimage.iterate_structure, and an
all-foreground mask opens to itself under the square where its sides reach 2r + 1 (the erosion eats r pixels from the border, where
outside counts as background; a smaller mask does not survive that and opens to nothing, and the diamond grows back all but the
image's corners: the image is a rectangle in a sea of background, and a diamond rounds a rectangle's corners)."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_reference as CR                                                   # noqa: E402

SHAPES = [(1, 1), (1, 9), (9, 1), (37, 53), (17, 65), (40, 70)]
RADII = (1, 2, 3, 7)
AREAS = (1, 2, 5, 64)


def main():
    out = {}
    masks = [m for shape in SHAPES for _, m in CR.mask_inputs(shape)]
    out["n"] = np.int64(len(masks))
    out["radii"] = np.array(RADII, np.int64)
    out["areas"] = np.array(AREAS, np.int64)
    for i, x in enumerate(masks):
        out[f"x_{i}"] = np.packbits(x)
        out[f"shape_{i}"] = np.array(x.shape, np.int64)
        for k in (1, 2):
            st = ndimage.generate_binary_structure(2, k)
            for r in RADII:
                o = ndimage.binary_opening(x, st, iterations=r)
                assert np.array_equal(o, ndimage.binary_opening(x, ndimage.iterate_structure(st, r))), (i, r, k)
                if x.all() and k == 2:                                         # the border erodes r pixels, which grow back
                    assert o.all() == (min(x.shape) >= 2 * r + 1), (i, r, k)   # where a pixel is left to grow from
                out[f"o_{r}_{k}_{i}"] = np.packbits(o)
        for c in (1, 2):
            lab, _ = ndimage.label(x, structure=ndimage.generate_binary_structure(2, c))
            sizes = np.bincount(lab.ravel())
            for a in AREAS:
                keep = sizes >= a
                keep[0] = False
                out[f"d_{a}_{c}_{i}"] = np.packbits(keep[lab])
    out["versions"] = np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_clean.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(masks), "masks")


if __name__ == "__main__":
    main()
