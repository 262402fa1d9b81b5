"""Generates tests/golden/golden_segment.npz with the REAL libraries the built-in segmenter is stated against.

Run with the image's conda interpreter (scikit-image 0.18.3, SciPy 1.7.1, numpy 1.26.4):

    /opt/conda/bin/python3.9 tests/golden/make_golden_segment.py

For a handful of small synthetic images (uint8 / uint16, at most 128 x 128) it stores the image and
    thr_i          skimage.filters.threshold_otsu(image)
    fill_i         scipy.ndimage.binary_fill_holes(image > thr_i)
    lab1_i, lab2_i skimage.measure.label(image > thr_i, connectivity=1 / 2)
    flab1_i, flab2_i   the same of fill_i
Nothing of the project is imported: these are library calls."""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from scipy import ndimage                                      # noqa: E402
from skimage.filters import threshold_otsu                     # noqa: E402
from skimage.measure import label                              # noqa: E402

# (H, W, dtype, kind)
CASES = [
    (48, 64, "u16", "cells"), (80, 64, "u8", "cells"), (64, 64, "u16", "rings"), (80, 72, "u8", "rings"),
    (32, 48, "u16", "noise"), (37, 53, "u8", "noise"), (32, 32, "u16", "two"), (16, 24, "u8", "const"),
    (64, 64, "u16", "touching"), (1, 70, "u8", "noise"), (70, 1, "u16", "noise"), (60, 80, "u16", "skew"),
]


def make_image(rng, H, W, dt, kind):
    top = 255 if dt == "u8" else 65535
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "const":
        img = np.full((H, W), 0.37)
    elif kind == "noise":
        img = rng.random((H, W))
    elif kind == "two":
        img = np.where(rng.random((H, W)) < 0.3, 0.8, 0.1)
    elif kind == "rings":
        img = 0.05 + 0.02 * rng.standard_normal((H, W))
        for _ in range(4):
            cy, cx, r = rng.uniform(10, H - 10), rng.uniform(10, W - 10), rng.uniform(6, 16)
            d = np.hypot(yy - cy, xx - cx)
            img[(d <= r) & (d >= 0.55 * r)] = 0.7 + 0.03 * rng.standard_normal()
            img[d <= 0.2 * r] = 0.7                              # an island inside the hole
    else:
        img = 0.05 + 0.02 * rng.standard_normal((H, W))
        n = 14 if kind == "touching" else 7
        for _ in range(n):
            cy, cx = rng.uniform(4, H - 4), rng.uniform(4, W - 4)
            ry, rx = rng.uniform(4, 12), rng.uniform(4, 12)
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            img[m] = rng.uniform(0.5, 0.9) + 0.03 * rng.standard_normal(int(m.sum()))
        if kind == "skew":
            img = img ** 3                                      # most of the range empty: long runs of zero bins
    img = np.clip(img, 0, 1)
    return np.round(img * top).astype(np.uint8 if dt == "u8" else np.uint16)


def main():
    rng = np.random.default_rng(20240611)
    out = {"n": np.int64(len(CASES))}
    for i, (H, W, dt, kind) in enumerate(CASES):
        img = make_image(rng, H, W, dt, kind)
        thr = threshold_otsu(img)
        mask = img > thr
        fill = ndimage.binary_fill_holes(mask)
        out[f"image_{i}"] = img
        out[f"thr_{i}"] = np.int64(thr)
        out[f"fill_{i}"] = fill
        for c in (1, 2):
            out[f"lab{c}_{i}"] = label(mask, connectivity=c).astype(np.int32)
            out[f"flab{c}_{i}"] = label(fill, connectivity=c).astype(np.int32)
    import scipy
    import skimage
    out["versions"] = np.array([f"scikit-image {skimage.__version__}", f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_segment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
