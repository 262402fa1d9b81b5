"""Generates tests/golden/golden_preprocess_sized.npz with the REAL libraries the reference calls, for output sizes other
than the reference's (64, 64).

Run with the image's conda interpreter (scikit-image 0.18.3, SciPy 1.7.1, numpy 1.26.4):

    /opt/conda/bin/python3.9 tests/golden/make_golden_preprocess_sized.py

For every (crop, output size) pair of CASES it stores the crop and

    out_i : resize(exposure.equalize_adapthist(crop, clip_limit=0.02), (out_h, out_w), anti_aliasing=True)   (float64)

i.e. improved_detection.py:98-99 with the one edit a model of another input_shape needs.  The pairs cover up- and
down-scaling, one axis each way, the boundary ratio side = 16 x out, a constant and a saturated crop, and sizes from (8, 8)
to (256, 256) with non-square ones.  Few large outputs, many small ones: float64 outputs hardly compress and the file has
to stay below 1 MB.  Nothing from the reference project is imported: the two calls are library calls.
"""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from skimage import exposure                                   # noqa: E402
from skimage.transform import resize                           # noqa: E402

from make_golden_preprocess import make_crop                   # noqa: E402  (the same synthetic crops)

CLIP = 0.02

# (H, W, dtype, kind, (out_h, out_w))
CASES = [
    (8, 8, "u8", "noise", (8, 8)),              # smallest crop, smallest output: identity
    (8, 8, "u8", "noise", (128, 128)),          # 16x up-scale on both axes
    (16, 16, "u16", "blob", (32, 32)),
    (23, 31, "u8", "blob", (64, 128)),          # up both, non-square
    (37, 52, "u16", "blob", (128, 64)),
    (48, 40, "u8", "blob", (32, 32)),           # down both
    (100, 71, "u16", "blob", (128, 48)),        # rows up, columns down
    (37, 152, "u16", "blob", (32, 256)),        # rows down, columns up
    (181, 97, "u16", "blob", (96, 48)),
    (128, 90, "u8", "blob", (8, 8)),            # rows at the boundary ratio 16
    (40, 256, "u8", "blob", (48, 16)),          # columns at the boundary ratio 16
    (33, 33, "u8", "const", (256, 256)),        # constant crop, largest output
    (72, 56, "u8", "sat", (48, 128)),
    (56, 72, "u16", "flat", (16, 16)),
    (15, 120, "u16", "noise", (256, 32)),
    (64, 64, "u16", "noise", (64, 128)),        # rows untouched, columns up
    (200, 150, "u8", "blob", (128, 128)),       # down both to the large model's size
    (9, 15, "u8", "blob", (8, 8)),
    (127, 128, "u8", "blob", (64, 32)),
    (64, 64, "u8", "blob", (96, 96)),
]


def main():
    rng = np.random.default_rng(20250311)
    out = {"n": np.int64(len(CASES)), "clip_limit": np.float64(CLIP)}
    for i, (H, W, dt, kind, hw) in enumerate(CASES):
        crop = make_crop(rng, H, W, dt, kind)
        eq = exposure.equalize_adapthist(crop, clip_limit=CLIP)
        out[f"crop_{i}"] = crop
        out[f"hw_{i}"] = np.array(hw, np.int64)
        out[f"out_{i}"] = resize(eq, hw, anti_aliasing=True)
        assert out[f"out_{i}"].dtype == np.float64 and out[f"out_{i}"].shape == hw
    import skimage, scipy
    out["versions"] = np.array([f"scikit-image {skimage.__version__}", f"scipy {scipy.__version__}",
                                f"numpy {np.__version__}"])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_preprocess_sized.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
