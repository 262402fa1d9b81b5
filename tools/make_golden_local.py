"""Generates tests/golden/golden_local.npz: small images and scikit-image's local mean threshold of them, the library twin of the
segmenter's threshold="local" (cs_segment_local, tests/local_reference.py).

Run with the conda interpreter that has scikit-image 0.18.3 (SciPy 1.7.1):

    python3.9 tools/make_golden_local.py

The integer rule and the library differ on purpose where n * (x - delta) equals the window's sum exactly: the float64 mean may
fall on either side of such a tie.  So every pixel here is odd (x | 1, which also leaves no zero pixel) and every delta is odd:
n = (2r + 1)^2 is odd, the sum of n odd numbers is odd, n * x is odd and n * delta is odd, so n * x - S - n * delta is odd and
never zero.  This tool asserts that before it writes, and then the comparison in tests/test_local_cpu.py is np.array_equal over
every pixel.

Per image i (uint8 and uint16; noise over the full range and a ramp; shapes up to 130 x 200):
    x_i              the image
    m_{r}_{d}_i      numpy.packbits of  x > skimage.filters.threshold_local(x, 2r + 1, method='mean', offset=-d)  for r in RADII
                     and d in DELTAS (d < 0 written as m<d>: m_7_m3_0)"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from skimage.filters import threshold_local                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_reference as LR                                                  # noqa: E402

SHAPES = [(37, 53), (17, 65), (130, 200), (3, 40)]
RADII = (1, 2, 7, 31, 64, 127, 255)
DELTAS = (-3, 1, 5)


def key(r, d, i):
    return f"m_{r}_{'m' + str(-d) if d < 0 else d}_{i}"


def images():
    rng = np.random.default_rng(20240921)
    out = []
    for dtype in (np.uint8, np.uint16):
        top = int(np.iinfo(dtype).max)
        for H, W in SHAPES:
            out.append((rng.integers(0, top + 1, (H, W)) | 1).astype(dtype))
            ramp = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5) * (top // 256 + 1) % (top + 1)
            out.append((ramp | 1).astype(dtype))
    return out


def main():
    out = {}
    xs = images()
    out["n"] = np.int64(len(xs))
    out["radii"] = np.array(RADII, np.int64)
    out["deltas"] = np.array(DELTAS, np.int64)
    for i, x in enumerate(xs):
        assert (x & 1).all()
        out[f"x_{i}"] = x
        for r in RADII:
            sums = LR.window_sum(x, r)
            for d in DELTAS:
                assert d & 1
                g = LR.margin(x, r, d, sums)
                assert (g != 0).all() and (g & 1).all(), (i, r, d)            # no tie can exist
                m = x > threshold_local(x, 2 * r + 1, method="mean", offset=-d)
                out[key(r, d, i)] = np.packbits(m)
    import scipy
    import skimage
    out["versions"] = np.array([f"scikit-image {skimage.__version__}", f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_local.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(xs), "images,", len(xs) * len(RADII) * len(DELTAS), "masks")


if __name__ == "__main__":
    main()
