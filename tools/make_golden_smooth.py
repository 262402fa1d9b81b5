"""Generates tests/golden/golden_smooth.npz: small images, the segmenter's fixed-point Gaussian tables and SciPy's float64
gaussian_filter of the images, the library twin of the segmenter's smooth_sigma (cs_segment_smooth,
tests/smooth_reference.py).

Run with SciPy 1.15.3:

    python tools/make_golden_smooth.py

The integer rule is not the library's own integer output (that one truncates a float64 and depends on its last bit); what is
pinned is the float64 result f = scipy.ndimage.gaussian_filter(x.astype(float64), sigma, mode='reflect', truncate=4.0), which
tests/test_smooth_cpu.py holds the restatement to within 0.5 + top * (2 eps + eps^2) + 1e-6 on every pixel stored here.

A table must not depend on the last bit of exp: this tool asserts that no e_k = 65536 g_k / sum g of a tabulated sigma lies
within 1e-6 of a half, and that no two remainders of one table lie within 1e-9 of each other unless they are equal.

    sigmas           the tabulated sigmas
    w_{s}            int32 table w[0..r] of sigmas[s]
    n                number of images
    x_i              image i (uint8 and uint16; full-range noise, a ramp, saturated; 1 x 1, 3 x 40, 17 x 33, 37 x 53, 130 x 200)
    rows_i, cols_i   the rows and columns of image i whose outputs are stored: all of them for images of up to 600 pixels, a
                     grid that keeps both edges for the larger ones (float64 noise does not compress)
    f_{s}_i          float64 gaussian_filter output of image i under sigmas[s] at rows_i x cols_i"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_reference as SM                                                 # noqa: E402

SIGMAS = (0.25, 1.0, 2.0, 4.0, 8.0, 15.875)
SHAPES = [(1, 1), (3, 40), (17, 33), (37, 53), (130, 200)]
FULL_PIXELS = 600


def images():
    rng = np.random.default_rng(20241017)
    out = []
    for dtype in (np.uint8, np.uint16):
        top = int(np.iinfo(dtype).max)
        for H, W in SHAPES:
            out.append(rng.integers(0, top + 1, (H, W)).astype(dtype))
            if H * W <= 2000:
                ramp = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5) * (top // 256 + 1) % (top + 1)
                out.append(ramp.astype(dtype))
                out.append(np.full((H, W), top, dtype))
    return out


def grid(n, step):
    return np.array(sorted(set(range(0, n, step)) | {n - 1}), np.int64)


def main():
    out = {"sigmas": np.array(SIGMAS, np.float64)}
    for s, sigma in enumerate(SIGMAS):
        rem = SM.remainders(sigma)
        e_half = min(abs(v - 0.5) for v in rem)
        assert e_half > 1e-6, (sigma, e_half)                                 # no e_k near a half
        srt = sorted(rem[1:])
        assert all(b - a > 1e-9 or b == a for a, b in zip(srt, srt[1:])), sigma         # the order of the remainders is robust
        w = SM.smooth_weights(sigma)
        SM.check_table(w)
        out[f"w_{s}"] = np.array(w, np.int32)
    xs = images()
    out["n"] = np.int64(len(xs))
    for i, x in enumerate(xs):
        H, W = x.shape
        full = H * W <= FULL_PIXELS
        rows, cols = (np.arange(H), np.arange(W)) if full else (grid(H, max(1, H // 18)), grid(W, max(1, W // 24)))
        out[f"x_{i}"], out[f"rows_{i}"], out[f"cols_{i}"] = x, rows, cols
        for s, sigma in enumerate(SIGMAS):
            f = ndimage.gaussian_filter(x.astype(np.float64), sigma, mode="reflect", truncate=4.0)
            out[f"f_{s}_{i}"] = f[np.ix_(rows, cols)]
    out["versions"] = np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_smooth.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400_000, size
    print("wrote", path, size, "bytes,", len(xs), "images,", len(xs) * len(SIGMAS), "outputs")


if __name__ == "__main__":
    main()
