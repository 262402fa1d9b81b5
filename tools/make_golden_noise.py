"""Generates tests/golden/golden_noise.npz: small images with the meshes and planes of the segmenter's noise-adaptive threshold
(cs_segment_noise) as tests/noise_reference.py computes them.

    python tools/make_golden_noise.py

Per image i (tests/noise_reference.py's golden_inputs: GOLDEN_SHAPES in uint8 and uint16):
    x_i, tile_i      the image and its tile side
    mesh_{f}_i       int32 [2, my, mx], the filtered mesh under floor8 = f, for each floor8 among GOLDEN_RULES
    p_{r}_i          numpy.packbits of the 0 / 1 plane under rule r of GOLDEN_RULES (k8, weak8, floor8, connectivity)
No library computes this rule (SExtractor, SEP and photutils cut the same way in floating point, with other statistics, and none
of them is on the machine this file was made on), so the file is no outside witness: it pins the restatement against drift, and
tests/test_noise_cpu.py holds the restatement to a slow form in exact rationals that shares no code with it."""
import os
import sys

import numpy as np
import scipy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_reference as NR                                                   # noqa: E402


def main():
    out = {}
    inputs = NR.golden_inputs()
    out["n"] = np.int64(len(inputs))
    out["rules"] = np.array([[k8, -1 if w is None else w, f, c] for k8, w, f, c in NR.GOLDEN_RULES], np.int64)
    for i, (x, T) in enumerate(inputs):
        out[f"x_{i}"] = x
        out[f"tile_{i}"] = np.int64(T)
        for f in sorted({r[2] for r in NR.GOLDEN_RULES}):
            out[f"mesh_{f}_{i}"] = NR.mesh(x, T, f)
        for r, (k8, weak8, f, c) in enumerate(NR.GOLDEN_RULES):
            out[f"p_{r}_{i}"] = np.packbits(NR.noise_mask(x, T, k8, weak8, f, c))
    out["versions"] = np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_noise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(inputs), "images")


if __name__ == "__main__":
    main()
