"""Generates tests/golden/golden_illumination.npz: the flat-field correction of tests/illumination_reference.py's GOLDEN_CASES
(cs_illum_tile_stats / cs_illum_reduce / cs_illum_apply), which pins that restatement against drift.

    python tools/make_golden_illumination.py

No library computes this rule, so the file records the restatement's own results; tests/test_illumination_cpu.py holds the
restatement to a slow form in exact rationals and its optional filters to SciPy.  Per case i:
    image_i    the input stack, uint8 / uint16 [B,H,W] or [B,H,W,C]
    out_i      the corrected stack, the input's dtype and shape
    clipped_i  int64 [B,C,2]: the pixels clamped at 0 and at top
    F8_i       int32 [C,my,mx]: the function in 1/256 counts
    G8_i       int64 [C]: the scale
n_cases counts them; the parameters of a case are GOLDEN_CASES[i]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import illumination_reference as IR                                            # noqa: E402


def main():
    out = {}
    for i, (case, (y, clipped, F8, G8)) in enumerate(zip(IR.GOLDEN_CASES, IR.golden_outputs())):
        image = IR.golden_field(case[0], case[1])
        print(f"case {i}: {image.shape} {image.dtype}, T {case[2]}, mesh {F8.shape[1:]}, G8 {G8}, clipped {clipped.sum(axis=(0, 1)).tolist()}")
        out.update({f"image_{i}": image, f"out_{i}": y, f"clipped_{i}": clipped, f"F8_{i}": F8, f"G8_{i}": np.array(G8, np.int64)})
    out["n_cases"] = np.int64(len(IR.GOLDEN_CASES))
    path = os.path.join(ROOT, "tests", "golden", "golden_illumination.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
