"""Writes tests/golden/golden_texture.npz: small scenes and their texture records (cs_label_texture) from the slow form
of tests/texture_reference.py, one Python loop over the pixel pairs, so that a later change of the vectorised restatement, or of
the rule, is noticed.  The file is pinned to the rule as include/cellscreen.h states it, not to a library: neither mahotas nor
scikit-image took part.

Usage: python tools/make_golden_texture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cell-image-analysis_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NOTE = "records of tests/texture_reference.measure_slow: pinned to the rule of cs_label_texture, not to a library"


def cases():
    """(name, image [B,H,W,C], labels, exclude, distance, levels, ranges)"""
    import texture_reference as TR
    shape = (14, 19)
    lab = np.stack([TR.disks(shape, 4, 1, radii=(3, 5)), TR.disks(shape, 4, 2, radii=(3, 5))])
    ring = np.stack([TR.disks(shape, 4, 1, radii=(1, 2)), np.zeros(shape, np.int32)])
    two = np.zeros((1,) + shape, np.int32)
    two[0, :4, :5] = 2
    two[0, -4:, -5:] = 2
    two[0, 6:8, 2:17] = 1
    smooth = (np.add.outer(np.arange(14) * 900, np.arange(19) * 2500) % 65536).astype(np.uint16)[None, :, :, None]
    return [("uint8 noise C2 d1 L8", TR.noise((2,) + shape, 2, np.uint8, 3), lab, np.zeros_like(lab), 1, 8, [(0, 255), (16, 200)]),
            ("uint16 noise C1 d2 L13 exclude", TR.noise((2,) + shape, 1, np.uint16, 4), lab, ring, 2, 13, [(0, 65535)]),
            ("uint16 ramp C1 d3 L64 two pieces", smooth, two, np.zeros_like(two), 3, 64, [(1000, 50000)]),
            ("uint8 noise C3 d5 L2", TR.noise((1,) + shape, 3, np.uint8, 5), two, np.zeros_like(two), 5, 2, [(0, 255)] * 3)]


def main():
    import texture_reference as TR
    out = {"note": np.array(NOTE), "n_cases": np.array(len(cases()))}
    for i, (name, image, labels, ex, d, levels, ranges) in enumerate(cases()):
        count, marg, sumsq, clogc, glcm = TR.measure_slow(image, labels, d, levels, ranges, ex, glcm=True)
        out.update({f"name_{i}": np.array(name), f"image_{i}": image, f"labels_{i}": labels, f"exclude_{i}": ex,
                    f"distance_{i}": np.array(d), f"levels_{i}": np.array(levels), f"ranges_{i}": np.array(ranges, np.int32),
                    f"count_{i}": count, f"marg_{i}": marg, f"sumsq_{i}": sumsq, f"clogc_{i}": clogc, f"glcm_{i}": glcm})
    path = os.path.join(ROOT, "tests", "golden", "golden_texture.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
