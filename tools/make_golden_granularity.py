"""Generates tests/golden/golden_granularity.npz: small scenes measured by SciPy's own filters and labelled sums, the outside
witness of tests/granularity_reference.py (cs_label_granularity).

    python tools/make_golden_granularity.py

SciPy 1.15.3 / numpy 2.2.6 wrote the committed file.  Per case i (one image), with `index` the labels present once the pixels
under `exclude` are taken out, C channels and K steps:
    image_i     uint8 / uint16 [H,W,C]     labels_i   int32 [H,W]     exclude_i   int32 [H,W] (all zero: none)
    steps_i, subsample_i, masked_i  int64
    index_i     int32 [n]
    planes_i    uint16 [K+1,C,Hs,Ws]: P by a Python loop over the blocks, then per step scipy.ndimage.grey_erosion(footprint=cross,
                mode='reflect') and the reconstruction by scipy.ndimage.grey_dilation(footprint=cross, mode='constant', cval=0)
                and numpy.minimum, repeated until nothing changes
    sums_i      int64 [n,K+1,C]: scipy.ndimage.sum_labels of the plane read back at [r // s][c // s], over the effective labels
    image_sums_i int64 [K+1,C]
    name_i
n_cases counts them."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expand_reference as ER                                                  # noqa: E402
import intensity_reference as IR                                               # noqa: E402

CROSS = ndi.generate_binary_structure(2, 1)


def scipy_table(image, labels, exclude, steps, s, masked):
    """SciPy on one image [H,W,C]."""
    eff = np.where(exclude != 0, 0, labels).astype(np.int32)
    index = np.unique(eff[eff > 0]).astype(np.int32)
    H, W, C = image.shape
    hs, ws = -(-H // s), -(-W // s)
    planes = np.zeros((steps + 1, C, hs, ws), np.int64)
    for ch in range(C):
        for R in range(hs):
            for Cc in range(ws):
                blk = image[R * s:(R + 1) * s, Cc * s:(Cc + 1) * s, ch].astype(np.int64)
                if masked:
                    blk = blk * (eff[R * s:(R + 1) * s, Cc * s:(Cc + 1) * s] > 0)
                planes[0, ch, R, Cc] = (2 * int(blk.sum()) + blk.size) // (2 * blk.size)
        p = planes[0, ch]
        e = p
        for k in range(1, steps + 1):
            e = ndi.grey_erosion(e, footprint=CROSS, mode="reflect")
            r = e
            while True:
                n = np.minimum(ndi.grey_dilation(r, footprint=CROSS, mode="constant", cval=0), p)
                if np.array_equal(n, r):
                    break
                r = n
            planes[k, ch] = r
    rr, cc = np.mgrid[0:H, 0:W]
    sums = np.zeros((len(index), steps + 1, C), np.int64)
    for k in range(steps + 1):
        for ch in range(C):
            full = planes[k, ch][rr // s, cc // s]
            sums[:, k, ch] = np.rint(ndi.sum_labels(full, eff, index)).astype(np.int64)      # below 2^53: exact in float64
    return dict(index=index, planes=planes.astype(np.uint16), sums=sums, image_sums=planes.sum(axis=(2, 3)))


def speckles(shape, seed, dtype):
    """Smooth blobs with 3 x 3 and single-pixel speckles on a low noisy background, two channels."""
    rng = np.random.default_rng(seed)
    H, W = shape
    top = np.iinfo(dtype).max
    a = rng.integers(0, top // 16 + 1, (H, W, 2)).astype(np.int64)
    for _ in range(12):
        r, c = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1))
        a[r - 1:r + 2, c - 1:c + 2, 0] += top // 2
        a[r, c, 1] += top // 3
    yy, xx = np.mgrid[0:H, 0:W]
    a[..., 1] += (top // 4 * np.exp(-((yy - H / 2) ** 2 + (xx - W / 2) ** 2) / 60.0)).astype(np.int64)
    return np.clip(a, 0, top).astype(dtype)


def cases():
    """(name, image, labels, exclude, steps, subsample, masked)"""
    a = ER.disks((40, 64), 9, 1)
    nuclei = ER.disks((37, 61), 7, 3, radii=(2, 4))
    grown = ER.expand(nuclei, 6)[0]
    z = np.zeros_like
    return [("40x64 disks, uint16 speckles, 2 channels, 5 steps", speckles(a.shape, 1, np.uint16), a, z(a), 5, 1, 0),
            ("37x61 rings: grown cells less their nuclei, uint8 noise, 3 channels, 4 steps, masked", IR.noise(grown.shape, 3, np.uint8, 7), grown,
             nuclei, 4, 1, 1),
            ("37x61 grown cells, uint16 speckles, block means of 2, 3 steps", speckles(grown.shape, 2, np.uint16), grown, z(grown), 3, 2, 0),
            ("40x64 disks, uint8 speckles, block means of 4, masked, 2 steps", speckles(a.shape, 3, np.uint8), a, z(a), 2, 4, 1)]


def main():
    out = {}
    cs = cases()
    for i, (name, image, labels, exclude, steps, s, masked) in enumerate(cs):
        t = scipy_table(image, labels, exclude, steps, s, masked)
        print(f"{name}: {len(t['index'])} objects, {image.dtype} x {image.shape[2]}, image sums {t['image_sums'][:, 0].tolist()}")
        out.update({f"name_{i}": name, f"image_{i}": image, f"labels_{i}": labels.astype(np.int32), f"exclude_{i}": exclude.astype(np.int32),
                    f"steps_{i}": np.int64(steps), f"subsample_{i}": np.int64(s), f"masked_{i}": np.int64(masked)})
        out.update({f"{k}_{i}": v for k, v in t.items()})
    out["n_cases"] = np.int64(len(cs))
    out["scipy_version"] = scipy.__version__
    out["numpy_version"] = np.__version__
    path = os.path.join(ROOT, "tests", "golden", "golden_granularity.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
