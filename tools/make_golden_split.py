"""Generates tests/golden/golden_split.npz: small masks with the stages of the split_touching option, each taken
from the library that defines the same thing, and the labels of the restatement where no library does.

Run with the conda interpreter that has scikit-image 0.18.3 (SciPy 1.7.1):

    python3.9 tools/make_golden_split.py

Per mask i, connectivity c in (1, 2) and h in (1, 3, 8):
    mask_i          the boolean mask (at most 96 x 128)
    d2_i            scipy.ndimage.distance_transform_edt(mask) ** 2, rounded (int32; 2^30 where the mask has no background)
    dq_i            min(math.isqrt(4 * d2), 255)
    r_{c}_{h}_i     skimage.morphology.reconstruction(max(dq - h, 0), dq, 'dilation', <the c-neighbourhood>)
    seed_{c}_{h}_i  skimage.morphology.local_maxima(where(mask, r + 1, 0), connectivity=c) & mask  (the + 1 keeps a component
                    whose r is 0 everywhere apart from the background, which the definition does by looking inside the mask;
                    a mask without background is one plateau and one seed, where the library reports no maximum at all)
    lab_{c}_{h}_i   tests/split_reference.py's labels: the flooding rule has no library twin
    agree_{c}_{h}_i share of mask pixels on which skimage.segmentation.watershed(-dq, seeds, mask=mask) -- which breaks
                    ties by queue order -- puts the same pixels together (a record for DESIGN 3k, not a gate)."""
import math
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from scipy import ndimage                                                     # noqa: E402
from skimage.morphology import local_maxima, reconstruction                   # noqa: E402
from skimage.segmentation import watershed                                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import split_reference as SR                                                  # noqa: E402

HS = (1, 3, 8)


def disks(H, W, spec):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.any([(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r for cy, cx, r in spec], axis=0)


def masks():
    rng = np.random.default_rng(20240907)
    out = [disks(64, 96, [(30, 28, 18), (30, 60, 18), (52, 84, 6)]),                       # an equal touching pair, one alone
           disks(80, 128, [(40, 36, 28), (40, 72, 10), (20, 104, 9), (34, 112, 9), (48, 104, 9)]),     # 28/10 pair, a triple
           disks(48, 48, [(10, 10, 7), (36, 36, 9)]),                                       # nothing to split
           np.ones((24, 40), bool), np.zeros((16, 16), bool), np.ones((1, 1), bool)]
    m = np.ones((40, 70), bool)
    m[20, 35] = False                                                                       # one background pixel
    out.append(m)
    out.append(rng.random((48, 64)) < 0.62)                                                 # percolation noise
    m = np.zeros((96, 128), bool)
    for _ in range(16):                                                                     # a crowded field of ellipses
        cy, cx, ry, rx = rng.uniform(8, 88), rng.uniform(8, 120), rng.uniform(5, 14), rng.uniform(5, 14)
        yy, xx = np.mgrid[0:96, 0:128]
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    out.append(m)
    m = disks(64, 64, [(32, 32, 26)]) & ~disks(64, 64, [(32, 32, 12)])                      # a ring: one plateau all around
    out.append(m)
    out.append(np.ones((1, 50), bool) & (np.arange(50) % 17 != 0)[None])                    # one row
    bar = np.zeros((30, 90), bool)
    bar[8:22, 4:86] = True                                                                  # a bar: a long ridge plateau
    out.append(bar)
    return out


def main():
    out = {}
    ms = masks()
    out["n"] = np.int64(len(ms))
    for i, m in enumerate(ms):
        out[f"mask_{i}"] = m
        if m.all():
            d2 = np.full(m.shape, 2 ** 30, np.int64)
        else:
            d2 = np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64)
        dq = np.array([min(math.isqrt(4 * int(v)), 255) for v in d2.ravel()], np.uint8).reshape(m.shape)
        out[f"d2_{i}"] = d2.astype(np.int32)
        out[f"dq_{i}"] = dq
        for c in (1, 2):
            st = ndimage.generate_binary_structure(2, c)
            for h in HS:
                marker = np.maximum(dq.astype(np.int16) - h, 0).astype(np.uint8)
                r = reconstruction(marker, dq, method="dilation", selem=st).astype(np.uint8)
                seed = local_maxima(np.where(m, r.astype(np.int16) + 1, 0), connectivity=c).astype(bool) & m
                if m.all():
                    seed = m.copy()                 # the library calls a constant image free of maxima; here it is one plateau
                lab, n, dq_r = SR.split_mask(m, c, h)
                assert np.array_equal(dq_r, dq)
                out[f"r_{c}_{h}_{i}"] = r
                out[f"seed_{c}_{h}_{i}"] = seed
                out[f"lab_{c}_{h}_{i}"] = lab
                markers, ns = ndimage.label(seed, structure=st)
                assert ns == n, (i, c, h, ns, n)
                ws = watershed(-dq.astype(np.int16), markers, connectivity=c, mask=m)
                # the same partition: compare through the seeds' own labels
                of_seed = np.zeros(ns + 1, np.int64)
                of_seed[markers[seed]] = lab[seed]
                out[f"agree_{c}_{h}_{i}"] = np.float64((of_seed[ws][m] == lab[m]).mean() if m.any() else 1.0)
    import scipy
    import skimage
    out["versions"] = np.array([f"scikit-image {skimage.__version__}", f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(ROOT, "tests", "golden", "golden_split.npz")
    np.savez_compressed(path, **out)
    agree = {k: float(out[k]) for k in out if k.startswith("agree_")}
    px = {k: int(out["mask_" + k.rsplit("_", 1)[1]].sum()) for k in agree}
    print("wrote", path, os.path.getsize(path), "bytes; watershed agreement: worst %.4f (%s), over all mask pixels %.4f"
          % (min(agree.values()), min(agree, key=agree.get), sum(agree[k] * px[k] for k in agree) / sum(px.values())))


if __name__ == "__main__":
    main()
