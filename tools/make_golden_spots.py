"""Generates tests/golden/golden_spots.npz: small scenes with SciPy's float64 difference of Gaussians and its maximum filter, the
outside witness of tests/spots_reference.py (cs_spot_detect), and the restatement's own records on scenes with
deliberate ties, which pin the tie rule against a later edit.

    python tools/make_golden_spots.py

SciPy 1.15.3 wrote the committed file.  Per SciPy case i (n_cases of them):
    image_i    uint8 / uint16 [H,W]          sigma_i    float64 [2]: fine (0: the image itself) and coarse          m_i, T_i
    dog_i      float64 [H,W]: gaussian_filter(x, fine) - gaussian_filter(x, coarse), mode='reflect', truncate=4.0, x as float64
    maxf_i     int32 [H,W]: maximum_filter(R, 2 m + 1, mode='constant', cval=INT32_MIN) of the restatement's integer response R
                (the float planes tie where the integers do not and the other way round, so the peak comparison is on R)
Per tie scene j (n_ties of them): tie_image_j uint16 [B,H,W], tie_labels_j int32 [B,H,W], tie_params_j int64 [4] (sigma in
1/1000, coarse in 1/1000, m, T), and the restatement's tie_counts_j, tie_offsets_j, tie_list_j, tie_geom_j, tie_records_j."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_reference as SM                                                  # noqa: E402
import spots_reference as SR                                                   # noqa: E402


def tables(fine, coarse):
    return (None if fine == 0 else SM.smooth_weights(fine)), SM.smooth_weights(coarse)


def scipy_cases():
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:48, 0:64]
    blobs = 300.0 + sum(2500.0 * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * s * s)) for y, x, s in ((10, 12, 1.2), (30, 40, 2.0), (40, 8, 1.0), (5, 60, 1.5)))
    return [(np.clip(np.rint(blobs + rng.normal(0, 12, blobs.shape)), 0, 65535).astype(np.uint16), 1.0, 1.6, 2, 40 * 256),
            (rng.integers(0, 65536, (21, 33)).astype(np.uint16), 2.0, 3.2, 3, 256),
            (rng.integers(0, 256, (17, 9)).astype(np.uint8), 0.0, 1.0, 1, 64),
            (rng.integers(0, 4096, (9, 11)).astype(np.uint16), 3.0, 5.0, 1, 16)]                 # radii above both sides


def tie_scenes():
    a = np.full((3, 24, 30), 200, np.uint16)
    a[0, 10:12, 10:12] = 3000                                                  # a 2 x 2 plateau
    a[0, 5, 20] = a[0, 5, 22] = 3000                                           # equal peaks 2 apart
    yy, xx = np.mgrid[0:24, 0:30]
    a[1] = (500 + 1500 * ((yy // 2 + xx // 2) & 1)).astype(np.uint16)          # a checkerboard
    lab = np.zeros(a.shape, np.int32)                                          # the third image is constant
    lab[0, 2:14, 2:26], lab[0, 14:22, 2:12], lab[1, :, :15], lab[1, :, 15:] = 1, 2, 3, 1
    return [(a, lab, 0.0, 1.0, 2, 1), (a, lab, 1.0, 1.6, 1, 1)]


def main():
    out = {"scipy_version": np.array(scipy.__version__)}
    cases = scipy_cases()
    for i, (x, fine, coarse, m, T) in enumerate(cases):
        f = x.astype(np.float64)
        low = f if fine == 0 else ndi.gaussian_filter(f, fine, mode="reflect", truncate=4.0)
        R = SR.response(x, *tables(fine, coarse))
        out.update({f"image_{i}": x, f"sigma_{i}": np.array([fine, coarse]), f"m_{i}": np.array(m), f"T_{i}": np.array(T),
                    f"dog_{i}": low - ndi.gaussian_filter(f, coarse, mode="reflect", truncate=4.0),
                    f"maxf_{i}": ndi.maximum_filter(R, 2 * m + 1, mode="constant", cval=SR.INT32_MIN)})
    out["n_cases"] = np.array(len(cases))
    ties = tie_scenes()
    for j, (a, lab, fine, coarse, m, T) in enumerate(ties):
        counts, offsets, lst, geom, rec, _ = SR.detect(a, [T] * len(a), *tables(fine, coarse), m, 0, lab, None, 3)
        out.update({f"tie_image_{j}": a, f"tie_labels_{j}": lab, f"tie_params_{j}": np.array([round(1000 * fine), round(1000 * coarse), m, T], np.int64),
                    f"tie_counts_{j}": counts, f"tie_offsets_{j}": offsets, f"tie_list_{j}": lst, f"tie_geom_{j}": geom, f"tie_records_{j}": rec})
    out["n_ties"] = np.array(len(ties))
    path = os.path.join(ROOT, "tests", "golden", "golden_spots.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
