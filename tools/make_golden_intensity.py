"""Generates tests/golden/golden_intensity.npz: small label images measured by scipy.ndimage's labelled statistics, the outside
witness of tests/intensity_reference.py (cs_label_intensity).

    python tools/make_golden_intensity.py

scikit-image is not a dependency: regionprops' intensity properties are these SciPy calls (SciPy 1.15.3 wrote the committed
file).  Per case i, with `index` the labels present once the pixels under `exclude` are taken out:
    image_i     uint8 / uint16 [H,W,C]       labels_i   int32 [H,W]       exclude_i   int32 [H,W] (all zero: none)
    index_i     int32 [n]
    area_i      float64 [n]: ndimage.sum of ones            centroid_i  float64 [n,2]: center_of_mass of ones
    sum_i, mean_i, std_i, min_i, max_i   float64 [n,C]: ndimage.sum / mean / standard_deviation / minimum / maximum of the channel as
                float64
    wc_i        float64 [n,C,2]: center_of_mass of the channel (NaN where the object's sum is 0)
    name_i
n_cases counts them."""
import os
import sys
import warnings

import numpy as np
import scipy
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expand_reference as ER                                                  # noqa: E402
import intensity_reference as IR                                               # noqa: E402


def scipy_table(image, labels, exclude):
    """The SciPy calls on one image [H,W,C]; float64 copies, as a caller without the device would make them."""
    lab = np.where(exclude != 0, 0, labels)
    index = np.unique(lab[lab > 0]).astype(np.int32)
    ones = np.ones(lab.shape)
    out = dict(index=index, area=np.asarray(ndi.sum(ones, lab, index), np.float64),
               centroid=np.asarray(ndi.center_of_mass(ones, lab, index), np.float64).reshape(len(index), 2))
    per = {k: [] for k in ("sum", "mean", "std", "min", "max", "wc")}
    for ch in range(image.shape[2]):
        v = image[:, :, ch].astype(np.float64)
        per["sum"].append(ndi.sum(v, lab, index))
        per["mean"].append(ndi.mean(v, lab, index))
        per["std"].append(ndi.standard_deviation(v, lab, index))
        per["min"].append(ndi.minimum(v, lab, index))
        per["max"].append(ndi.maximum(v, lab, index))
        with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
            warnings.simplefilter("ignore")
            per["wc"].append(np.asarray(ndi.center_of_mass(v, lab, index), np.float64).reshape(len(index), 2))
    for k in ("sum", "mean", "std", "min", "max"):
        out[k] = np.stack([np.asarray(x, np.float64) for x in per[k]], axis=1)
    out["wc"] = np.stack(per["wc"], axis=1)
    return out


def cases():
    a = ER.disks((48, 100), 14, 1)
    b = ER.disks((40, 60), 8, 2)
    nuclei = ER.disks((40, 64), 7, 3, radii=(2, 4))
    grown = ER.expand(nuclei, 16)[0]
    sparse = ER.disks((24, 40), 5, 4, ids=[7, 1000, 3, 5000, 12])
    dark = IR.noise((24, 40), 2, np.uint8, 8)
    dark[:, :, 1] = 0                                                           # a channel without light: sum v = 0
    zero = np.zeros_like(a)
    return [("48x100 disks, uint16 noise, 3 channels", IR.noise(a.shape, 3, np.uint16, 5), a, zero),
            ("40x60 disks, uint16 60000 + U[0,600)", IR.noise(b.shape, 1, np.uint16, 6, base=60000, spread=600), b, np.zeros_like(b)),
            ("40x64 rings: grown cells less their nuclei, uint8, 4 channels", IR.noise(grown.shape, 4, np.uint8, 7), grown, nuclei),
            ("24x40 sparse ids, uint8, a dark channel", dark, sparse, np.zeros_like(sparse))]


def main():
    out = {}
    cs = cases()
    for i, (name, image, labels, exclude) in enumerate(cs):
        t = scipy_table(image, labels, exclude)
        print(f"{name}: {len(t['index'])} objects, {image.dtype} x {image.shape[2]}")
        out.update({f"name_{i}": name, f"image_{i}": image, f"labels_{i}": labels.astype(np.int32), f"exclude_{i}": exclude.astype(np.int32)})
        out.update({f"{k}_{i}": v for k, v in t.items()})
    out["n_cases"] = np.int64(len(cs))
    out["scipy_version"] = scipy.__version__
    path = os.path.join(ROOT, "tests", "golden", "golden_intensity.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
