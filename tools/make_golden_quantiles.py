"""Generates tests/golden/golden_quantiles.npz: small label images whose objects are measured by numpy.quantile, numpy.median
and scipy.stats.median_abs_deviation, the outside witness of tests/quantile_reference.py (cs_label_quantiles).

    python tools/make_golden_quantiles.py

numpy 2.2.6 and SciPy 1.15.3 wrote the committed file.  The four kinds of case are golden_intensity.npz's.  Per case i, with
`index` the labels present once the pixels under `exclude` are taken out, and the twelve quantiles of q_num / q_den:
    image_i     uint8 / uint16 [H,W,C]       labels_i   int32 [H,W]       exclude_i   int32 [H,W] (all zero: none)
    index_i     int32 [n]                    count_i    int64 [n]
    linear_i, lower_i, higher_i   float64 [n,C,12]: np.quantile(v, num / den, method=...) of the object's values as float64
    median_i    float64 [n,C]: np.median     mad_i      float64 [n,C]: scipy.stats.median_abs_deviation (scale 1)
    name_i
n_cases counts them."""
import os
import sys

import numpy as np
import scipy
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quantile_reference as QR                                                # noqa: E402
from make_golden_intensity import cases                                        # noqa: E402


def numpy_table(image, labels, exclude, quantiles=QR.TWELVE):
    """The numpy / SciPy calls on one image [H,W,C], object by object on float64 copies, as a caller without the device makes them."""
    lab = np.where(exclude != 0, 0, labels)
    index = np.unique(lab[lab > 0]).astype(np.int32)
    q = np.array([num / den for num, den in quantiles])
    n, nc = len(index), image.shape[2]
    out = dict(index=index, count=np.zeros(n, np.int64), median=np.zeros((n, nc)), mad=np.zeros((n, nc)))
    for k in ("linear", "lower", "higher"):
        out[k] = np.zeros((n, nc, len(q)))
    for i, label in enumerate(index):
        where = lab == label
        out["count"][i] = where.sum()
        for ch in range(nc):
            v = image[:, :, ch][where].astype(np.float64)
            for k in ("linear", "lower", "higher"):
                out[k][i, ch] = np.quantile(v, q, method=k)
            out["median"][i, ch] = np.median(v)
            out["mad"][i, ch] = stats.median_abs_deviation(v)
    return out


def main():
    out = {"q_num": np.array([a for a, _ in QR.TWELVE], np.int32), "q_den": np.array([b for _, b in QR.TWELVE], np.int32)}
    cs = cases()
    for i, (name, image, labels, exclude) in enumerate(cs):
        t = numpy_table(image, labels, exclude)
        print(f"{name}: {len(t['index'])} objects, {image.dtype} x {image.shape[2]}")
        out.update({f"name_{i}": name, f"image_{i}": image, f"labels_{i}": labels.astype(np.int32), f"exclude_{i}": exclude.astype(np.int32)})
        out.update({f"{k}_{i}": v for k, v in t.items()})
    out["n_cases"] = np.int64(len(cs))
    out["numpy_version"] = np.__version__
    out["scipy_version"] = scipy.__version__
    path = os.path.join(ROOT, "tests", "golden", "golden_quantiles.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
