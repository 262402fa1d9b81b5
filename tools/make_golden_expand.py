"""Generates tests/golden/golden_expand.npz: small label images grown by skimage.segmentation.expand_labels, the outside witness
of tests/expand_reference.py (cs_label_expand).

    python tools/make_golden_expand.py

scikit-image is not a dependency, so its six lines are restated here over scipy.ndimage.distance_transform_edt (SciPy 1.15.3
wrote the committed file).  Per case i:
    labels_i    int32, at most 70 x 300: random disks of radius 3..7, ids 1..n or sparse up to 2^31 - 1
    distance_i  float64, what the library was given; max_d2_i its integer form (tests/expand_reference.py, max_d2_of)
    lib_i       int32: expand_labels(labels_i, distance_i)
    d2_i        uint16: 0 on labelled pixels, the library's squared distance where `distances <= distance`, 65535 elsewhere
    tie_i       bool: the grown pixels whose nearest labelled pixels carry more than one label, found from all pairwise integer
                distances; there the library's choice follows its scan order and the project's rule takes the smallest label
    name_i
n_cases counts them."""
import os
import sys

import numpy as np
import scipy
from scipy.ndimage import distance_transform_edt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expand_reference as ER                                                  # noqa: E402


def expand_labels(label_image, distance):
    """skimage.segmentation.expand_labels, restated."""
    distances, nearest = distance_transform_edt(label_image == 0, return_indices=True)
    labels_out = np.zeros_like(label_image)
    dilate_mask = distances <= distance
    masked_nearest = [dim[dilate_mask] for dim in nearest]
    labels_out[dilate_mask] = label_image[tuple(masked_nearest)]
    return labels_out, distances, dilate_mask


def tie_mask(lab, grown):
    """The grown pixels with more than one label among their nearest labelled pixels."""
    ys, xs = np.nonzero(lab > 0)
    ids = lab[ys, xs].astype(np.int64)
    out = np.zeros(lab.shape, bool)
    for y, x in zip(*np.nonzero(grown & (lab == 0))):
        d = (ys - y) ** 2 + (xs - x) ** 2
        out[y, x] = len(np.unique(ids[d == d.min()])) > 1
    return out


def cases():
    sparse = [7, 3, 2 ** 31 - 1, 1000003, 12, 2 ** 30, 5, 99]
    a = ER.disks((70, 300), 40, 1)
    b = ER.disks((97, 131), 25, 2)
    c = ER.disks((64, 64), 8, 3, ids=sparse)
    return [("70x300 d3", a, 3), ("70x300 d5", a, 5), ("70x300 d12", a, 12), ("97x131 d5", b, 5), ("97x131 d127", b, 127),
            ("64x64 sparse ids d1.5", c, 1.5), ("64x64 sparse ids d2.9", c, 2.9), ("64x64 sparse ids d12", c, 12),
            ("64x64 sparse ids d127", c, 127)]


def main():
    out = {}
    cs = cases()
    for i, (name, lab, distance) in enumerate(cs):
        lib, distances, grown = expand_labels(lab, distance)
        sq = np.rint(distances * distances).astype(np.int64)
        d2 = np.where(lab > 0, 0, np.where(grown, sq, ER.FAR)).astype(np.uint16)
        tie = tie_mask(lab, grown)
        n_grown = int((grown & (lab == 0)).sum())
        print(f"{name}: {n_grown} grown pixels, {int(tie.sum())} ties ({100.0 * tie.sum() / max(n_grown, 1):.2f} %)")
        out.update({f"name_{i}": name, f"labels_{i}": lab.astype(np.int32), f"distance_{i}": np.float64(distance),
                    f"max_d2_{i}": np.int64(ER.max_d2_of(distance)), f"lib_{i}": lib.astype(np.int32), f"d2_{i}": d2, f"tie_{i}": tie})
    out["n_cases"] = np.int64(len(cs))
    out["scipy_version"] = scipy.__version__
    path = os.path.join(ROOT, "tests", "golden", "golden_expand.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
