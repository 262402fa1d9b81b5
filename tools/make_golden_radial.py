"""Generates tests/golden/golden_radial.npz: small scenes measured by SciPy and by boolean masks, the outside witness of
tests/radial_reference.py (cs_label_radial).

    python tools/make_golden_radial.py

SciPy 1.15.3 / numpy 2.2.6 wrote the committed file.  Per case i (one image), with `index` the labels present once the pixels
under `exclude` are taken out and C channels:
    image_i     uint8 / uint16 [H,W,C]     labels_i   int32 [H,W]     exclude_i   int32 [H,W] (all zero: none)     bins_i  int64
    index_i     int32 [n]
    d2_i        uint16 [H,W]: per object rint(scipy.ndimage.distance_transform_edt(np.pad(effective == l, 1)) ** 2), cropped
    center_i    int32 [n,4]: scipy.ndimage.maximum_position of d2 masked to the object (the first maximum in raster order),
                scipy.ndimage.maximum(d2, effective, index) and scipy.ndimage.sum_labels(d2 == 1, effective, index)
    edge_i      int64 [n,C,4]: scipy.ndimage.sum_labels of v and v^2, minimum and maximum over effective * (d2 == 1)
    ring_i      int64 [n,bins,8,1+C]: by a boolean mask per (object, ring, wedge), the ring from the integer rule on SciPy's d2 and
                centre
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
import radial_reference as RR                                                  # noqa: E402


def scipy_table(image, labels, exclude, bins):
    """SciPy and boolean masks on one image [H,W,C]."""
    eff = np.where(exclude != 0, 0, labels).astype(np.int32)
    index = np.unique(eff[eff > 0]).astype(np.int32)
    H, W = eff.shape
    C = image.shape[2]
    d2 = np.zeros((H, W), np.int64)
    for l in index:
        d = ndi.distance_transform_edt(np.pad(eff == l, 1))[1:-1, 1:-1]
        d2[eff == l] = np.rint(d * d).astype(np.int64)[eff == l]
    n = len(index)
    center = np.zeros((n, 4), np.int32)
    # per object on the masked plane: without `labels` maximum_position is the first maximum in raster order (an argmax); with
    # `labels` and `index` SciPy sorts the values first, and which of several equal maxima that leaves last is not defined
    center[:, :2] = np.array([ndi.maximum_position(np.where(eff == l, d2, 0)) for l in index], np.int32).reshape(n, 2)
    center[:, 2] = ndi.maximum(d2, eff, index)
    on_edge = eff * (d2 == 1)
    center[:, 3] = ndi.sum_labels(d2 == 1, eff, index)
    edge = np.zeros((n, C, 4), np.int64)
    ring = np.zeros((n, bins, 8, 1 + C), np.int64)
    rr, cc = np.mgrid[0:H, 0:W]
    for ch in range(C):
        v = image[:, :, ch].astype(np.int64)
        edge[:, ch, 0] = ndi.sum_labels(v, on_edge, index)
        edge[:, ch, 1] = ndi.sum_labels(v * v, on_edge, index)
        edge[:, ch, 2] = ndi.minimum(v, on_edge, index)
        edge[:, ch, 3] = ndi.maximum(v, on_edge, index)
    for k, l in enumerate(index):
        dr, dc = rr - int(center[k, 0]), cc - int(center[k, 1])
        c2 = dr * dr + dc * dc
        rg = sum(((bins - j) ** 2 * c2 >= j * j * d2).astype(np.int64) for j in range(1, bins)) if bins > 1 else np.zeros((H, W), np.int64)
        wd = (dr > 0).astype(np.int64) + 2 * (dc > 0) + 4 * (np.abs(dr) > np.abs(dc))
        for b in range(bins):
            for w in range(8):
                m = (eff == l) & (rg == b) & (wd == w)
                ring[k, b, w, 0] = m.sum()
                for ch in range(C):
                    ring[k, b, w, 1 + ch] = image[:, :, ch][m].astype(np.int64).sum()
    return dict(index=index, d2=d2.astype(np.uint16), center=center, edge=edge, ring=ring)


def touching_scene():
    """30 x 48: labels that touch with no background between them, one flush with three image edges, one in two pieces."""
    lab = np.zeros((30, 48), np.int32)
    lab[0:30, 0:10] = 1
    lab[3:27, 10:26] = 2
    lab[3:15, 26:44] = 3
    lab[15:27, 26:44] = 4
    lab[10:20, 20:32] = 5
    lab[0:2, 40:48] = 6
    lab[28:30, 40:48] = 6
    return lab


def cases():
    """(name, image, labels, exclude, bins)"""
    a = ER.disks((48, 100), 14, 1)
    nuclei = ER.disks((40, 64), 7, 3, radii=(2, 4))
    grown = ER.expand(nuclei, 16)[0]
    t = touching_scene()
    u = RR.u_shape()
    return [("48x100 disks, uint16 noise, 3 channels, 4 bins", IR.noise(a.shape, 3, np.uint16, 5), a, np.zeros_like(a), 4),
            ("40x64 rings: grown cells less their nuclei, uint8, 2 channels, 16 bins", IR.noise(grown.shape, 2, np.uint8, 7), grown, nuclei, 16),
            ("30x48 touching rectangles, uint8, 1 channel, 5 bins", IR.noise(t.shape, 1, np.uint8, 8), t, np.zeros_like(t), 5),
            ("a U-shaped object, uint16, 1 channel, 4 bins", IR.noise(u.shape, 1, np.uint16, 9), u, np.zeros_like(u), 4)]


def main():
    out = {}
    cs = cases()
    for i, (name, image, labels, exclude, bins) in enumerate(cs):
        t = scipy_table(image, labels, exclude, bins)
        print(f"{name}: {len(t['index'])} objects, {image.dtype} x {image.shape[2]}, deepest E2 {int(t['center'][:, 2].max())}, "
              f"{int(t['center'][:, 3].sum())} edge pixels")
        out.update({f"name_{i}": name, f"image_{i}": image, f"labels_{i}": labels.astype(np.int32), f"exclude_{i}": exclude.astype(np.int32),
                    f"bins_{i}": np.int64(bins)})
        out.update({f"{k}_{i}": v for k, v in t.items()})
    out["n_cases"] = np.int64(len(cs))
    out["scipy_version"] = scipy.__version__
    out["numpy_version"] = np.__version__
    path = os.path.join(ROOT, "tests", "golden", "golden_radial.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
