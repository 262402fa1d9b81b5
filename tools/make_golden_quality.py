"""Generates tests/golden/golden_quality.npz: small scenes measured by scipy.ndimage's filters and labelled statistics, the outside
witness of tests/quality_reference.py (cs_image_quality and cs_object_focus).

    python tools/make_golden_quality.py

SciPy 1.15.3 wrote the committed file.  The filters run on int64 copies (mode='reflect', whose border values never count: every
plane is cropped to the interior, the pixels with a full 3 x 3 neighbourhood, before anything is summed):
    L  = ndimage.laplace(x)                                  G = ndimage.sobel(x, 0)^2 + ndimage.sobel(x, 1)^2
    Br = ndimage.correlate(x, [[-1, 0, 1]])^2 + ndimage.correlate(x, [[-1], [0], [1]])^2
Per case i:
    image_i     uint8 / uint16 [H,W,C]       labels_i   int32 [H,W]       exclude_i   int32 [H,W] (all zero: none)
    sat_i       int32 [C]: the saturation levels          tile_i     the mesh's tile side
    image_rec_i int64 [C,13]: n, sum v, sum v^2, min, max (ndimage.minimum / maximum), n_at_min, n_at_max, n_sat, n_int, sum L,
                sum L^2, sum G, sum Br over the whole image
    mesh_i      int64 [C,m_r,m_c,8]: ndimage.sum over a label plane of the mesh tiles, built from CellProfiler's float grid
                int(i * float(m) / float(side)): n, sum v, sum v^2, n_int, sum L, sum L^2, sum G, sum Br
    index_i     int32 [n]: the labels present once the pixels under `exclude` are taken out
    focus_i     int64 [n,C,5]: ndimage.sum over those labels of the interior indicator, L, L^2, G, Br (planes zero off the interior)
    name_i
n_cases counts them.  ndimage.sum works in float64: every sum here is below 2^53, checked, so the int64 casts are exact."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expand_reference as ER                                                  # noqa: E402
import quality_reference as QR                                                 # noqa: E402


def scipy_planes(x):
    """(interior indicator, L, L^2, G, Br) of one channel, int64 [H,W], zero off the interior."""
    x = x.astype(np.int64)
    lap = ndi.laplace(x)
    g = ndi.sobel(x, 0) ** 2 + ndi.sobel(x, 1) ** 2
    br = ndi.correlate(x, np.array([[-1, 0, 1]])) ** 2 + ndi.correlate(x, np.array([[-1], [0], [1]])) ** 2
    inside = np.zeros(x.shape, np.int64)
    inside[1:-1, 1:-1] = 1
    return [inside] + [p * inside for p in (lap, lap * lap, g, br)]


def exact(a):
    a = np.asarray(a, np.float64)
    assert (np.abs(a) < 2.0 ** 53).all()
    return a.astype(np.int64)


def scipy_tables(image, labels, exclude, sat, tile):
    H, W, nc = image.shape
    m_r, m_c = QR.mesh_dims(H, W, tile)
    rows = np.array([int(i * float(m_r) / float(H)) for i in range(H)])         # CellProfiler's grid, in floats
    cols = np.array([int(j * float(m_c) / float(W)) for j in range(W)])
    tiles = (rows[:, None] * m_c + cols[None, :] + 1).astype(np.int32)
    lab = np.where(exclude != 0, 0, labels)
    index = np.unique(lab[lab > 0]).astype(np.int32)
    rec = np.zeros((nc, 13), np.int64)
    mesh = np.zeros((nc, m_r, m_c, 8), np.int64)
    focus = np.zeros((len(index), nc, 5), np.int64)
    for ch in range(nc):
        v = image[:, :, ch].astype(np.int64)
        planes = scipy_planes(v)
        lo, hi = int(ndi.minimum(v)), int(ndi.maximum(v))
        rec[ch] = [v.size, v.sum(), (v * v).sum(), lo, hi, (v == lo).sum(), (v == hi).sum(), (v >= sat[ch]).sum()] + [p.sum() for p in planes]
        for j, p in enumerate([np.ones_like(v), v, v * v] + planes):
            mesh[ch, :, :, j] = exact(ndi.sum(p, tiles, np.arange(1, m_r * m_c + 1))).reshape(m_r, m_c)
        for j, p in enumerate(planes):
            focus[:, ch, j] = exact(ndi.sum(p, lab, index))
    return dict(image_rec=rec, mesh=mesh, index=index, focus=focus)


def blurred(shape, channels, dtype, seed, sigma):
    """Noise smoothed by a Gaussian: what a defocused field looks like next to the raw noise."""
    a = QR.noise(shape, channels, dtype, seed).astype(np.float64)
    return np.stack([ndi.gaussian_filter(a[:, :, c], sigma) for c in range(channels)], axis=2).round().astype(dtype)


def cases():
    a = ER.disks((40, 64), 9, 1)
    b = ER.disks((33, 50), 6, 2)
    nuclei = ER.disks((36, 48), 5, 3, radii=(2, 4))
    grown = ER.expand(nuclei, 16)[0]
    clipped = QR.noise((20, 37), 2, np.uint8, 14)
    clipped[:, :20, 0] = 255                                                    # half a channel clipped, the other dark
    clipped[:, :, 1] = 0
    whole = np.ones((20, 37), np.int32)
    whole[0, :] = 0
    return [("40x64 disks, uint16 noise, 3 channels, tile 16", QR.noise(a.shape, 3, np.uint16, 11), a, np.zeros_like(a), [65535, 60000, 1], 16),
            ("33x50 disks, uint16 noise blurred by sigma 2, tile 17", blurred(b.shape, 1, np.uint16, 12, 2.0), b, np.zeros_like(b), [40000], 17),
            ("36x48 rings: grown cells less their nuclei, uint8, 4 channels, tile 16", QR.noise(grown.shape, 4, np.uint8, 13), grown, nuclei,
             [255, 200, 0, 256], 16),
            ("20x37 clipped and dark channels, uint8, one object to the border, tile 16", clipped, whole, np.zeros_like(whole), [255, 255], 16)]


def main():
    out = {}
    cs = cases()
    for i, (name, image, labels, exclude, sat, tile) in enumerate(cs):
        t = scipy_tables(image, labels, exclude, sat, tile)
        print(f"{name}: {len(t['index'])} objects, {image.dtype} x {image.shape[2]}, mesh {t['mesh'].shape[1:3]}")
        out.update({f"name_{i}": name, f"image_{i}": image, f"labels_{i}": labels.astype(np.int32), f"exclude_{i}": exclude.astype(np.int32),
                    f"sat_{i}": np.array(sat, np.int32), f"tile_{i}": np.int64(tile)})
        out.update({f"{k}_{i}": v for k, v in t.items()})
    out["n_cases"] = np.int64(len(cs))
    out["scipy_version"] = scipy.__version__
    path = os.path.join(ROOT, "tests", "golden", "golden_quality.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
