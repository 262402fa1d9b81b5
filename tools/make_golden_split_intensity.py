"""Generates tests/golden/golden_split_intensity.npz: small guide + mask pairs with the heights and the labels of the
split_by="intensity" option as tests/split_intensity_reference.py computes them.

    python tools/make_golden_split_intensity.py

Note on what this pins.  scikit-image is not installed where this was written, so nothing here comes from its watershed or its
h-maxima; the reconstruction, the seeds and the flood are split_reference's, which golden_split.npz pins to scikit-image 0.18.3
on distance planes.  `heights` is pinned to SciPy 1.15.3 only: its components are scipy.ndimage.label's and its ranges
scipy.ndimage.minimum / maximum, and this script checks them against a plain loop over the components before it records them.
The labels are a record of the restatement on planes of this kind, so that a later change of it shows.

Per pair i (guide_i uint8 / uint16, mask_i bool, contrast_i = the min_contrast used), connectivity c in (1, 2), depth d in (4, 16, 64):
    hq_{c}_i        heights(mask, guide, c, contrast)
    lab_{c}_{d}_i   split_intensity(mask, guide, c, d, contrast)[0]
    n_{c}_{d}_i     its region count
    base_{c}_i      scipy.ndimage.label's component count of the mask"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segment_reference as R                                                 # noqa: E402
import smooth_reference as MR                                                 # noqa: E402
import split_intensity_reference as IR                                        # noqa: E402

DEPTHS = (4, 16, 64)


def cells(H, W, spec, background=300.0):
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.full((H, W), float(background))
    for cy, cx, r, a in spec:
        f += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.5 * r) ** 2))
    return f


def pairs():
    """(name, guide, mask, min_contrast)"""
    rng = np.random.default_rng(20261018)
    out = []
    g = MR.smooth_sigma(IR.scene(60.0), 1.5)                                                # the specifying scene
    out.append(("scene", g, R.mask_of(g, R.otsu(g), True), 0))
    f = cells(64, 128, [(20, 20, 12, 200), (20, 36, 12, 200), (44, 80, 12, 20000), (44, 96, 12, 20000)])
    g = np.rint(f).astype(np.uint16)                                                        # a dim pair beside a bright pair
    out.append(("dim_bright", g, g > 360, 0))
    f = cells(56, 96, [(28, 28, 16, 90000), (28, 62, 14, 30000)])
    g = np.rint(np.clip(f, 0, 65535)).astype(np.uint16)                                     # a saturated core: a plateau at 65535
    out.append(("saturated", g, g > 2000, 0))
    yy, xx = np.mgrid[0:40, 0:48]
    disk = (yy - 20) ** 2 + (xx - 24) ** 2 <= 15 ** 2
    out.append(("flat", np.where(disk, 1000, 300).astype(np.uint16), disk, 0))               # a constant component: all 1
    m = np.zeros((12, 20), bool)
    m[3, 4] = m[8, 15] = m[0, 0] = m[11, 19] = True
    out.append(("one_pixel", rng.integers(0, 65536, (12, 20)).astype(np.uint16), m, 0))     # components of one pixel
    out.append(("noise_u8", rng.integers(0, 256, (48, 64)).astype(np.uint8), rng.random((48, 64)) < 0.62, 0))
    ramp = np.linspace(0, 65535, 16 * 40).reshape(16, 40)
    out.append(("full_ramp", np.rint(ramp).astype(np.uint16), np.ones((16, 40), bool), 0))  # 0 and 65535 in one component
    out.append(("empty", rng.integers(0, 256, (9, 13)).astype(np.uint8), np.zeros((9, 13), bool), 0))
    f = cells(48, 80, [(24, 24, 14, 600), (24, 56, 14, 600)], 400.0) + rng.normal(0.0, 12.0, (48, 80))
    g = np.rint(f).astype(np.uint16)                                                        # two faint cells, noisy tops ...
    out.append(("faint", g, g > 520, 0))
    out.append(("faint_guarded", g, g > 520, 20000))                                        # ... not stretched: nothing splits
    g8 = MR.smooth_sigma(IR.scene(60.0, dtype=np.uint8), 1.5)[:85, :130]                    # the uint8 scene's upper left
    out.append(("scene_u8", np.ascontiguousarray(g8), R.mask_of(g8, R.otsu(g8), True), 0))
    return out


def heights_by_loop(mask, guide, connectivity, contrast):
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(2, connectivity))
    out = np.zeros(mask.shape, np.uint8)
    for k in range(1, n + 1):
        sel = lab == k
        v = [int(x) for x in guide[sel]]
        lo, span = min(v), max(max(v) - min(v), contrast, 1)
        out[sel] = [1 + ((x - lo) * 254) // span for x in v]
    return out, n


def main():
    assert scipy.__version__ == "1.15.3", scipy.__version__
    out = {}
    ps = pairs()
    out["n"] = np.int64(len(ps))
    out["names"] = np.array([p[0] for p in ps])
    for i, (name, g, m, contrast) in enumerate(ps):
        out[f"guide_{i}"], out[f"mask_{i}"], out[f"contrast_{i}"] = g, m, np.int64(contrast)
        for c in (1, 2):
            hq = IR.heights(m, g, c, contrast)
            loop, base = heights_by_loop(m, g, c, contrast)
            assert hq.dtype == np.uint8 and np.array_equal(hq, loop), (name, c)
            out[f"hq_{c}_{i}"], out[f"base_{c}_{i}"] = hq, np.int64(base)
            for d in DEPTHS:
                lab, n, hq2 = IR.split_intensity(m, g, c, d, contrast)
                assert np.array_equal(hq2, hq)
                out[f"lab_{c}_{d}_{i}"], out[f"n_{c}_{d}_{i}"] = lab, np.int64(n)
            print(name, g.dtype, g.shape, "c", c, "components", base, "regions", [int(out[f"n_{c}_{d}_{i}"]) for d in DEPTHS])
    out["versions"] = np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])
    out["note"] = np.array("heights pinned to SciPy 1.15.3 (ndimage.label / minimum / maximum) only; labels are the restatement's own: "
                           "scikit-image was not available")
    path = os.path.join(ROOT, "tests", "golden", "golden_split_intensity.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
