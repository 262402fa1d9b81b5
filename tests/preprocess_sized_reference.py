"""CPU reference of the crop preprocess at any output size -- TEST INFRASTRUCTURE ONLY.

oracle/preprocess_oracle.py restates improved_detection.py:98-99 for the reference's (64, 64); `resize_to_64(x, s)` there
takes one side.  This is the same function with separate out_h / out_w -- the resize a user gets by editing the one line
`resize(cell_image_eq, (H, W), anti_aliasing=True)` -- built from that module's own _gauss1d, _warp_reflect and
equalize_adapthist, with the same operations in the same order (bit-equal to resize_to_64 for square sizes).  It is pinned
to real scikit-image 0.18.3 / SciPy 1.7.1 outputs by tests/golden/golden_preprocess_sized.npz
(tests/golden/make_golden_preprocess_sized.py)."""
import numpy as np

from oracle import preprocess_oracle as po


def resize_to(image, out_h, out_w):
    """skimage.transform.resize(image, (out_h, out_w), anti_aliasing=True) for a float64 2-D image: per axis
    gaussian_filter(sigma=max(0, (factor-1)/2), mode='mirror') -- an axis that is not scaled down is not filtered --, then
    the bilinear warp with half-pixel centres, mode='reflect', clipped to the blurred image's range."""
    x = np.asarray(image, dtype=np.float64)
    H, W = x.shape
    fr, fc = H / float(out_h), W / float(out_w)
    sr, sc = max(0.0, (fr - 1.0) / 2.0), max(0.0, (fc - 1.0) / 2.0)
    if sr > 1e-15:
        x = po._gauss1d(x, sr, 0)
    if sc > 1e-15:
        x = po._gauss1d(x, sc, 1)
    lo, hi = x.min(), x.max()
    r = fr * np.arange(out_h, dtype=np.float64) + (fr * 0.5 - 0.5)
    c = fc * np.arange(out_w, dtype=np.float64) + (fc * 0.5 - 0.5)
    r0, c0 = np.floor(r), np.floor(c)
    r1, c1 = np.ceil(r), np.ceil(c)
    dr, dc = (r - r0)[:, None], (c - c0)[None, :]
    r0i, r1i = po._warp_reflect(r0.astype(np.int64), H), po._warp_reflect(r1.astype(np.int64), H)
    c0i, c1i = po._warp_reflect(c0.astype(np.int64), W), po._warp_reflect(c1.astype(np.int64), W)
    top = (1.0 - dc) * x[np.ix_(r0i, c0i)] + dc * x[np.ix_(r0i, c1i)]
    bot = (1.0 - dc) * x[np.ix_(r1i, c0i)] + dc * x[np.ix_(r1i, c1i)]
    out = (1.0 - dr) * top + dr * bot
    return np.clip(out, lo, hi)


def preprocess_crop(image, out_hw, clip_limit=0.02):
    """One crop through improved_detection.py:98-99 with resize(., out_hw); float64 (out_h, out_w)."""
    return resize_to(po.equalize_adapthist(image, clip_limit), int(out_hw[0]), int(out_hw[1]))


def preprocess_crops(images, out_hw, clip_limit=0.02):
    """List of 2-D uint8/uint16 crops -> float32 [n,out_h,out_w] (the cast of improved_detection.py:122)."""
    out = np.empty((len(images), int(out_hw[0]), int(out_hw[1])), dtype=np.float32)
    for i, im in enumerate(images):
        out[i] = preprocess_crop(im, out_hw, clip_limit).astype(np.float32)
    return out
