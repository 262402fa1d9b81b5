"""CPU restatement of the segmenter's Gaussian smoothing (cs_segment_smooth in csrc/segment.hip,
ThresholdSegmenter(smooth_sigma=...)): what the device kernels are compared against, with numpy only.

  smooth_weights  the fixed-point table w[0..r] of a sigma (an identical copy of cellscreen.segment.smooth_weights): r =
                  int(truncate * sigma + 0.5), e_k = 65536 * g_k / (g_0 + 2 * sum g_k) with g_k = exp(-k^2 / (2 sigma^2)),
                  w_k = floor(e_k), and the deficit 65536 - w_0 - 2 * sum w_k handed out by largest remainder over k >= 1 (ties
                  to the smaller k, +1 each, which costs 2), the centre taking the last 0 or 1.  w_0 + 2 * sum w_k = 65536.
  smooth          y = (A + 2^31) >> 32 with T(i, j) = sum_k w[|k|] x(i, fold(j + k, W)) and A(i, j) = sum_k w[|k|]
                  T(fold(i + k, H), j): separable, integers only, one rounding at the very end.  fold is local_reference.fold
                  (d c b a | a b c d, scipy's mode='reflect'; period 2 * side, so r may exceed a side).  T fits 32 bits and A
                  48; a constant image is a fixed point.  With median the plane of background_reference.median3 is smoothed.
  smooth_direct   the same straight from the definition: the 2-D sum of w[|di|] * w[|dj|] * x over folded indices
  tap_error       eps = sum over the 2r + 1 taps of |w / 65536 - g|, g the library's normalised float64 kernel
  bound           0.5 + top * (2 eps + eps^2) + 1e-6: how far y may lie from scipy.ndimage.gaussian_filter's float64 result
This is scipy.ndimage.gaussian_filter(x, sigma, mode='reflect', truncate=4.0) with the kernel quantised to 16 bits and the
result rounded to nearest once.  The library's own integer output truncates a float64 and depends on its last bit, so it is
not reproduced bit for bit; tests/golden/golden_smooth.npz (tools/make_golden_smooth.py) pins the float64 result instead."""
import math

import numpy as np

import background_reference as BR
from local_reference import fold

MAX_R = 64
ONE = 1 << 16


def smooth_weights(sigma: float, truncate: float = 4.0):
    r = int(truncate * sigma + 0.5)
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(r + 1)]
    norm = g[0] + 2.0 * sum(g[1:])
    e = [65536.0 * gk / norm for gk in g]
    w = [int(math.floor(ek)) for ek in e]
    deficit = ONE - w[0] - 2 * sum(w[1:])
    for k in sorted(range(1, r + 1), key=lambda k: (-(e[k] - w[k]), k)):
        if deficit < 2:
            break
        w[k] += 1
        deficit -= 2
    w[0] += deficit
    return w


def remainders(sigma: float, truncate: float = 4.0):
    """e_k - floor(e_k) of every tap: what the largest-remainder rule sorts by."""
    r = int(truncate * sigma + 0.5)
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(r + 1)]
    norm = g[0] + 2.0 * sum(g[1:])
    return [65536.0 * gk / norm - math.floor(65536.0 * gk / norm) for gk in g]


def check_table(w):
    w = [int(v) for v in w]
    r = len(w) - 1
    if not 1 <= r <= MAX_R:
        raise ValueError("radius outside 1..64")
    if min(w) < 0 or w[0] < 1 or w[0] + 2 * sum(w[1:]) != ONE:
        raise ValueError("weights must be non-negative with w[0] >= 1 and w[0] + 2 * sum(w[1:]) == 65536")
    return w


def _pass(x: np.ndarray, w) -> np.ndarray:
    """sum_k w[|k|] * x[:, fold(j + k)] along the last axis, uint64."""
    r, n = len(w) - 1, x.shape[1]
    p = x[:, fold(np.arange(-r, n + r), n)]
    out = np.uint64(w[0]) * x
    for k in range(1, r + 1):
        out = out + np.uint64(w[k]) * (p[:, r - k:r - k + n] + p[:, r + k:r + k + n])
    return out


def smooth(x: np.ndarray, w, median: bool = False) -> np.ndarray:
    """The smoothed plane of one 2-D uint8 / uint16 image under the table w."""
    if x.ndim != 2 or x.dtype not in (np.uint8, np.uint16):
        raise TypeError("2-D uint8 / uint16 image expected")
    w = check_table(w)
    if median:
        x = BR.median3(x)
    t = _pass(x.astype(np.uint64), w)
    assert int(t.max()) < 1 << 32
    a = _pass(np.ascontiguousarray(t.T), w).T
    return ((a + np.uint64(1 << 31)) >> np.uint64(32)).astype(x.dtype)


def smooth_direct(x: np.ndarray, w) -> np.ndarray:
    w = check_table(w)
    r = len(w) - 1
    H, W = x.shape
    k2 = np.array([[w[abs(di)] * w[abs(dj)] for dj in range(-r, r + 1)] for di in range(-r, r + 1)], dtype=object)
    xo = x.astype(object)
    out = np.zeros((H, W), x.dtype)
    for i in range(H):
        rows = fold(np.arange(i - r, i + r + 1), H)
        for j in range(W):
            cols = fold(np.arange(j - r, j + r + 1), W)
            out[i, j] = (int((k2 * xo[np.ix_(rows, cols)]).sum()) + (1 << 31)) >> 32
    return out


def smooth_sigma(x: np.ndarray, sigma: float, median: bool = False) -> np.ndarray:
    return smooth(x, smooth_weights(sigma), median)


def smooth_batch(images: np.ndarray, sigma: float, median: bool = False, channel=None) -> np.ndarray:
    if images.ndim == 3:
        chan = images
    else:
        ch = channel if channel is not None else (2 if images.shape[3] >= 3 else 0)
        chan = images[..., ch]
    w = smooth_weights(sigma)
    return np.stack([smooth(np.ascontiguousarray(c), w, median) for c in chan])


def library_kernel(sigma: float, radius: int) -> np.ndarray:
    """scipy.ndimage's normalised float64 Gaussian kernel of 2 * radius + 1 taps (_gaussian_kernel1d, order 0)."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def tap_error(w, sigma: float) -> float:
    r = len(w) - 1
    full = np.array([w[abs(k)] for k in range(-r, r + 1)], np.float64) / 65536.0
    return float(np.abs(full - library_kernel(sigma, r)).sum())


def bound(w, sigma: float, top: int) -> float:
    eps = tap_error(w, sigma)
    return 0.5 + top * (2.0 * eps + eps * eps) + 1e-6
