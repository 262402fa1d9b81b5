"""CPU restatement of the segmenter's noise-adaptive threshold (cs_segment_noise in csrc/segment.hip,
ThresholdSegmenter(threshold="noise", ...)): what the device kernels are compared against, with numpy sorts and int64
arithmetic only (DESIGN 3r has the definition).

  axis_tiles     the tiles of one axis: m = max(1, n // T), tile i = [i T, (i + 1) T), the last one runs to n
  tile_stats     per tile: med = the value of rank (N - 1) // 2 in sorted order, dev = the same rank of |x - med|;
                 B8 = 256 med, S8 = max((dev * 97164) >> 8, floor8), both int64 [my, mx]
  filter3        the median (fifth of nine) of the 3 x 3 mesh neighbourhood, the mesh replicated at its edges
  mesh           int32 [2, my, mx] after the filter: B8 then S8
  axis_weights   per pixel of one axis: the two nodes, their weights w0, w1 and D = w0 + w1 (bilinear between tile centres at the
                 doubled coordinates C2_i = start_i + end_i - 1, constant outside the outer centres, one node: D = 1, w0 = 1)
  maps           (N_B, N_S, D) per pixel, int64
  levels         0 background, 1 where 256 (256 v D - N_B) > weak8 N_S only, 2 where it is > k8 N_S; without a weak rule
                 (weak8 None or -1) the plane is 0 / 1
  noise_mask     the 0 / 1 plane: levels, linked by tests/hysteresis_reference.py's hysteresis with a weak rule
  segment        noise_mask, then what the segmenter does with a mask; the threshold reported is -1
No library computes this rule; tests/golden/golden_noise.npz (tools/make_golden_noise.py) pins this file against drift, and
tests/test_noise_cpu.py checks it against a slow form in exact rationals."""
import numpy as np

import hysteresis_reference as HR
import local_reference as LR

MAD_Q16 = 97164                                                  # 1.4826 * 65536


def k8_of(k: float) -> int:
    return int(float(k) * 256 + 0.5)


def axis_tiles(n: int, T: int):
    """[(start, end)] with end exclusive."""
    m = max(1, n // T)
    return [(i * T, (i + 1) * T if i < m - 1 else n) for i in range(m)]


def _check(x, T, floor8):
    if x.ndim != 2 or x.dtype not in (np.uint8, np.uint16):
        raise TypeError("2-D uint8 / uint16 plane expected")
    if T not in (16, 32, 64, 128, 256):
        raise ValueError("tile: a power of two in 16..256")
    if not 0 <= floor8 <= 4095 * 256:
        raise ValueError("floor8 outside 0..4095 * 256")


def tile_stats(x: np.ndarray, T: int, floor8: int):
    _check(x, T, floor8)
    ty, tx = axis_tiles(x.shape[0], T), axis_tiles(x.shape[1], T)
    B8 = np.zeros((len(ty), len(tx)), np.int64)
    S8 = np.zeros_like(B8)
    for j, (y0, y1) in enumerate(ty):
        for i, (x0, x1) in enumerate(tx):
            v = np.sort(x[y0:y1, x0:x1].astype(np.int64).ravel())
            r = (v.size - 1) // 2
            med = int(v[r])
            dev = int(np.sort(np.abs(v - med))[r])
            B8[j, i] = 256 * med
            S8[j, i] = max((dev * MAD_Q16) >> 8, floor8)
    return B8, S8


def filter3(a: np.ndarray) -> np.ndarray:
    p = np.pad(a, 1, mode="edge")
    my, mx = a.shape
    nine = np.stack([p[dy:dy + my, dx:dx + mx] for dy in range(3) for dx in range(3)])
    return np.sort(nine, axis=0)[4]


def mesh(x: np.ndarray, T: int, floor8: int) -> np.ndarray:
    B8, S8 = tile_stats(x, T, floor8)
    return np.stack([filter3(B8), filter3(S8)]).astype(np.int32)


def axis_weights(n: int, T: int):
    """(i0, i1, w0, w1, D), int64 [n] each."""
    tiles = axis_tiles(n, T)
    c2 = np.array([s + e - 1 for s, e in tiles], np.int64)
    p2 = 2 * np.arange(n, dtype=np.int64)
    if len(tiles) == 1:
        z = np.zeros(n, np.int64)
        return z, z, z + 1, z, z + 1
    i0 = np.clip(np.searchsorted(c2, p2, side="right") - 1, 0, len(tiles) - 2)
    D = c2[i0 + 1] - c2[i0]
    w1 = np.clip(p2 - c2[i0], 0, D)
    return i0, i0 + 1, D - w1, w1, D


def maps(x: np.ndarray, T: int, floor8: int, m=None):
    """(N_B, N_S, D) of every pixel; m: the filtered mesh, if the caller has it."""
    m = (mesh(x, T, floor8) if m is None else m).astype(np.int64)
    y0, y1, wy0, wy1, Dy = axis_weights(x.shape[0], T)
    x0, x1, wx0, wx1, Dx = axis_weights(x.shape[1], T)

    def interp(a):
        return (wy0[:, None] * (wx0[None, :] * a[y0][:, x0] + wx1[None, :] * a[y0][:, x1]) +
                wy1[:, None] * (wx0[None, :] * a[y1][:, x0] + wx1[None, :] * a[y1][:, x1]))

    return interp(m[0]), interp(m[1]), Dy[:, None] * Dx[None, :]


def levels(x: np.ndarray, T: int, k8: int, weak8=None, floor8: int = 256, m=None) -> np.ndarray:
    if not 1 <= k8 <= 16383:
        raise ValueError("k8 outside 1..16383")
    if weak8 is not None and weak8 != -1 and not 1 <= weak8 <= k8:
        raise ValueError("weak8 outside 1..k8")
    NB, NS, D = maps(x, T, floor8, m)
    lhs = 256 * (256 * x.astype(np.int64) * D - NB)
    strong = (lhs > k8 * NS).astype(np.uint8)
    if weak8 is None or weak8 == -1:
        return strong
    return strong + (lhs > weak8 * NS).astype(np.uint8)


def noise_mask(x: np.ndarray, T: int = 64, k8: int = 1280, weak8=None, floor8: int = 256, connectivity: int = 1) -> np.ndarray:
    lv = levels(x, T, k8, weak8, floor8)
    return lv if weak8 is None or weak8 == -1 else HR.hysteresis(lv, connectivity)


def segment(channel: np.ndarray, T: int = 64, k8: int = 1280, weak8=None, floor8: int = 256, connectivity: int = 1,
            fill_holes: bool = True):
    """(labels, n_labels, -1) of one 2-D image."""
    return LR.label_plane(noise_mask(channel, T, k8, weak8, floor8, connectivity), connectivity, fill_holes)


def _channel(images, channel):
    if images.ndim == 3:
        return images
    return images[..., channel if channel is not None else (2 if images.shape[3] >= 3 else 0)]


def mesh_batch(images: np.ndarray, T: int = 64, floor8: int = 256, channel=None) -> np.ndarray:
    return np.stack([mesh(np.ascontiguousarray(c), T, floor8) for c in _channel(images, channel)])


def noise_mask_batch(images: np.ndarray, channel=None, **kw) -> np.ndarray:
    return np.stack([noise_mask(np.ascontiguousarray(c), **kw) for c in _channel(images, channel)])


def segment_batch(images: np.ndarray, channel=None, **kw):
    out = [segment(np.ascontiguousarray(c), **kw) for c in _channel(images, channel)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
GOLDEN_SHAPES = [((1, 1), 16), ((1, 40), 16), ((40, 1), 16), ((15, 33), 16), ((37, 53), 16), ((48, 49), 16), ((40, 70), 32),
                 ((130, 200), 64)]
GOLDEN_RULES = [(1280, None, 256, 1), (1536, 768, 256, 1), (1536, 768, 256, 2), (384, 64, 0, 1)]     # k8, weak8, floor8, connectivity


def noise_field(shape, dtype, seed=0) -> np.ndarray:
    """One 2-D image: a sloped background under Gaussian noise with blocks of several brightnesses and sizes on it."""
    H, W = shape
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    f = top * 0.12 + rng.normal(0.0, top * 0.012, shape) + top * 0.001 * (xx + 2 * yy)
    for _ in range(max(1, H * W // 250)):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        f[y:y + int(rng.integers(1, 7)), x:x + int(rng.integers(1, 7))] += top * rng.uniform(0.02, 0.6)
    return np.clip(np.rint(f), 0, top).astype(dtype)


def golden_inputs():
    """[(image, tile)] of tests/golden/golden_noise.npz, both pixel types of every shape."""
    return [(noise_field(shape, dtype), T) for shape, T in GOLDEN_SHAPES for dtype in (np.uint8, np.uint16)]
