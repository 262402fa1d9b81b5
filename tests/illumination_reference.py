"""CPU restatement of the flat-field correction (cs_illum_tile_stats, cs_illum_reduce, cs_illum_apply in csrc/illumination.hip,
cellscreen.IlluminationCorrector): what the device kernels are compared against, with numpy sorts and int64
arithmetic only.  The rule: all integers, no tolerance anywhere, bit-identical run to run.

Images are [B][H][W][C] or [B][H][W], C in 1..4, uint8 or uint16, sides 1..4096, batch 1..65535.  The mesh is DESIGN 3r's
(noise_reference.axis_tiles): tile side T a power of two in 16..256, m = max(1, n // T) tiles per axis, the last one runs to n.

  tile_stats     1. per image, channel and tile the value of rank (q_num (N - 1)) // q_den among the tile's N sorted pixels,
                 0 <= q_num <= q_den <= 65536 (1 / 2: the lower median, 0: the minimum); int32 [B,C,my,mx]
  across         2. per channel and node over the n stacked meshes (1 <= n <= 16384) the value of rank (a_num (n - 1)) // a_den, or
                 with "mean" (2 sum + n) // (2 n); int64 [C,my,mx]
  reduce         ... then F8 = 256 max(value - offset_c, floor), offset 0..65535 per channel, floor 1..4095; then, both optional and
                 off by default, in this order: noise_reference.filter3 (the 3 x 3 mesh median, replicated edges) and smooth_mesh;
                 int32 [C,my,mx], 256 <= F8 < 2^24
  smooth_mesh    a Gaussian over the mesh with a smooth_reference.smooth_weights table (radius <= 64), the mesh reflected at its
                 edges (local_reference.fold), rows then columns in int64 (row sums < 2^40, full sums < 2^56), ONE rounding
                 (A + 2^31) >> 32 at the end, floored at 256 floor again
  scale          3. G8_c in Python ints: the rounded mean (2 sum + n) // (2 n), the lower median, the max or the min of F8_c, or the
                 caller's integer; 1 <= G8 < 2^24
  axis_weights   4. per pixel of one axis the two nodes, w0, w1 and D between the tile centres at the doubled coordinates
                 C2_i = start_i + end_i - 1: i with C2_i <= 2p < C2_{i+1}, clamped to the first or last pair; w1 = 2p - C2_i is NOT
                 clamped (negative left of the first centre, above D right of the last: linear extrapolation), w0 = D - w1; one
                 node: D = 1, w0 = 1, w1 = 0.  constant=True clamps w1 to 0..D: DESIGN 3r's constant continuation, kept here for
                 the comparison the defaults rest on
  maps           N = max(sum wy wx F8, 256 floor D) and D = Dy Dx per pixel, int64
  apply          5. y = clamp(pedestal_c + floor((2 (v - offset_c) G8_c D + N) / (2 N)), 0, top): Python's // on int64, which rounds
                 the quotient half up and floors a negative numerator; clipped int64 [B,C,2]: the pixels clamped at 0 and at top
|w| < 5 T, so |sum| < 2^47 and the numerator is below 2^62: everything fits int64.  tests/golden/golden_illumination.npz
(tools/make_golden_illumination.py) pins this file against drift, and tests/test_illumination_cpu.py holds it to a slow form in
exact rationals."""
import numpy as np

from local_reference import fold
from noise_reference import axis_tiles, filter3
from smooth_reference import check_table, smooth_weights  # noqa: F401

TILES = (16, 32, 64, 128, 256)
F8_MIN, F8_END = 256, 1 << 24


def _stack4(images):
    if images.dtype not in (np.uint8, np.uint16) or images.ndim not in (3, 4):
        raise TypeError("[B,H,W] or [B,H,W,C] uint8 / uint16 expected")
    x = images[..., None] if images.ndim == 3 else images
    if not 1 <= x.shape[3] <= 4:
        raise ValueError("1..4 channels")
    return x


def tile_stats(images: np.ndarray, T: int, q=(1, 2)) -> np.ndarray:
    x = _stack4(images)
    q_num, q_den = q
    if T not in TILES or not 0 <= q_num <= q_den <= 65536 or q_den < 1:
        raise ValueError("tile or quantile out of range")
    B, H, W, C = x.shape
    ty, tx = axis_tiles(H, T), axis_tiles(W, T)
    out = np.zeros((B, C, len(ty), len(tx)), np.int32)
    for j, (y0, y1) in enumerate(ty):
        for i, (x0, x1) in enumerate(tx):
            v = np.sort(x[:, y0:y1, x0:x1, :].reshape(B, -1, C), axis=1)
            out[:, :, j, i] = v[:, (q_num * (v.shape[1] - 1)) // q_den, :]
    return out


def across(stack: np.ndarray, rule=(1, 2)) -> np.ndarray:
    if stack.ndim != 4 or stack.dtype != np.int32 or not 1 <= stack.shape[0] <= 16384:
        raise TypeError("[n,C,my,mx] int32 expected, n in 1..16384")
    if stack.min() < 0 or stack.max() > 65535:
        raise ValueError("a value of the stack is outside 0..65535")
    s = stack.astype(np.int64)
    n = s.shape[0]
    if isinstance(rule, str):
        if rule != "mean":
            raise ValueError("across: (num, den) or 'mean'")
        return (2 * s.sum(axis=0) + n) // (2 * n)
    a_num, a_den = rule
    if not 0 <= a_num <= a_den <= 65536 or a_den < 1:
        raise ValueError("across out of range")
    return np.sort(s, axis=0)[(a_num * (n - 1)) // a_den]


def _pass(x: np.ndarray, w) -> np.ndarray:
    """sum_k w[|k|] x[:, fold(j + k)] along the last axis, int64."""
    r, n = len(w) - 1, x.shape[1]
    p = x[:, fold(np.arange(-r, n + r), n)]
    out = w[0] * x
    for k in range(1, r + 1):
        out = out + w[k] * (p[:, r - k:r - k + n] + p[:, r + k:r + k + n])
    return out


def smooth_mesh(F: np.ndarray, w, floor: int) -> np.ndarray:
    """One channel's mesh [my,mx] int64 under the table w."""
    w = check_table(w)
    t = _pass(F.astype(np.int64), w)
    assert int(t.max()) < 1 << 40
    a = _pass(np.ascontiguousarray(t.T), w).T
    assert int(a.max()) < 1 << 56
    return np.maximum((a + (1 << 31)) >> 32, F8_MIN * floor)


def _per_channel(v, C):
    return [int(v)] * C if np.isscalar(v) else [int(x) for x in v]


def reduce(stack: np.ndarray, rule=(1, 2), offset=0, floor: int = 1, mesh_median: bool = False, weights=None) -> np.ndarray:
    C = stack.shape[1]
    off = _per_channel(offset, C)
    if len(off) != C or min(off) < 0 or max(off) > 65535 or not 1 <= floor <= 4095:
        raise ValueError("offset or floor out of range")
    value = across(stack, rule)
    F = np.stack([256 * np.maximum(value[c] - off[c], floor) for c in range(C)])
    if mesh_median:
        F = np.stack([filter3(F[c]) for c in range(C)])
    if weights is not None:
        F = np.stack([smooth_mesh(F[c], weights, floor) for c in range(C)])
    assert F.min() >= F8_MIN and F.max() < F8_END
    return F.astype(np.int32)


def scale(F8: np.ndarray, normalize="mean"):
    out = []
    for c in range(F8.shape[0]):
        v = sorted(int(x) for x in F8[c].ravel())
        n = len(v)
        if normalize == "mean":
            g = (2 * sum(v) + n) // (2 * n)
        elif normalize == "median":
            g = v[(n - 1) // 2]
        elif normalize == "max":
            g = v[-1]
        elif normalize == "min":
            g = v[0]
        else:
            g = int(normalize)
        if not 1 <= g < F8_END:
            raise ValueError("G8 outside [1, 2^24)")
        out.append(g)
    return out


def axis_weights(n: int, T: int, constant: bool = False):
    """(i0, i1, w0, w1, D), int64 [n] each."""
    tiles = axis_tiles(n, T)
    z = np.zeros(n, np.int64)
    if len(tiles) == 1:
        return z, z, z + 1, z, z + 1
    c2 = np.array([s + e - 1 for s, e in tiles], np.int64)
    p2 = 2 * np.arange(n, dtype=np.int64)
    i0 = np.clip(np.searchsorted(c2, p2, side="right") - 1, 0, len(tiles) - 2)
    D = c2[i0 + 1] - c2[i0]
    w1 = p2 - c2[i0]
    if constant:
        w1 = np.clip(w1, 0, D)
    return i0, i0 + 1, D - w1, w1, D


def maps(F8c: np.ndarray, H: int, W: int, T: int, floor: int = 1, constant: bool = False):
    """(N, D) of every pixel of one channel, int64 [H,W]; F8c: [my,mx]."""
    a = F8c.astype(np.int64)
    if a.shape != (max(1, H // T), max(1, W // T)):
        raise ValueError("the mesh does not match (H, W, T)")
    if a.min() < F8_MIN or a.max() >= F8_END:
        raise ValueError("F8 outside [256, 2^24)")
    y0, y1, wy0, wy1, Dy = axis_weights(H, T, constant)
    x0, x1, wx0, wx1, Dx = axis_weights(W, T, constant)
    N = (wy0[:, None] * (wx0[None, :] * a[y0][:, x0] + wx1[None, :] * a[y0][:, x1]) +
         wy1[:, None] * (wx0[None, :] * a[y1][:, x0] + wx1[None, :] * a[y1][:, x1]))
    D = Dy[:, None] * Dx[None, :]
    assert int(np.abs(N).max()) < 1 << 47
    return np.maximum(N, F8_MIN * floor * D), D


def apply(images: np.ndarray, F8: np.ndarray, G8, T: int, offset=0, pedestal=None, floor: int = 1, constant: bool = False):
    """(corrected stack of the images' dtype and shape, clipped int64 [B,C,2])."""
    x = _stack4(images)
    B, H, W, C = x.shape
    off = _per_channel(offset, C)
    ped = off if pedestal is None else _per_channel(pedestal, C)
    G8 = [int(g) for g in G8]
    if F8.shape[0] != C or len(G8) != C or min(G8) < 1 or max(G8) >= F8_END or min(ped) < 0 or max(ped) > 65535:
        raise ValueError("F8, G8 or pedestal out of range")
    top = int(np.iinfo(x.dtype).max)
    out = np.empty_like(x)
    clipped = np.zeros((B, C, 2), np.int64)
    for c in range(C):
        N, D = maps(F8[c], H, W, T, floor, constant)
        num = 2 * (x[..., c].astype(np.int64) - off[c]) * G8[c] * D[None] + N[None]
        assert int(np.abs(num).max()) < 1 << 62
        y = ped[c] + num // (2 * N[None])
        clipped[:, c, 0] = (y < 0).sum(axis=(1, 2))
        clipped[:, c, 1] = (y > top).sum(axis=(1, 2))
        out[..., c] = np.clip(y, 0, top).astype(x.dtype)
    return out.reshape(images.shape), clipped


def correct(images: np.ndarray, T: int, q=(1, 2), rule=(1, 2), offset=0, floor: int = 1, mesh_median: bool = False, weights=None,
            normalize="mean", pedestal=None):
    """The whole chain on one stack: (corrected, clipped, F8, G8)."""
    F8 = reduce(tile_stats(images, T, q), rule, offset, floor, mesh_median, weights)
    G8 = scale(F8, normalize)
    out, clipped = apply(images, F8, G8, T, offset, pedestal, floor)
    return out, clipped, F8, G8


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def vignette(H: int, W: int, edge: float, centre=(0.45, 0.55)) -> np.ndarray:
    """The true function of plate(), float64 [H,W]: 1 at its (off-centre) peak, `edge` at the farthest corner, a paraboloid."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = centre[0] * (H - 1), centre[1] * (W - 1)
    r2 = (yy - cy) ** 2 + (xx - cx) ** 2
    return 1.0 - (1.0 - edge) * r2 / r2.max()


def plate(seed: int, n: int = 16, side: int = 256, cells: int = 8, edge: float = 0.5, dark: int = 100, sigma: float = 12.0,
          background: float = 2000.0, dtype=np.uint16):
    """(fields [n,side,side] of dtype, truth): n fields of `cells` bright discs at random places on a flat background, all under
    the vignette `truth`, on a dark level with Gaussian noise."""
    rng = np.random.default_rng(seed)
    truth = vignette(side, side, edge)
    yy, xx = np.mgrid[0:side, 0:side]
    out = np.empty((n, side, side), dtype)
    top = int(np.iinfo(dtype).max)
    for k in range(n):
        f = np.full((side, side), background)
        for _ in range(cells):
            cy, cx, r = rng.uniform(0, side), rng.uniform(0, side), rng.uniform(5.0, 9.0)
            f[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] += rng.uniform(3000.0, 12000.0)
        out[k] = np.clip(np.rint(dark + f * truth + rng.normal(0.0, sigma, (side, side))), 0, top).astype(dtype)
    return out, truth


GOLDEN_CASES = [  # shape [B,H,W(,C)], dtype, T, q, rule, offset, floor, mesh_median, sigma, normalize, pedestal
    ((3, 40, 40), np.uint16, 16, (1, 2), (1, 2), 0, 1, False, 0.0, "mean", None),
    ((4, 33, 49, 4), np.uint8, 16, (1, 4), "mean", [3, 0, 7, 1], 2, False, 0.0, "min", 0),
    ((5, 70, 40, 2), np.uint16, 32, (0, 1), (1, 1), 90, 5, True, 0.0, "median", [100, 0]),
    ((1, 130, 200, 3), np.uint16, 64, (65535, 65536), (0, 1), [0, 10, 20], 1, True, 1.0, "max", None),
    ((3, 15, 97), np.uint8, 16, (1, 2), (1, 2), 1, 1, False, 2.5, 40000, 5),
]


def golden_field(shape, dtype, seed=0) -> np.ndarray:
    """A stack under a vignette with blocks of several brightnesses on it."""
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(seed + 7 * int(np.prod(shape)))
    B, H, W = shape[:3]
    C = shape[3] if len(shape) == 4 else 1
    v = vignette(H, W, 0.45)[None, :, :, None]
    f = top * 0.2 * v + rng.normal(0.0, top * 0.01, (B, H, W, C))
    for _ in range(max(1, B * H * W // 300)):
        b, y, x = int(rng.integers(0, B)), int(rng.integers(0, H)), int(rng.integers(0, W))
        f[b, y:y + int(rng.integers(1, 7)), x:x + int(rng.integers(1, 7))] += top * rng.uniform(0.05, 0.9)
    return np.clip(np.rint(f), 0, top).astype(dtype).reshape(shape)


def golden_outputs():
    """[(corrected, clipped, F8, G8)] of GOLDEN_CASES."""
    out = []
    for shape, dtype, T, q, rule, offset, floor, med, sigma, normalize, pedestal in GOLDEN_CASES:
        w = smooth_weights(sigma) if sigma else None
        out.append(correct(golden_field(shape, dtype), T, q, rule, offset, floor, med, w, normalize, pedestal))
    return out
