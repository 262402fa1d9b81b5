"""The rule of cs_label_propagate (include/cellscreen.h) restated on the CPU, all integers.

Per image: a seed pixel (seeds > 0, labels 1..MAX_LABEL) is a source of cost 0; it keeps its label whatever the mask says, is never
relabelled and is never entered by a path.  A path starts at a seed pixel and then moves only through open pixels (no seed, mask
non-zero) to 4- or 8-neighbours inside the image.  A step q -> p costs lam * w + |g(p) - g(q)|: w = 1 on 4-neighbours ("cityblock"),
1 on 8-neighbours ("chessboard"), 5 axial and 7 diagonal on 8-neighbours ("chamfer"); g is the guide's channel, 0 without a guide.
A candidate whose cost exceeds max_cost is not taken.  A pixel's key is the lexicographic minimum over all such paths of (cost,
label of the path's seed); a pixel that no path reaches keeps label 0 and cost -1.

propagate_one is the restatement: Dijkstra's algorithm on the tuples (cost, label).  Every step costs at least lam >= 1, so a tuple
popped from the heap is final.  relax_sync is a second form that shares nothing with it but STEPS: the whole plane relaxed
synchronously on the packed keys (cost << 24) | label until nothing changes, the least fixed point of
K(p) = min(K(p), min over q of K(q) + step(q, p)).  Costs only grow along a path, so the rule with max_cost equals the rule without,
cut at max_cost afterwards (cut); the GPU tests compute one plane per content and cut it."""
import heapq
import math
from fractions import Fraction

import numpy as np

MAX_LABEL = 1 << 20
NO_LIMIT = (1 << 40) - 2
LABEL_BITS = 24
NONE = np.uint64((1 << 64) - 1)
UNREACHED = -1
WEIGHTS = {"cityblock": (1, 0), "chessboard": (1, 1), "chamfer": (5, 7)}   # axial, diagonal (0: no diagonal steps)
METRICS = tuple(WEIGHTS)


def steps_of(metric, lam):
    """[(dy, dx, lam * w)] of the metric's neighbourhood."""
    a, d = WEIGHTS[metric]
    out = [(0, -1, lam * a), (0, 1, lam * a), (-1, 0, lam * a), (1, 0, lam * a)]
    if d:
        out += [(-1, -1, lam * d), (-1, 1, lam * d), (1, -1, lam * d), (1, 1, lam * d)]
    return out


def max_cost_of(distance, metric="chamfer", lam=1):
    """floor(distance * lam * a), a the metric's axial weight, exactly of the number given."""
    exact = Fraction(int(distance)) if isinstance(distance, (int, np.integer)) else Fraction(float(distance))
    return math.floor(exact * lam * WEIGHTS[metric][0])


def check_seeds(seeds):
    if seeds.dtype != np.int32:
        raise TypeError("seeds must be int32")
    if (seeds < 0).any() or (seeds > MAX_LABEL).any():
        raise ValueError("a seed is negative or exceeds MAX_LABEL")


def propagate_one(seeds, mask=None, guide=None, metric="chamfer", lam=1, max_cost=NO_LIMIT):
    """seeds int32 [H,W], mask None or [H,W] (non-zero = open), guide None or an integer plane [H,W].  Returns (labels int32,
    cost int64)."""
    check_seeds(seeds)
    assert metric in WEIGHTS and 1 <= lam <= 255 and 1 <= max_cost <= NO_LIMIT
    H, W = seeds.shape
    steps = steps_of(metric, lam)
    is_seed = (seeds > 0).tolist()
    opened = ((seeds == 0) & (np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0)).tolist()
    g = (np.zeros((H, W), np.int64) if guide is None else np.asarray(guide).astype(np.int64)).tolist()
    lab = seeds.astype(np.int64).tolist()
    cost = np.where(seeds > 0, 0, UNREACHED).astype(np.int64).tolist()
    final = [[False] * W for _ in range(H)]
    heap = [(0, lab[y][x], y, x) for y in range(H) for x in range(W) if is_seed[y][x]]
    heapq.heapify(heap)
    while heap:
        c, l, y, x = heapq.heappop(heap)
        if not is_seed[y][x]:
            if final[y][x] or (c, l) != (cost[y][x], lab[y][x]):
                continue                                # an entry that a better one has overtaken
            final[y][x] = True
        gq = g[y][x]
        for dy, dx, w in steps:
            yy, xx = y + dy, x + dx
            if not (0 <= yy < H and 0 <= xx < W) or not opened[yy][xx] or final[yy][xx]:
                continue
            cc = c + w + abs(g[yy][xx] - gq)
            if cc > max_cost:
                continue
            if cost[yy][xx] == UNREACHED or (cc, l) < (cost[yy][xx], lab[yy][xx]):
                cost[yy][xx], lab[yy][xx] = cc, l
                heapq.heappush(heap, (cc, l, yy, xx))
    return np.array(lab, np.int32).reshape(H, W), np.array(cost, np.int64).reshape(H, W)


def guide_plane(guide, guide_channel=0):
    """[B,H,W] of a guide [B,H,W] or [B,H,W,C], or None."""
    if guide is None:
        return None
    return guide if guide.ndim == 3 else guide[..., guide_channel]


def propagate(seeds, mask=None, guide=None, guide_channel=0, metric="chamfer", lam=1, max_cost=None):
    """The batch form, image by image: seeds int32 [B,H,W], mask None or [B,H,W], guide None or [B,H,W] / [B,H,W,C]; max_cost None: no
    limit.  Returns (labels int32 [B,H,W], cost int64 [B,H,W])."""
    gp = guide_plane(guide, guide_channel)
    got = [propagate_one(seeds[b], None if mask is None else mask[b], None if gp is None else gp[b], metric, lam,
                         NO_LIMIT if max_cost is None else max_cost) for b in range(seeds.shape[0])]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def cut(labels, cost, max_cost):
    """What the rule gives with max_cost, from what it gives without: costs only grow along a path."""
    far = cost > max_cost
    return np.where(far, 0, labels).astype(np.int32), np.where(far, UNREACHED, cost).astype(np.int64)


def relax_sync(seeds, mask=None, guide=None, metric="chamfer", lam=1, max_cost=NO_LIMIT):
    """The second form, one image: every pixel of the plane relaxed at once from the keys of the sweep before, on the packed keys,
    until a sweep changes nothing.  Returns (labels int32, cost int64, sweeps)."""
    check_seeds(seeds)
    H, W = seeds.shape
    opened = (seeds == 0) & (np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0)
    g = np.zeros((H, W), np.int64) if guide is None else np.asarray(guide).astype(np.int64)
    K = np.where(seeds > 0, seeds.astype(np.uint64), NONE)
    low = np.uint64((1 << LABEL_BITS) - 1)
    sweeps = 0
    while True:
        sweeps += 1
        Kp = np.pad(K, 1, constant_values=NONE)
        gp = np.pad(g, 1)
        new = K.copy()
        for dy, dx, w in steps_of(metric, lam):
            Kq = Kp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            c = (Kq >> np.uint64(LABEL_BITS)).astype(np.int64) + w + np.abs(g - gp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
            ok = opened & (Kq != NONE) & (c <= max_cost)
            cand = (np.where(ok, c, 0).astype(np.uint64) << np.uint64(LABEL_BITS)) | (Kq & low)
            new = np.where(ok & (cand < new), cand, new)
        if np.array_equal(new, K):
            break
        K = new
    none = K == NONE
    return (np.where(none, 0, K & low).astype(np.int32), np.where(none, UNREACHED, (K >> np.uint64(LABEL_BITS)).astype(np.int64)), sweeps)


# ---- contents ----------------------------------------------------------------------------------------------------------------------
def field(shape, seed, cells=None, channels=1, dtype=np.uint16):
    """One field: (seeds int32 [H,W], mask uint8 [H,W], guide dtype [H,W,channels]).  Cell bodies are disks of radius 8..15 in the mask,
    the nuclei disks of radius 2..4 off their centres, labels in a shuffled order; the guide is a Gaussian bump per cell plus noise
    (in every channel another draw).  A later body may cover an earlier nucleus: seeds win."""
    H, W = shape
    rng = np.random.default_rng(seed)
    n = max(1, H * W // 900) if cells is None else cells
    yy, xx = np.mgrid[0:H, 0:W]
    seeds = np.zeros(shape, np.int32)
    mask = np.zeros(shape, np.uint8)
    top = 255.0 if dtype == np.uint8 else 4000.0
    f = np.zeros((channels, H, W))
    for lab in rng.permutation(n) + 1:
        cy, cx, R, r = rng.integers(0, H), rng.integers(0, W), rng.integers(8, 16), rng.integers(2, 5)
        oy, ox = rng.integers(-4, 5, 2)
        mask[(yy - cy) ** 2 + (xx - cx) ** 2 <= R * R] = 1
        spot = (yy - cy - oy) ** 2 + (xx - cx - ox) ** 2 <= r * r
        if not spot.any():
            spot = (yy == min(max(cy, 0), H - 1)) & (xx == min(max(cx, 0), W - 1))
        seeds[spot] = lab
        for ch in range(channels):
            f[ch] += 0.6 * top * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.6 * R) ** 2))
    f += rng.normal(0.0, top / 60.0, f.shape) + top / 20.0
    guide = np.clip(np.rint(f), 0, 255 if dtype == np.uint8 else 65535).astype(dtype)
    return seeds, mask, np.ascontiguousarray(guide.transpose(1, 2, 0))


def serpentine(H=48, W=192):
    """(seeds, mask) of a one-pixel-wide corridor that runs along every other row and turns at alternating ends, one seed at its
    mouth (0, 0)."""
    mask = np.zeros((H, W), np.uint8)
    mask[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        mask[y, W - 1 if k % 2 == 0 else 0] = 1
    seeds = np.zeros((H, W), np.int32)
    seeds[0, 0] = 1
    return seeds, mask
