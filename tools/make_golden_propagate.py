"""Writes tests/golden/golden_propagate.npz: small fields with what scipy.sparse.csgraph.dijkstra says of them, for
tests/test_propagate_cpu.py to hold the restatement of tests/propagate_reference.py to.  The expected planes are derived without
the restatement's code: per label l one Dijkstra run from that label's seed pixels over the graph of the rule's steps (edges lead
into open pixels only, so none enters a seed), D_l; the expected cost is min over l of D_l and the expected label the smallest l that
attains it; max_cost is applied afterwards.  lam >= 1 keeps every edge weight positive, so the sparse graph holds no zero entry.

Made with numpy 2.2.6 and SciPy 1.15.3.  Usage: python tools/make_golden_propagate.py"""
import os
import sys

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import propagate_reference as PR  # noqa: E402  (the contents and the table of weights only)

# name, shape, content seed, metric, guide, lam, max_cost (0: none), extra
CASES = [("chamfer_plain", (70, 300), 1, "chamfer", False, 1, 0, ""),
         ("chamfer_guide", (70, 300), 2, "chamfer", True, 8, 0, ""),
         ("chamfer_guide_lam1_capped", (33, 129), 3, "chamfer", True, 1, 600, ""),
         ("cityblock_plain_capped", (33, 129), 4, "cityblock", False, 1, 6, ""),
         ("cityblock_guide", (70, 300), 5, "cityblock", True, 8, 0, ""),
         ("chessboard_plain", (17, 65), 6, "chessboard", False, 8, 0, ""),
         ("chessboard_guide", (33, 129), 7, "chessboard", True, 1, 0, ""),
         ("seed_outside_its_mask", (33, 129), 8, "chamfer", True, 8, 0, "outside"),
         ("pocket_no_seed_reaches", (33, 129), 9, "cityblock", False, 1, 0, "pocket")]


def contents(shape, seed, extra):
    H, W = shape
    seeds, mask, guide = PR.field(shape, seed, cells=max(3, H * W // 900))
    if extra == "outside":                              # a seed on closed ground next to a body, and one far from any
        ys, xs = np.nonzero((mask == 0) & (seeds == 0))
        k = len(ys) // 2
        seeds[ys[k], xs[k]] = seeds.max() + 1
        mask[seeds == 1] = 0                            # and a whole nucleus whose own pixels the mask leaves out
    if extra == "pocket":
        mask[:, W // 2 - 1:W // 2 + 2] = 0              # a wall
        seeds[:, W // 2 + 2:] = 0                       # nothing right of it: its bodies are pockets
        assert mask[:, W // 2 + 2:].any() and seeds.any()
    return seeds, mask, guide[..., 0]


def graph_of(seeds, mask, guide, metric, lam):
    """The rule's steps as a sparse directed graph over the pixels (row = from, column = to), and the pixels' indices [H,W]."""
    H, W = seeds.shape
    opened = (seeds == 0) & (mask != 0)
    source_ok = opened | (seeds > 0)
    idx = np.arange(H * W).reshape(H, W)
    g = guide.astype(np.int64) if guide is not None else np.zeros((H, W), np.int64)
    a, d = PR.WEIGHTS[metric]
    moves = [(0, 1, a), (0, -1, a), (1, 0, a), (-1, 0, a)] + ([(1, 1, d), (1, -1, d), (-1, 1, d), (-1, -1, d)] if d else [])
    rows, cols, vals = [], [], []
    for dy, dx, w in moves:
        q = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))          # from
        p = (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))          # to
        ok = source_ok[q] & opened[p]
        rows.append(idx[q][ok])
        cols.append(idx[p][ok])
        vals.append((lam * w + np.abs(g[p] - g[q]))[ok])
    graph = coo_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()
    assert graph.data.min() >= 1.0
    return graph, idx


def scipy_planes(seeds, mask, guide, metric, lam):
    """(cost int64 with -1, labels int32) from one csgraph.dijkstra run per label."""
    H, W = seeds.shape
    graph, idx = graph_of(seeds, mask, guide, metric, lam)
    best = np.full(H * W, np.inf)
    who = np.zeros(H * W, np.int32)
    for l in np.unique(seeds[seeds > 0]):               # ascending: an equal distance keeps the smaller label
        D = dijkstra(graph, directed=True, indices=idx[seeds == l], min_only=True)
        take = D < best
        best[take], who[take] = D[take], l
    cost = np.where(np.isinf(best), -1, best).astype(np.int64).reshape(H, W)
    assert np.array_equal(cost >= 0, who.reshape(H, W) > 0) and (cost[seeds > 0] == 0).all()
    return cost, who.reshape(H, W)


def main():
    out = {"n_cases": np.int64(len(CASES))}
    for i, (name, shape, seed, metric, with_guide, lam, max_cost, extra) in enumerate(CASES):
        seeds, mask, guide = contents(shape, seed, extra)
        cost, labels = scipy_planes(seeds, mask, guide if with_guide else None, metric, lam)
        if max_cost:
            far = cost > max_cost
            cost, labels = np.where(far, -1, cost), np.where(far, 0, labels).astype(np.int32)
        grown = int(((labels > 0) & (seeds == 0)).sum())
        print(f"{name}: {shape}, {int((seeds > 0).sum())} seed px of {len(np.unique(seeds)) - 1} labels, {grown} grown, "
              f"{int(((mask != 0) & (labels == 0)).sum())} open px unreached, max cost {int(cost.max())}")
        assert grown > 100
        out.update({f"name_{i}": np.array(name), f"seeds_{i}": seeds, f"mask_{i}": mask, f"metric_{i}": np.array(metric),
                    f"lam_{i}": np.int64(lam), f"max_cost_{i}": np.int64(max_cost), f"cost_{i}": cost, f"labels_{i}": labels.astype(np.int32)})
        if with_guide:
            out[f"guide_{i}"] = guide
    path = os.path.join(ROOT, "tests", "golden", "golden_propagate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
