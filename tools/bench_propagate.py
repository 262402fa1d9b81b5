"""Throughput of the geodesic label growth (cs_label_propagate, cellscreen/propagate.py, csrc/propagate.hip) and writes
profiles/propagate_bench.json.  The workload is the other label tools': --images fields of 2048 x 2048 uint16 with 640 cells each
(synth.label_images).  The painted cells are the mask; the seeds are the cells shrunk by --shrink pixels inside their own label
(the nuclei); the guide is the fields' channel 1.  All planes are resident on the device.  Per metric (cityblock, chessboard,
chamfer), with and without the guide, with a limit (the max_cost that `distance` 16 stands for) and without one:

  ms_per_image                          LabelPropagator.propagate_batch with return_cost (one library call, wall clock), median of --reps
  rounds                                the relaxation rounds of a call, the closing quiet one included
  init_ms, relax_ms, finish_ms          HIP-event times of the three passes per image, medians
and in the same run
  expand_ms_per_image                   LabelExpander.expand_batch of the same seeds at 16 px, and ratio_to_expand of every case above
  host_dijkstra_ms                      scipy.sparse.csgraph.dijkstra(min_only=True) from all seed pixels of one field (chamfer, no guide,
                                        no limit) on the host, the graph's construction apart; its cost plane must equal the device's
Before any time is taken one field's labels and costs are compared with tests/propagate_reference.py on a 200 x 200 corner.

The parent process never opens the GPU: every group of timed launches (one per metric, one for the expansion) is a child process
of its own under --limit seconds, and the first child that fails or runs out of time ends the run without a result file.  No time is
a pass condition.

Usage: python tools/bench_propagate.py [--images 8] [--side 2048] [--cells 640] [--shrink 6] [--reps 10] [--warmup 2] [--limit 240]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cell-image-analysis_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

METRICS = ("cityblock", "chessboard", "chamfer")
DISTANCE, LAM, GUIDE_LAM, GUIDE_CHANNEL = 16, 1, 4, 1


def shrink(labs, k):
    """The labels less every pixel within k 4-steps of another label or of the background."""
    keep = labs > 0
    for _ in range(k):
        p = np.pad(np.where(keep, labs, 0), ((0, 0), (1, 1), (1, 1)))
        c = p[:, 1:-1, 1:-1]
        keep = (c > 0) & (p[:, :-2, 1:-1] == c) & (p[:, 2:, 1:-1] == c) & (p[:, 1:-1, :-2] == c) & (p[:, 1:-1, 2:] == c)
    return np.where(keep, labs, 0).astype(np.int32)


def workload(a):
    from cellscreen import synth
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    return imgs, shrink(labs, a.shrink), (labs > 0).astype(np.uint8)


def child(a):
    """One group of timed launches on the device; prints one JSON line."""
    import torch

    import propagate_reference as PR
    from cellscreen import expand as EX
    from cellscreen import propagate as PG

    if not torch.cuda.is_available():
        raise SystemExit("bench_propagate needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    z = np.load(a.planes)
    imgs, seeds, mask = z["imgs"], z["seeds"], z["mask"]
    n = seeds.shape[0]
    ti, ts, tm = torch.from_numpy(imgs.view(np.int16)).to(dev), torch.from_numpy(seeds).to(dev), torch.from_numpy(mask).to(dev)
    out = torch.empty_like(ts)
    torch.cuda.synchronize()
    med = lambda v: float(np.median(v))

    def timed(fn, timing):
        walls, stages = [], []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stages.append(timing())
        return walls, stages

    if a.child == "expand":
        exp = EX.LabelExpander(0)
        walls, _ = timed(lambda: exp.expand_batch(ts, DISTANCE, out=out), exp.last_timing)
        print(json.dumps({"expand_ms_per_image": 1e3 * med(walls) / n, "expand_distance": DISTANCE}))
        return
    metric = a.child
    tool = PG.LabelPropagator(0)
    c = 200                                             # the outputs first: a corner against the restatement
    cs, cm, cg = (np.ascontiguousarray(x[:1, :c, :c]) for x in (seeds, mask, imgs))
    for guide, lam in ((None, LAM), (cg, GUIDE_LAM)):
        got = tool.propagate_batch(cs, mask=cm, guide=guide, guide_channel=GUIDE_CHANNEL if guide is not None else 0, metric=metric, lam=lam,
                                   return_cost=True)
        want = PR.propagate(cs, cm, guide, GUIDE_CHANNEL, metric, lam)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            raise SystemExit(f"{metric}: labels or costs differ from tests/propagate_reference.py")
    cases = []
    for with_guide in (False, True):
        lam = GUIDE_LAM if with_guide else LAM
        for limit in (PG.max_cost_of(DISTANCE, metric, lam), None):
            kw = dict(mask=tm, guide=ti if with_guide else None, guide_channel=GUIDE_CHANNEL if with_guide else 0, metric=metric, lam=lam,
                      max_cost=limit, return_cost=True, out=out)
            walls, stages = timed(lambda: tool.propagate_batch(ts, **kw), tool.last_timing)
            grown = int(((out > 0) & (ts == 0)).sum())
            e = {"metric": metric, "guide": with_guide, "lam": lam, "max_cost": limit, "ms_per_image": 1e3 * med(walls) / n,
                 "ms_per_image_range": [1e3 * min(walls) / n, 1e3 * max(walls) / n], "rounds": med([s["propagate_rounds"] for s in stages]),
                 "grown_pixels_per_image": grown / n}
            for key in ("propagate_init_ms", "propagate_relax_ms", "propagate_finish_ms"):
                e[key[10:] + "_per_image"] = med([s[key] / n for s in stages])
            cases.append(e)
    res = {"cases": cases}
    if metric == "chamfer":                             # one field's cost plane for the host's Dijkstra to be held to
        cost = tool.propagate_batch(ts[:1].contiguous(), mask=tm[:1].contiguous(), metric=metric, lam=LAM, return_cost=True)[1]
        np.save(a.planes + ".cost.npy", cost.cpu().numpy())
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=640)
    ap.add_argument("--shrink", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--planes", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    from scipy.sparse.csgraph import dijkstra

    from build import source_hash
    from make_golden_propagate import graph_of

    imgs, seeds, mask = workload(a)
    res = {"tool": "bench_propagate", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells, "shrink": a.shrink,
           "reps": a.reps, "warmup": a.warmup, "seed_fraction": float((seeds > 0).mean()), "mask_fraction": float(mask.mean()),
           "distance": DISTANCE, "lam": LAM, "guide_lam": GUIDE_LAM, "guide_channel": GUIDE_CHANNEL,
           "checked": "labels and costs of a 200 x 200 corner equal the restatement, per metric, with and without the guide; "
                      "the cost plane of one field equals scipy's Dijkstra", "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        planes = os.path.join(tmp, "planes.npz")
        np.savez(planes, imgs=imgs, seeds=seeds, mask=mask)
        for group in ("expand",) + METRICS:             # chained: the first failure ends the run
            cmd = [sys.executable, os.path.abspath(__file__), "--child", group, "--planes", planes, "--reps", str(a.reps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{group}: no result within {a.limit} s; nothing more is started")
            if r.returncode != 0:
                raise SystemExit(f"{group}: exit status {r.returncode}; nothing more is started\n{r.stdout}{r.stderr}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            res["cases"] += got.pop("cases", [])
            res.update(got)
            print(group, "done", file=sys.stderr)
        device_cost = np.load(planes + ".cost.npy")[0]
    for e in res["cases"]:
        e["ratio_to_expand"] = e["ms_per_image"] / res["expand_ms_per_image"]
    t0 = time.perf_counter()
    graph, idx = graph_of(seeds[0], mask[0], None, "chamfer", LAM)
    t1 = time.perf_counter()
    D = dijkstra(graph, directed=True, indices=idx[seeds[0] > 0], min_only=True)
    t2 = time.perf_counter()
    host_cost = np.where(np.isinf(D), -1, D).astype(np.int64).reshape(seeds[0].shape)
    if not np.array_equal(host_cost, device_cost):
        raise SystemExit("the device's cost plane differs from scipy.sparse.csgraph.dijkstra")
    res["host_graph_ms"], res["host_dijkstra_ms"] = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "propagate_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
