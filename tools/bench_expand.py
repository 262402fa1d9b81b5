"""Throughput of the label expansion (cs_label_expand, cellscreen/expand.py, csrc/expand.hip) and writes
profiles/expand_bench.json.  The workload: --images fields of 2048 x 2048 with 640 cells each (synth.label_images), images and
painted labels resident on the device.  One image's d2 plane is compared with scipy.ndimage.distance_transform_edt first (d2 has
no ties), and its labels with tests/expand_reference.py's rule on a 160 x 160 corner.  Then, per distance (4, 16 and 64 px):

  expand_images_per_s                   LabelExpander.expand_batch on the painted labels, in place on a copy (one library call,
                                        wall clock), median of --reps
  expand_columns_ms, expand_rows_ms     HIP-event times of the two passes per image: median and [min, max] over the repetitions
  segment_images_per_s                  ThresholdSegmenter.segment_batch of the same run without the expansion
  segment_expand_images_per_s           ... with expand_distance: the labels grown in place behind the segmenter
  host_edt_ms_per_image                 scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True) on --host-images
                                        of the same fields: the transform alone, without the gather that expand_labels adds
No time is a pass condition.

Usage: python tools/bench_expand.py [--images 8] [--side 2048] [--cells 640] [--reps 10] [--warmup 2] [--host-images 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cell-image-analysis_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DISTANCES = (4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-images", type=int, default=2)
    a = ap.parse_args()

    import torch
    from scipy.ndimage import distance_transform_edt

    import expand_reference as ER
    from build import source_hash
    from cellscreen import expand as EX
    from cellscreen import segment as S
    from cellscreen import synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_expand needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    span = lambda v: [float(np.min(v)), float(np.max(v))]
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    tl = torch.from_numpy(labs).to(dev)
    work = torch.empty_like(tl)
    torch.cuda.synchronize()
    exp = EX.LabelExpander(0)

    # the outputs first: d2 against SciPy on one whole field, labels against the restatement on a corner
    g, d2 = exp.expand_batch(tl[:1].contiguous(), 16, return_d2=True)
    edt = distance_transform_edt(labs[0] == 0)
    sq = np.rint(edt * edt).astype(np.int64)
    want_d2 = np.where(labs[0] > 0, 0, np.where(edt <= 16, sq, 65535)).astype(np.uint16)
    got_d2 = d2[0].view(torch.int16).cpu().numpy().view(np.uint16)
    if not np.array_equal(got_d2, want_d2):
        raise SystemExit("d2 differs from scipy.ndimage.distance_transform_edt")
    corner = np.ascontiguousarray(labs[:1, :160, :160])
    if not np.array_equal(exp.expand_batch(corner, 16), ER.expand(corner, 256)[0]):
        raise SystemExit("labels differ from tests/expand_reference.py")
    grown_px = int(((g[0] > 0) & (tl[0] == 0)).sum())

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

    res = {"tool": "bench_expand", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells, "reps": a.reps,
           "warmup": a.warmup, "labelled_fraction": float((labs > 0).mean()), "grown_pixels_image0_distance16": grown_px,
           "checked": "d2 of one field equals scipy's transform; labels of a 160 x 160 corner equal the restatement", "distances": []}
    plain = S.ThresholdSegmenter(0)
    plain_walls, plain_stages = timed(lambda: plain.segment_batch(ti), plain.last_timing)
    res["segment_images_per_s"] = a.images / med(plain_walls)
    res["segment_ms_per_image"] = 1e3 * med(plain_walls) / a.images
    for distance in DISTANCES:
        def alone():
            work.copy_(tl)
            exp.expand_batch(work, distance, out=work)

        copy_walls, _ = timed(lambda: work.copy_(tl), dict)
        walls, stages = timed(alone, exp.last_timing)
        seg = S.ThresholdSegmenter(0, expand_distance=distance)
        seg_walls, seg_stages = timed(lambda: seg.segment_batch(ti), seg.last_timing)
        net = med(walls) - med(copy_walls)                              # the call without the copy that restores its input
        e = {"distance": distance, "max_d2": int(EX.expand_params(distance).max_d2),
             "expand_images_per_s": a.images / net, "expand_ms_per_image": 1e3 * net / a.images,
             "segment_expand_images_per_s": a.images / med(seg_walls), "segment_expand_ms_per_image": 1e3 * med(seg_walls) / a.images}
        for key in ("expand_columns_ms", "expand_rows_ms"):
            v = [s[key] / a.images for s in stages]
            e[key + "_per_image"] = med(v)
            e[key + "_per_image_range"] = span(v)
            e["segment_" + key + "_per_image"] = med([s[key] / a.images for s in seg_stages])
        res["distances"].append(e)
        seg.close()
    host = []
    for b in range(min(a.host_images, a.images)):
        t0 = time.perf_counter()
        distance_transform_edt(labs[b] == 0, return_indices=True)
        host.append(time.perf_counter() - t0)
    res["host_images"] = len(host)
    res["host_edt_ms_per_image"] = 1e3 * med(host)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "expand_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
