"""Throughput of the per-object shape records (cs_label_shape, cellscreen/shape.py, csrc/shape.hip) and writes
profiles/shape_bench.json.  The workload is tools/bench_texture.py's: --images fields of 2048 x 2048 with 640 cells each
(synth.label_images), resident on the device; the objects are the painted labels grown by 6 px (LabelExpander).  One field's records
are compared with tests/shape_reference.py first.  Then, with and without the hull:

  moments_ms_per_image, outline_ms_per_image
                                         HIP-event times of the two spans (clearing + moments and bounding boxes; the quads, the
                                         perimeter classes and the hull): median and [min, max] over the repetitions
  device_ms_per_image                    their sum
  call_ms_per_image                      ShapeMeasurer.measure_dense, wall clock: the spans, the records to the host
  ratio_to_intensity_pass                device_ms / cs_label_intensity's pass (one uint16 channel, same fields, same run)
  ratio_to_texture_matrices              outline_ms / cs_label_texture's matrices at 8 levels, d = 1 (same fields, same run)
  host_reference_ms_per_image            tests/shape_reference.measure, the numpy restatement, on --host-images of the same fields
  host_table_ms_per_image                cellscreen.shape.shape_table on the device's records: the derivation in Python ints
No time is a pass condition.

Usage: python tools/bench_shape.py [--images 8] [--side 2048] [--cells 640] [--reps 10] [--warmup 2] [--host-images 1]"""
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

GROW = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-images", type=int, default=1)
    a = ap.parse_args()

    import torch

    import shape_reference as SR
    from build import source_hash
    from cellscreen import expand as EX
    from cellscreen import intensity as IN
    from cellscreen import shape as SH
    from cellscreen import synth
    from cellscreen import texture as TX

    if not torch.cuda.is_available():
        raise SystemExit("bench_shape needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    span = lambda v: [float(np.min(v)), float(np.max(v))]
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    tl = torch.from_numpy(labs).to(dev)
    grown = EX.LabelExpander(0).expand_batch(tl, GROW)
    h_grown = grown.cpu().numpy()
    max_label = int(labs.max())
    meas, inten, tex = SH.ShapeMeasurer(0), IN.IntensityMeasurer(0), TX.TextureMeasurer(0)
    t_img = torch.from_numpy(np.ascontiguousarray(imgs[..., 1:2]).view(np.int16)).to(dev)

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

    res = {"tool": "bench_shape", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells, "reps": a.reps,
           "warmup": a.warmup, "grown_by": GROW, "max_label": max_label, "labelled_fraction": float((h_grown > 0).mean()),
           "objects_per_image": float(np.mean([len(np.unique(x)) - 1 for x in h_grown])),
           "checked": "the records of one field equal tests/shape_reference.py with and without the hull", "configs": []}
    _, i_stages = timed(lambda: inten.measure_dense(t_img, grown, max_label=max_label), inten.last_timing)
    ipass = [s["intensity_pass_ms"] / a.images for s in i_stages]
    _, t_stages = timed(lambda: tex.measure_dense(t_img, grown, 1, 8, max_label=max_label), tex.last_timing)
    tmat = [s["texture_matrices_ms"] / a.images for s in t_stages]
    host = []
    for b in range(min(a.host_images, a.images)):
        t0 = time.perf_counter()
        want = SR.measure(h_grown[b:b + 1], max_label=max_label)
        host.append(time.perf_counter() - t0)
        if b == 0:
            for hull in (True, False):
                got = meas.measure_dense(grown[:1].contiguous(), max_label=max_label, hull=hull)
                if not all(np.array_equal(g, w) for g, w in zip(got, want) if g is not None):
                    raise SystemExit(f"the records differ from tests/shape_reference.py (hull={hull})")
    for hull in (True, False):
        walls, stages = timed(lambda: meas.measure_dense(grown, max_label=max_label, hull=hull), meas.last_timing)
        per = {k: [s[f"shape_{k}_ms"] / a.images for s in stages] for k in ("moments", "outline")}
        total = [sum(x) for x in zip(*per.values())]
        rec = meas.measure_dense(grown, max_label=max_label, hull=hull)
        t0 = time.perf_counter()
        table = SH.shape_table(*rec)
        t_table = time.perf_counter() - t0
        cfg = {"hull": hull, "objects": len(table)}
        for k, v in per.items():
            cfg[f"{k}_ms_per_image"] = med(v)
            cfg[f"{k}_ms_per_image_range"] = span(v)
        cfg.update({"device_ms_per_image": med(total), "call_ms_per_image": 1e3 * med(walls) / a.images,
                    "intensity_pass_ms_per_image": med(ipass), "ratio_to_intensity_pass": med(total) / med(ipass),
                    "texture_matrices_ms_per_image": med(tmat), "ratio_to_texture_matrices": med(per["outline"]) / med(tmat),
                    "host_images": len(host), "host_reference_ms_per_image": 1e3 * med(host),
                    "host_table_ms_per_image": 1e3 * t_table / a.images})
        res["configs"].append(cfg)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "shape_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
