"""Throughput of the per-object texture records (cs_label_texture, cellscreen/texture.py, csrc/texture.hip) and writes
profiles/texture_bench.json.  The workload is tools/bench_quantiles.py's: --images fields of 2048 x 2048 with 640 cells each
(synth.label_images), uint16, resident on the device; the objects are the painted labels grown by 6 px (LabelExpander).  One
field's records are compared with tests/texture_reference.py first.  Then, for 1 and 3 channels, 8 / 32 / 64 levels and the
distances 1 and 3:

  boxes_ms_per_image, matrices_ms_per_image
                                         HIP-event times of the two spans (clearing + counts and bounding boxes, the matrices with
                                         their reduction): median and [min, max] over the repetitions
  device_ms_per_image                    their sum
  call_ms_per_image                      TextureMeasurer.measure_dense, wall clock: the spans, the records to the host
  ratio_to_intensity_pass                device_ms / cs_label_intensity's pass (IntensityMeasurer, same fields and channels, same run)
  host_reference_ms_per_image            tests/texture_reference.measure, the numpy restatement (a shifted comparison of whole planes
                                         per direction, then np.add.at), on --host-images of the same fields
No time is a pass condition.

Usage: python tools/bench_texture.py [--images 8] [--side 2048] [--cells 640] [--reps 10] [--warmup 2] [--host-images 1]"""
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

CHANNELS = (1, 3)
LEVELS = (8, 32, 64)
DISTANCES = (1, 3)
GROW = 6
CLOGC_REL = 2.0 ** -40


def equal(got, want):
    """the records of the device against the restatement's: integers equal, clogc within 2^-40 of it"""
    return (all(np.array_equal(got[k], want[k]) for k in (0, 1, 2)) and bool((np.abs(got[3] - want[3]) <= CLOGC_REL * want[3]).all()))


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

    import texture_reference as TR
    from build import source_hash
    from cellscreen import expand as EX
    from cellscreen import intensity as IN
    from cellscreen import synth
    from cellscreen import texture as TX

    if not torch.cuda.is_available():
        raise SystemExit("bench_texture needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    span = lambda v: [float(np.min(v)), float(np.max(v))]
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    tl = torch.from_numpy(labs).to(dev)
    grown = EX.LabelExpander(0).expand_batch(tl, GROW)
    h_grown = grown.cpu().numpy()
    max_label = int(labs.max())
    meas = TX.TextureMeasurer(0)
    inten = IN.IntensityMeasurer(0)

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

    res = {"tool": "bench_texture", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells, "reps": a.reps,
           "warmup": a.warmup, "pixel_type": "uint16", "grown_by": GROW, "max_label": max_label,
           "labelled_fraction": float((h_grown > 0).mean()),
           "objects_per_image": float(np.mean([len(np.unique(x)) - 1 for x in h_grown])),
           "checked": "the records of one field equal tests/texture_reference.py in every configuration (clogc within 2^-40)", "configs": []}
    for nc in CHANNELS:
        h_img = np.ascontiguousarray(imgs[..., :nc] if nc > 1 else imgs[..., 1:2])
        t_img = torch.from_numpy(h_img.view(np.int16)).to(dev)
        ranges = TR.full_range(np.uint16, nc)
        _, i_stages = timed(lambda: inten.measure_dense(t_img, grown, max_label=max_label), inten.last_timing)
        ipass = [s["intensity_pass_ms"] / a.images for s in i_stages]
        for levels in LEVELS:
            for d in DISTANCES:
                got = meas.measure_dense(t_img[:1].contiguous(), grown[:1].contiguous(), d, levels, max_label=max_label)
                t0 = time.perf_counter()
                want = TR.measure(h_img[:1], h_grown[:1], d, levels, ranges, max_label=max_label)
                host = [time.perf_counter() - t0]
                if not equal(got, want):
                    raise SystemExit(f"the records differ from tests/texture_reference.py at {nc} channels, {levels} levels, distance {d}")
                for b in range(1, min(a.host_images, a.images)):
                    t0 = time.perf_counter()
                    TR.measure(h_img[b:b + 1], h_grown[b:b + 1], d, levels, ranges, max_label=max_label)
                    host.append(time.perf_counter() - t0)
                walls, stages = timed(lambda: meas.measure_dense(t_img, grown, d, levels, max_label=max_label), meas.last_timing)
                per = {k: [s[f"texture_{k}_ms"] / a.images for s in stages] for k in ("boxes", "matrices")}
                total = [sum(x) for x in zip(*per.values())]
                cfg = {"channels": nc, "levels": levels, "distance": d}
                for k, v in per.items():
                    cfg[f"{k}_ms_per_image"] = med(v)
                    cfg[f"{k}_ms_per_image_range"] = span(v)
                cfg.update({"device_ms_per_image": med(total), "call_ms_per_image": 1e3 * med(walls) / a.images,
                            "intensity_pass_ms_per_image": med(ipass), "ratio_to_intensity_pass": med(total) / med(ipass),
                            "host_images": len(host), "host_reference_ms_per_image": 1e3 * med(host)})
                res["configs"].append(cfg)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "texture_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
