"""Throughput of the per-object granularity spectrum (cs_label_granularity, cellscreen/granularity.py, csrc/granularity.hip) and
writes profiles/granularity_bench.json.  The workload is the other label benches': --images fields of 2048 x 2048 with 640 cells
each (synth.label_images), uint16, resident on the device; the objects are the painted labels grown by 6 px (LabelExpander).  The
records and the planes of a 256 x 256 corner of one field are compared with tests/granularity_reference.py in every configuration
first.  Then, for 16 steps, 1 and 3 channels and subsample 1 and 4:

  prepare_ms_per_image, steps_ms_per_image, sums_ms_per_image
                                         HIP-event times of the three parts (the clearing is in the first; the second is the
                                         erosions with their reconstructions; the third the steps + 1 sums passes): median and
                                         [min, max] over the repetitions
  device_ms_per_image                    their sum
  call_ms_per_image                      GranularityMeasurer.measure_dense, wall clock: the parts, the reads of the control word,
                                         the records to the host
  rounds_per_step, reads_per_step        reconstruction rounds and control-word reads of a call, over its steps
  ratio_to_intensity_pass                device_ms / cs_label_intensity's pass (IntensityMeasurer, same fields and channels, same run)
and once per subsample, beside the configurations and not in them (host_scipy):
  ms, dilations_per_step                 the SciPy form on the host for ONE channel of a --host-side x --host-side corner of one
                                         field (not a whole field and not the device's workload: see host_scipy_note; no ratio to
                                         the device figures is formed): per step scipy.ndimage.grey_erosion,
                                         scipy.ndimage.grey_dilation and numpy.minimum repeated to the fixed point, and
                                         scipy.ndimage.sum_labels
No time is a pass condition.

Usage: python tools/bench_granularity.py [--images 8] [--side 2048] [--cells 640] [--reps 5] [--warmup 1] [--host-side 512]"""
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
SUBSAMPLES = (1, 4)
STEPS = 16
GROW = 6
PARTS = ("prepare", "steps", "sums")


def scipy_form(plane, labels, steps, s):
    """One channel [H,W] on the host with SciPy: the sums [n,steps+1] per object, for the time it takes; also the dilations it took."""
    from scipy import ndimage as ndi
    cross = ndi.generate_binary_structure(2, 1)
    H, W = plane.shape
    hs, ws = -(-H // s), -(-W // s)
    tot = np.zeros((hs * s, ws * s), np.int64)
    cnt = np.zeros((hs * s, ws * s), np.int64)
    tot[:H, :W] = plane
    cnt[:H, :W] = 1
    tot, cnt = tot.reshape(hs, s, ws, s).sum(axis=(1, 3)), cnt.reshape(hs, s, ws, s).sum(axis=(1, 3))
    p = (2 * tot + cnt) // (2 * cnt)
    rr, cc = np.mgrid[0:H, 0:W]
    index = np.unique(labels[labels > 0])
    out, e, dilations = [ndi.sum_labels(p[rr // s, cc // s], labels, index)], p, 0
    for _ in range(steps):
        e = ndi.grey_erosion(e, footprint=cross, mode="reflect")
        r = e
        while True:
            n = np.minimum(ndi.grey_dilation(r, footprint=cross, mode="constant", cval=0), p)
            dilations += 1
            if np.array_equal(n, r):
                break
            r = n
        out.append(ndi.sum_labels(r[rr // s, cc // s], labels, index))
    return np.stack(out, axis=1), dilations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-side", type=int, default=512)
    a = ap.parse_args()

    import torch

    import granularity_reference as GR
    from build import source_hash
    from cellscreen import expand as EX
    from cellscreen import granularity as GA
    from cellscreen import intensity as IN
    from cellscreen import synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_granularity needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))
    span = lambda v: [float(np.min(v)), float(np.max(v))]
    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    tl = torch.from_numpy(labs).to(dev)
    grown = EX.LabelExpander(0).expand_batch(tl, GROW)
    h_grown = grown.cpu().numpy()
    max_label = int(labs.max())
    meas = GA.GranularityMeasurer(0)
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

    corner, hside = min(a.side, 256), min(a.side, a.host_side)
    res = {"tool": "bench_granularity", "source_hash": source_hash(), "images": a.images, "side": a.side, "cells": a.cells, "reps": a.reps,
           "warmup": a.warmup, "pixel_type": "uint16", "grown_by": GROW, "max_label": max_label, "steps": STEPS,
           "labelled_fraction": float((h_grown > 0).mean()),
           "objects_per_image": float(np.mean([len(np.unique(x)) - 1 for x in h_grown])),
           "checked": f"the records and the planes of a {corner} x {corner} corner of one field equal tests/granularity_reference.py in every configuration",
           "host_scipy_note": f"host_scipy is ONE channel of a {hside} x {hside} corner of one field, not a whole field and not the workload of the "
                              "device figures: the dilations to the fixed point per step grow with the side",
           "configs": []}
    host = {}
    for s in SUBSAMPLES:
        t0 = time.perf_counter()
        _, dil = scipy_form(imgs[0, :hside, :hside, 0], h_grown[0, :hside, :hside], STEPS, s)
        host[s] = (1e3 * (time.perf_counter() - t0), dil)
    res["host_scipy"] = [{"subsample": s, "side": hside, "channels": 1, "ms": host[s][0], "dilations_per_step": host[s][1] / STEPS} for s in SUBSAMPLES]
    for nc in CHANNELS:
        h_img = np.ascontiguousarray(imgs[..., :nc])
        t_img = torch.from_numpy(h_img.view(np.int16)).to(dev)
        _, i_stages = timed(lambda: inten.measure_dense(t_img, grown, max_label=max_label), inten.last_timing)
        ipass = [x["intensity_pass_ms"] / a.images for x in i_stages]
        for s in SUBSAMPLES:
            kw = dict(steps=STEPS, subsample=s, max_label=max_label)
            c_img, c_lab = np.ascontiguousarray(h_img[:1, :corner, :corner]), np.ascontiguousarray(h_grown[:1, :corner, :corner])
            got = meas.measure_dense(c_img, c_lab, want_planes=True, **kw)
            want = GR.measure(c_img, c_lab, **kw)
            if not all(np.array_equal(g, w) for g, w in zip(got, want)):
                raise SystemExit(f"the records differ from tests/granularity_reference.py at {nc} channels, subsample {s}")
            rounds = []
            walls, stages = timed(lambda: (meas.measure_dense(t_img, grown, **kw), rounds.append(meas.last_rounds())), meas.last_timing)
            per = {k: [x[f"granularity_{k}_ms"] / a.images for x in stages] for k in PARTS}
            total = [sum(x) for x in zip(*per.values())]
            cfg = {"channels": nc, "subsample": s}
            for k, v in per.items():
                cfg[f"{k}_ms_per_image"] = med(v)
                cfg[f"{k}_ms_per_image_range"] = span(v)
            cfg.update({"device_ms_per_image": med(total), "device_ms_per_image_range": span(total), "call_ms_per_image": 1e3 * med(walls) / a.images,
                        "rounds_per_step": rounds[-1][0] / STEPS, "reads_per_step": rounds[-1][1] / STEPS,
                        "intensity_pass_ms_per_image": med(ipass), "ratio_to_intensity_pass": med(total) / med(ipass)})
            res["configs"].append(cfg)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "granularity_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
