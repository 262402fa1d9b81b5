"""Throughput of the quality-cell extraction from label images (cellscreen.extract, csrc/extract.hip): 32 images of
2048 x 2048 x 3 uint16 with about 1,000 labels each (synth.label_images), resident on the device, through the whole chain
from label image to the [n,64,64] cells.  Prints one JSON line:

  images_per_s, regions_per_s, cells_per_s      whole chain (two library calls, wall clock), median of --reps
  label_ms, region_ms, cells_ms                 HIP-event times of the label pass, the per-region pass (+ scan) and the
                                                gather + preprocess, median and [min, max] over the repetitions
  label_pass_TBps, label_pass_hbm_share         label bytes read (4 B per pixel) over the label-pass time, share of 8 TB/s
  screen_cells_per_s                            (--screen) the same cells through cs_screen afterwards
  restatement_*                                 the CPU restatement (tests/extract_reference.py, numpy + scipy) on
                                                --restate images, for scale: it is the tests' reference, not a product path

Usage: python tools/bench_extract.py [--images 32] [--side 2048] [--cells 1000] [--reps 10] [--screen] [--restate 1]"""
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--screen", action="store_true")
    ap.add_argument("--restate", type=int, default=1)
    a = ap.parse_args()

    import torch
    from cellscreen import extract as X
    from cellscreen import synth

    imgs, labs = synth.label_images(2024, a.images, hw=(a.side, a.side), n_cells=a.cells)
    dev = torch.device("cuda", 0)
    ti = torch.from_numpy(imgs.view(np.int16)).to(dev)
    tl = torch.from_numpy(labs).to(dev)
    torch.cuda.synchronize()
    ext = X.CellExtractor(0)
    for _ in range(a.warmup):
        r = ext.extract_batch(ti, tl)
    walls, times = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ext.extract_batch(ti, tl)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        times.append(ext.last_timing())
    n_reg, n_cell = len(r.regions), int(r.cells.shape[0])
    wall = float(np.median(walls))
    spread = lambda k: [round(float(np.median([t[k] for t in times])), 4), round(min(t[k] for t in times), 4),
                        round(max(t[k] for t in times), 4)]
    label_ms = float(np.median([t["label_ms"] for t in times]))
    label_bytes = labs.nbytes
    res = {
        "images": a.images, "side": a.side, "regions": n_reg, "cells": n_cell,
        "images_per_s": round(a.images / wall, 2), "regions_per_s": round(n_reg / wall, 1), "cells_per_s": round(n_cell / wall, 1),
        "wall_ms": [round(wall * 1e3, 3), round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)],
        "label_ms": spread("label_ms"), "region_ms": spread("region_ms"), "cells_ms": spread("cells_ms"),
        "label_bytes": label_bytes,
        "label_pass_TBps": round(label_bytes / (label_ms * 1e-3) / 1e12, 3),
        "label_pass_hbm_share": round(label_bytes / (label_ms * 1e-3) / HBM_PEAK, 3),
        "reps": a.reps,
    }
    if a.screen:
        from cellscreen.detector_fit import fit_detector
        from cellscreen.engine import Engine
        w = synth.random_cae(seed=42)
        e0 = Engine.from_weights(w, device_id=0)
        xt = np.concatenate([synth.synth_crops(42, 0, 1000), synth.blob_crops(5, 32)])
        det, _ = fit_detector(e0.encode(xt, which=0), pca_random_state=0)
        e0.close()
        eng = Engine.from_weights(w, None, det, device_id=0)
        eng.screen(r.cells)
        torch.cuda.synchronize()
        sw = []
        for _ in range(max(3, a.reps // 2)):
            t0 = time.perf_counter()
            eng.screen(r.cells)
            torch.cuda.synchronize()
            sw.append(time.perf_counter() - t0)
        res["screen_cells_per_s"] = round(n_cell / float(np.median(sw)), 1)
        res["extract_plus_screen_cells_per_s"] = round(n_cell / (wall + float(np.median(sw))), 1)
        eng.close()
    if a.restate > 0:
        import extract_reference as R
        t0 = time.perf_counter()
        nr = 0
        for b in range(a.restate):
            _, regs, _ = R.extract(labs[b], imgs[b, ..., 1])
            nr += len(regs)
        dt = time.perf_counter() - t0
        res["restatement_images_per_s"] = round(a.restate / dt, 4)
        res["restatement_regions_per_s"] = round(nr / dt, 1)
        res["restatement_note"] = "CPU restatement of the tests (numpy + scipy, one process), not scikit-image"
    ext.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
