"""Side bench of the crop preprocess at other output sizes: the workload of bench_preprocess.py (raw ragged uint16
bounding-box crops resident in HBM, synth.raw_crops seed 7, sides U[32,100], 512 distinct crops cycled) ->
float32 [n,out_h,out_w] resident in HBM, for each --out-hw.  One JSON line per size; the lines are also written to
--out (default profiles/preprocess_sized_bench.json, merged into what that file already holds under "sizes").

    python tools/bench_preprocess_sized.py [--out-hw 64x64 128x128 64x128] [--crops N] [--steps K] [--warmup W]

hbm_bytes_per_crop is the algorithmic traffic: the crop's raw pixels in (2 B each) + 4 * out_h * out_w bytes out.  The work
per crop grows with the output (the fp64 warp is per output pixel: 4 x at 128x128), so the rates of different sizes are
recorded side by side, not compared.

--dump FILE stores what one pass produced -- the first --dump-cells cells as they are plus the sha256 of all of them -- so
that two trees can be compared bit for bit; --tree DIR benches the package of another checkout of this project (one that
may predate out_hw: 64x64 is then run through a handle that is never told a size)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_hw(s):
    h, w = s.lower().split("x")
    return int(h), int(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-hw", nargs="+", default=["64x64", "128x128", "64x128"])
    ap.add_argument("--crops", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-side", type=int, default=32)
    ap.add_argument("--max-side", type=int, default=100)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_sized_bench.json"))
    ap.add_argument("--dump", default=None)
    ap.add_argument("--dump-cells", type=int, default=1024)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(tree, "cell-image-analysis_amd"))
    sys.path.insert(0, tree)
    import torch
    from cellscreen import preprocess as pp
    from cellscreen import synth

    base = synth.raw_crops(7, 512, np.uint16, a.min_side, a.max_side)
    crops = [base[i % len(base)] for i in range(a.crops)]
    pix, off, hs, ws = pp.pack_crops(crops)
    d_pix = torch.from_numpy(pix.view(np.int16)).cuda()
    lines = []
    for hw in (parse_hw(s) for s in a.out_hw):
        proc = pp.Preprocessor(0) if hw == (64, 64) else pp.Preprocessor(0, out_hw=hw)
        d_out = torch.empty((a.crops,) + hw, dtype=torch.float32, device="cuda")
        for _ in range(a.warmup):
            proc.run_packed(d_pix, off, hs, ws, out=d_out)
        torch.cuda.synchronize()
        walls, kms = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            proc.run_packed(d_pix, off, hs, ws, out=d_out)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
            kms.append(proc.last_timing()[0])
        dt, km = float(np.median(walls)), float(np.median(kms))
        bytes_crop = pix.nbytes / a.crops + 4.0 * hw[0] * hw[1]
        line = {"metric": "crops_preprocessed_per_second", "out_hw": list(hw), "value": a.crops / dt, "unit": "crops/s",
                "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt * 1e3, "kernel_ms": km,
                "runs_crops_per_s": [a.crops / w for w in walls], "higher_is_better": True,
                "hbm_bytes_per_crop": bytes_crop, "hbm_GBps_algorithmic": bytes_crop * a.crops / (km * 1e-3) / 1e9,
                "config": {"workload": f"{a.crops} uint16 crops, sides U[{a.min_side},{a.max_side}], CLAHE(0.02)+resize {hw[0]}x{hw[1]}",
                           "mean_pixels": float(pix.size / a.crops)}}
        if a.dump and hw == parse_hw(a.out_hw[0]):
            sha = hashlib.sha256()
            step = max(1, (256 << 20) // (4 * hw[0] * hw[1]))
            for i in range(0, a.crops, step):
                sha.update(d_out[i:i + step].cpu().numpy().tobytes())
            os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
            np.savez(a.dump, cells=d_out[:a.dump_cells].cpu().numpy(), sha256=np.array(sha.hexdigest()), n=np.int64(a.crops))
            line["dump"] = {"file": os.path.basename(a.dump), "sha256_all_cells": sha.hexdigest()}
        proc.close()
        del d_out
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc.setdefault("sizes", {})
        for ln in lines:
            doc["sizes"]["%dx%d" % tuple(ln["out_hw"])] = ln
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
