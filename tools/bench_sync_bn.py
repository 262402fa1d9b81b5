"""What the BatchNormalization exchange costs a data-parallel step: ms per batch-32 forward_backward -> gradient all-reduce ->
apply on ONE GPU with a world-size-1 `nccl` (= RCCL) process group, for the reference graph and for BASELINE.json configs[4]
(128x128 crops, filters 32-64-128 | 128-64-32-1), in three forms measured in one process and alternated:
    none      no synchronisation (per-rank statistics)
    blocking  cs_train_set_sync_bn: the library drains its stream before each of the 12 all-gathers, the hook synchronises after it
    stream    cs_train_set_sync_bn_stream: the all-gathers are ordered on the handle's stream, the host waits once per step
World size 1 is the only multi-rank arithmetic one GPU can time honestly: the collective's launch path is real, its wire time
is not (multi-GPU wire time: not measured).  For the reference graph `blocking` is what the step did before the stream-ordered
hook existed; for configs[4] `none` is the only earlier figure.
Timing: a warm-up of every form first, then --repeats rounds; in a round each form runs --steps steps inside a host-clock window
that ends in a device synchronise.  Prints one JSON object (and writes it to --out).
Usage: python tools/bench_sync_bn.py [--steps 200] [--warmup 20] [--repeats 3] [--out FILE]"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cell-image-analysis_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from cellscreen import dist as csdist, synth  # noqa: E402
from cellscreen.trainer import Trainer  # noqa: E402

FORMS = ("none", "blocking", "stream")
SHAPES = {"reference": ((64, 64), None, 3), "configs4": ((128, 128), (32, 64, 128, 128, 64, 32, 1), 3)}


def make(shape, form):
    hw, ch, ne = SHAPES[shape]
    w = synth.random_cae(seed=5, trivial_bn=True) if ch is None else synth.random_cae(seed=5, hw=hw, channels=ch, n_enc=ne, trivial_bn=True)
    tr = Trainer(w)
    g = torch.zeros(tr.n_trainable, dtype=torch.float32, device="cuda")
    tr.use_grad_tensor(g)
    if form != "none":
        tr.enable_sync_bn(dist, 0, 1, blocking=form == "blocking")
    return tr, g


def run(tr, g, x, steps):
    for _ in range(steps):
        tr.forward_backward(x, x)
        csdist.allreduce_mean_(g)
        tr.apply(1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    result = {"workload": f"batch-{a.batch} forward_backward -> all-reduce -> apply, world-size-1 nccl on one GPU", "steps": a.steps,
              "warmup": a.warmup, "repeats": a.repeats, "multi_gpu_wire_time": "not measured", "shapes": {}}
    try:
        for shape, (hw, _ch, _ne) in SHAPES.items():
            x = torch.from_numpy(synth.blob_crops(7, a.batch, **({} if hw == (64, 64) else {"hw": hw}))).cuda()
            handles = {f: make(shape, f) for f in FORMS}
            for f in FORMS:
                run(*handles[f], x, a.warmup)
            torch.cuda.synchronize()
            ms = {f: [] for f in FORMS}
            for _ in range(a.repeats):
                for f in FORMS:                                    # alternated: every form in every round
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(*handles[f], x, a.steps)
                    torch.cuda.synchronize()
                    ms[f].append((time.perf_counter() - t0) / a.steps * 1e3)
            for tr, _g in handles.values():
                tr.close()
            med = {f: float(np.median(v)) for f, v in ms.items()}
            result["shapes"][shape] = {
                "ms_per_step": {f: [round(v, 4) for v in ms[f]] for f in FORMS},
                "median_ms": {f: round(med[f], 4) for f in FORMS},
                "spread_ms": {f: round(max(ms[f]) - min(ms[f]), 4) for f in FORMS},
                "stream_over_blocking": round(med["stream"] / med["blocking"], 4),
                "blocking_over_none": round(med["blocking"] / med["none"], 4),
                "stream_over_none": round(med["stream"] / med["none"], 4)}
    finally:
        dist.destroy_process_group()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
