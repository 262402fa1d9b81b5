"""bench.py as the benchmark driver runs it, at a small size: a plain run prints the headline line without the figures that
--full adds, --steps sets the timed steps, and --dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from cellscreen import synth
from oracle import oracle


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    n, seed = 8192, 42
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--cells", str(n),
           "--chunk", "4096", "--train-cells", "1000", "--seed", str(seed), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "cells/s" and line["higher_is_better"] is True
    assert line["metric"].startswith("cells/sec screened") and line["dtype"].startswith("f32")
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-2
    for k in ("whole_path", "roofline", "kernels", "cpu_baseline", "small_n", "exact_fp32", "e2e_raw", "train_leg", "large_variant"):
        assert k not in line, k

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"mse", "mae", "cons_score", "mod_score", "cons_pred", "mod_pred"}
    for k, a in got.items():
        assert a.shape == (n,) and a.dtype == (np.float64 if k.endswith("_score") else np.float32) and np.all(np.isfinite(a)), k
    for k in ("cons_pred", "mod_pred"):
        assert set(np.unique(got[k])) <= {-1.0, 1.0}
    # the reconstruction errors do not depend on the detector fit: cells 0.. of the run against the fp64-accumulating oracle
    m = 64
    ref = oracle.cae_forward(synth.random_cae(seed=seed), oracle.synth_crops(seed, 0, m), acc64=True, want=("mse", "mae"))
    H.assert_rel(got["mse"][:m], ref["mse"], H.TOL_ERR_REL, "dumped mse")
    H.assert_rel(got["mae"][:m], ref["mae"], H.TOL_ERR_REL, "dumped mae")
