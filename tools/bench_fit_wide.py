"""Detector fit (CAE_improved_modeltrain.py:408-427) on wide encoder features: the BASELINE.json configs[4] model (128 x 128
crops, filters 32-64-128 | 128-64-32-1, F = 32,768), N training cells encoded on the device.  The covariance path cannot
take F > 8192, so fit_detector_device runs the PCA as block subspace iteration (cs_fit_pca_subspace).  Times the device
fit per phase at --n and, with --sklearn-n, the host scikit-learn fit the reference runs at that (smaller) N together
with the device fit at the same N; prints one JSON line.

    python tools/bench_fit_wide.py --n 50000 --sklearn-n 10000
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cell-image-analysis_amd"))
from build import source_hash  # noqa: E402
from cellscreen import detector_fit as df, synth  # noqa: E402
from cellscreen.engine import Engine  # noqa: E402

LARGE_HW = (128, 128)
LARGE_CH = (32, 64, 128, 128, 64, 32, 1)


def encode(e, n, seed0):
    import torch
    out = torch.empty((n, e.info.feature_dim), dtype=torch.float32, device="cuda")
    for i in range(0, n, 5000):
        m = min(5000, n - i)
        out[i:i + m] = e.encode(torch.from_numpy(synth.blob_crops(seed0 + i, m, hw=LARGE_HW)).cuda(), which=0)
    torch.cuda.synchronize()
    return out


def device_fit(feats, repeat):
    res = {}
    for r in range(repeat):                                    # first pass pays the allocations
        t = {}
        t0 = time.perf_counter()
        det, objs = df.fit_detector_device(feats, timings=t)
        t["total_s"] = time.perf_counter() - t0
        res[f"pass{r}"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
    res["n_sv"] = [det.conservative.n_sv, det.moderate.n_sv]
    return res, det, objs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)          # the reference's training-set size (BASELINE.json configs[1])
    ap.add_argument("--sklearn-n", type=int, default=0, help="also time the host scikit-learn fit at this N (0: skip)")
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    w = synth.random_cae(seed=5, hw=LARGE_HW, channels=LARGE_CH, n_enc=3)
    e = Engine.from_weights(w, None, None)
    feats = encode(e, a.n, 100)
    e.close()
    out = {"tool": "bench_fit_wide", "source_hash": source_hash(), "n": a.n, "n_features": int(feats.shape[1])}
    out["device"], det, _ = device_fit(feats, a.repeat)
    if a.sklearn_n:
        from sklearn.decomposition import PCA
        from sklearn.preprocessing import RobustScaler
        from sklearn.svm import OneClassSVM
        sub = feats[:a.sklearn_n].contiguous()
        out["device_at_sklearn_n"], det_s, objs_s = device_fit(sub, a.repeat)
        x = sub.cpu().numpy()
        t = {}
        t0 = time.perf_counter(); sc = RobustScaler(); xs = sc.fit_transform(x); t["scaler_s"] = time.perf_counter() - t0
        k = min(100, x.shape[1], x.shape[0] - 1)
        t1 = time.perf_counter(); p = PCA(n_components=k, random_state=0); red = p.fit_transform(xs); t["pca_s"] = time.perf_counter() - t1
        iters = []
        for name, nu in (("conservative", 0.05), ("moderate", 0.10)):
            t1 = time.perf_counter(); d = OneClassSVM(kernel="rbf", gamma="scale", nu=nu).fit(red)
            t[f"svm_{name}_s"] = time.perf_counter() - t1; iters.append(int(d.n_iter_))
        t["total_s"] = time.perf_counter() - t0
        out["sklearn"] = {k_: round(v, 3) for k_, v in t.items()}
        out["sklearn"].update(n=a.sklearn_n, svm_iters=iters, pca_solver=p._fit_svd_solver,
                              threads=int(os.environ.get("OMP_NUM_THREADS", "0") or 0))
        out["scaler_equal"] = bool(np.array_equal(det_s.scaler_center, sc.center_) and np.array_equal(det_s.scaler_scale, sc.scale_))
        xc = (xs - xs.mean(axis=0)).astype(np.float64)
        cap = lambda c: float((np.linalg.norm(xc @ np.asarray(c, np.float64).T, axis=0) ** 2).sum() / (len(xc) - 1))  # noqa: E731
        out["captured_variance_device_over_sklearn"] = round(cap(objs_s["pca"].components_) / cap(p.components_), 6)
        out["speedup_at_sklearn_n"] = round(out["sklearn"]["total_s"] / out["device_at_sklearn_n"][f"pass{a.repeat - 1}"]["total_s"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
