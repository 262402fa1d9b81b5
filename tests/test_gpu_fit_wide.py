"""PCA of wide encoder features on the device (cs_fit_pca_subspace: block subspace iteration, nothing F x F) against an
exact fp64 PCA of the same scaled, float32-centred features, against the covariance path where both apply, and end to
end on the BASELINE.json configs[4] model (128 x 128 crops, filters 32-64-128 | 128-64-32-1: F = 32,768), whose detector
the covariance path cannot fit."""
import os
import pickle

import numpy as np
import pytest

from cellscreen import detector_fit as df
from cellscreen import synth
from cellscreen.engine import Engine

pytestmark = pytest.mark.gpu

LARGE_HW = (128, 128)
LARGE_CH = (32, 64, 128, 128, 64, 32, 1)
PLANTED = 24


@pytest.fixture(scope="module")
def fitter():
    f = df.Fitter(0)
    yield f
    f.close()


def _features(n, F, seed=0, dup=False):
    """Planted low-rank structure + noise through a ReLU, with dead columns (the style of test_gpu_fit._features)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(n, PLANTED)).astype(np.float32)
    w = rng.normal(size=(PLANTED, F)).astype(np.float32)
    x = np.maximum(z @ w * 0.2 + rng.normal(size=(n, F)).astype(np.float32) * 0.3 + 0.2, 0).astype(np.float32)
    x[:, :4] = 0.0                                          # dead features: IQR 0 -> scale 1
    if dup:
        x[1::2] = x[0::2][: n // 2]                         # every cell twice
        x[:, 7] = 3.0                                       # and a constant column
    return x


def _centred(x, center, scale):
    from sklearn.preprocessing import RobustScaler
    s = RobustScaler()
    s.center_, s.scale_ = center, scale
    xs = s.transform(x)
    return xs, (xs - xs.mean(axis=0)).astype(np.float64)   # PCA centres in float32; the reference factorises exactly


def _exact_pca(xc, k):
    """fp64 PCA of the centred features: eigh of the smaller of the two Gram matrices; ordered and signed like PCA.fit."""
    n, F = xc.shape
    if F <= n:
        w, v = np.linalg.eigh(xc.T @ xc)
        w, v = w[::-1][:k], v[:, ::-1][:, :k].T
    else:
        w, u = np.linalg.eigh(xc @ xc.T)
        w, u = w[::-1][:k], u[:, ::-1][:, :k]
        v = (xc.T @ u).T / np.sqrt(w)[:, None]
        v /= np.linalg.norm(v, axis=1, keepdims=True)
    idx = np.argmax(np.abs(v), axis=1)
    v *= np.sign(v[np.arange(k), idx])[:, None]
    return v, np.maximum(w, 0) / (n - 1)


def _captured(xc, comps):
    return float((np.linalg.norm(xc @ comps.T, axis=0) ** 2).sum() / (xc.shape[0] - 1))


def _check_exact(comps, ev, total, xc, lead=PLANTED, ev_rtol=2e-3):
    k = comps.shape[0]
    ref, ref_ev = _exact_pca(xc, k)
    dots = np.sum(comps[:lead] * ref[:lead], axis=1)
    assert dots.min() >= 1 - 1e-6, dots.min()                                   # same planted axes, same signs
    assert np.abs(ev[:lead] - ref_ev[:lead]).max() <= 1e-9 * ref_ev[:lead].min()
    rel = np.abs(ev - ref_ev) / ref_ev
    assert rel.max() <= ev_rtol, (rel.max(), int(rel.argmax()))
    cap = _captured(xc, comps)
    assert cap >= (1 - 1e-5) * ref_ev.sum(), (cap, ref_ev.sum())
    assert np.abs(comps @ comps.T - np.eye(k)).max() <= 1e-10
    assert abs(total - (xc ** 2).sum() / (xc.shape[0] - 1)) <= 1e-10 * total
    return cap


@pytest.fixture(scope="module")
def wide(fitter):
    x = _features(3000, 32768, seed=1)
    center, scale = fitter.scaler(x)
    xs, xc = _centred(x, center, scale)
    return x, center, scale, xs, xc


def test_subspace_pca_of_wide_features_is_exact(fitter, wide):
    from sklearn.decomposition import PCA
    x, center, scale, xs, xc = wide
    mean, comps, ev, total, n_iter = fitter.pca_subspace(x, center, scale, 100)
    assert np.array_equal(mean, xs.mean(axis=0))                                # PCA.fit's mean_, bit for bit
    assert comps.shape == (100, 32768) and comps.dtype == np.float64 and 7 <= n_iter <= 100
    cap = _check_exact(comps, ev, total, xc)
    rnd = PCA(n_components=100, svd_solver="randomized", random_state=0).fit(xs)  # what the reference's 'auto' picks here
    assert cap >= _captured(xc, rnd.components_.astype(np.float64)) * (1 - 1e-12)
    print(f"n_iter {n_iter}, captured {cap:.6g}")


def test_subspace_pca_is_deterministic(fitter, wide):
    x, center, scale, _, _ = wide
    import torch
    a = fitter.pca_subspace(x, center, scale, 100)
    b = fitter.pca_subspace(torch.from_numpy(x).cuda(), center, scale, 100)     # from device memory, same numbers
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))


def test_subspace_agrees_with_the_covariance_path(fitter):
    x = _features(3001, 2048, seed=0)
    center, scale = fitter.scaler(x)
    _, xc = _centred(x, center, scale)
    mean_c, scatter = fitter.pca_moments(x, center, scale)
    comps_c, ev_c, total_c = df.principal_axes(scatter, x.shape[0], 100)
    mean, comps, ev, total, _ = fitter.pca_subspace(x, center, scale, 100)
    assert np.array_equal(mean, mean_c)
    _check_exact(comps, ev, total, xc)
    assert np.abs(np.sum(comps[:PLANTED] * comps_c[:PLANTED], axis=1)).min() >= 1 - 1e-6
    assert np.abs(ev - ev_c).max() <= 2e-3 * ev_c.min() and abs(total - total_c) <= 1e-9 * total_c


def test_auto_solver_keeps_the_covariance_path_where_it_applies():
    x = _features(1500, 2048, seed=4)
    ta, tc, ts = {}, {}, {}
    det_a, objs_a = df.fit_detector_device(x, timings=ta)
    det_c, _ = df.fit_detector_device(x, timings=tc, pca_solver="covariance")
    det_s, objs_s = df.fit_detector_device(x, timings=ts, pca_solver="subspace")
    assert ta["pca_solver"] == tc["pca_solver"] == "covariance" and ts["pca_solver"] == "subspace"
    for name in ("pca_components", "pca_mean_proj", "scaler_center", "scaler_scale"):
        assert np.array_equal(getattr(det_a, name), getattr(det_c, name)), name
    assert np.array_equal(det_a.moderate.dual_coef, det_c.moderate.dual_coef)
    assert objs_a["pca"]._fit_svd_solver == "covariance_eigh" and objs_s["pca"]._fit_svd_solver == "randomized"
    with pytest.raises(ValueError):
        df.fit_detector_device(x, pca_solver="randomized")


def test_subspace_pca_of_narrow_odd_widths(fitter):
    """Any width, not only encoder output: F = 200 (not a multiple of 128) and F = 37 (the block spans everything)."""
    from sklearn.decomposition import PCA
    for F, k in ((200, 100), (37, 30)):
        x = _features(3000, F, seed=F)
        center, scale = fitter.scaler(x)
        xs, xc = _centred(x, center, scale)
        mean, comps, ev, total, _ = fitter.pca_subspace(x, center, scale, k)
        assert np.array_equal(mean, xs.mean(axis=0))
        _check_exact(comps, ev, total, xc, lead=min(PLANTED, k))
        full = PCA(n_components=k, svd_solver="full").fit(xs)                  # scikit-learn's exact solver, float32
        assert np.allclose(ev, full.explained_variance_, rtol=2e-4, atol=1e-6 * ev[0])
        assert np.sum(comps[:min(PLANTED, k)] * full.components_[:min(PLANTED, k)], axis=1).min() > 1 - 1e-3


def test_subspace_pca_with_duplicated_cells_and_constant_columns(fitter):
    """Every cell twice and a constant column: the orthonormalisation must not break on the rank the data lacks."""
    x = _features(2000, 4096 + 72, seed=8, dup=True)
    center, scale = fitter.scaler(x)
    _, xc = _centred(x, center, scale)
    mean, comps, ev, total, _ = fitter.pca_subspace(x, center, scale, 100)
    assert np.all(np.isfinite(comps))
    _check_exact(comps, ev, total, xc)
    # fewer distinct cells than the block is wide: 40 cells, 20 distinct (rank 19); components 20.. span no variance
    x = _features(40, 4096, seed=9, dup=True)
    center, scale = fitter.scaler(x)
    _, xc = _centred(x, center, scale)
    mean, comps, ev, total, _ = fitter.pca_subspace(x, center, scale, 39)
    assert np.abs(comps @ comps.T - np.eye(39)).max() <= 1e-10
    ref, ref_ev = _exact_pca(xc, 19)
    assert np.abs(ev[:19] - ref_ev).max() <= 1e-9 * ref_ev[0] and ev[19:].max() <= 1e-9 * ref_ev[0]
    assert np.abs(np.sum(comps[:19] * ref, axis=1)).min() >= 1 - 1e-6


def test_subspace_refusals(fitter):
    import ctypes as C
    lib = fitter._lib
    x = np.ones((10, 300), np.float32)
    c, s = np.zeros(300, np.float32), np.ones(300)
    mean, comps, ev = np.empty(300, np.float32), np.empty((128, 300)), np.empty(128)
    tot, it = C.c_double(), C.c_int32()

    def call(n=10, F=300, k=5, mean_p=mean.ctypes.data, comps_p=comps.ctypes.data, ev_p=ev.ctypes.data, tot_p=C.byref(tot)):
        return lib.cs_fit_pca_subspace(fitter._h, x.ctypes.data, n, F, 0, c.ctypes.data, s.ctypes.data, k, 0, mean_p, comps_p,
                                       ev_p, tot_p, C.byref(it))
    INVALID = -1                                                                # CS_ERR_INVALID
    for kw in (dict(mean_p=None), dict(comps_p=None), dict(ev_p=None), dict(tot_p=None), dict(k=0), dict(k=10), dict(k=129),
               dict(n=0), dict(F=0), dict(F=(1 << 20) + 1), dict(n=1, k=1)):
        assert call(**kw) == INVALID, kw
    assert call(k=9) == 0 and it.value >= 4
    with pytest.raises(RuntimeError, match="n_components"):
        fitter.pca_subspace(np.ones((300, 200), np.float32), c[:200], s[:200], 129)


def test_device_fit_with_fewer_cells_than_components_on_wide_features():
    """60 cells of the configs[4] model (F = 32,768): 59 components, which scikit-learn's PCA computes with its exact 'full'
    solver -- the block is the whole row space and the answer is exact."""
    w = synth.random_cae(seed=5, hw=LARGE_HW, channels=LARGE_CH, n_enc=3)
    e0 = Engine.from_weights(w, None, None)
    feats = e0.encode(synth.blob_crops(3, 60, hw=LARGE_HW), which=0)
    test = e0.encode(synth.blob_crops(4, 200, hw=LARGE_HW), which=0)
    e0.close()
    assert feats.shape == (60, 32768)
    t = {}
    det, objs = df.fit_detector_device(feats, timings=t)
    det_sk, objs_sk = df.fit_detector(feats)
    assert t["pca_solver"] == "subspace"
    assert det.n_components == det_sk.n_components == 59 and objs_sk["pca"]._fit_svd_solver == "full"
    assert np.array_equal(det.pca_mean, det_sk.pca_mean)
    xs = objs["scaler"].transform(feats)
    xc = (xs - xs.mean(axis=0)).astype(np.float64)
    ref, ref_ev = _exact_pca(xc, 59)
    ev = objs["pca"].explained_variance_
    assert np.abs(ev - ref_ev).max() <= 1e-9 * ref_ev[0]
    assert np.allclose(ev, objs_sk["pca"].explained_variance_, rtol=1e-3, atol=1e-5 * ref_ev[0])
    lead = int(np.sum(ref_ev > 1e-3 * ref_ev[0]))
    dots = np.sum(det.pca_components[:lead].astype(np.float64) * det_sk.pca_components[:lead], axis=1)
    assert np.all(dots > 0.98), dots.min()
    for name in ("Conservative", "Moderate"):
        mine = objs["detectors"][name].decision_function(objs["pca"].transform(objs["scaler"].transform(test)))
        ref_d = objs_sk["detectors"][name].decision_function(objs_sk["pca"].transform(objs_sk["scaler"].transform(test)))
        assert np.corrcoef(mine, ref_d)[0, 1] > 0.995
        assert ((mine < 0) == (ref_d < 0)).mean() >= 0.97


def test_large_variant_detector_fits_and_screens_on_the_device(tmp_path):
    """The configs[4] model end to end on the default path: create_anomaly_detector(encoder, crops) fits on the device,
    ProductionMutantScreening loads the directory and scores like the unpickled objects and like an all-scikit-learn fit."""
    from cellscreen.screening import ProductionMutantScreening
    from cellscreen.training import ImprovedAnomalyDetectionTraining
    w = synth.random_cae(seed=5, hw=LARGE_HW, channels=LARGE_CH, n_enc=3)
    cells = synth.blob_crops(21, 3000, hw=LARGE_HW)
    out = str(tmp_path / "large")
    t = ImprovedAnomalyDetectionTraining(out, verbose=0, detector_fit="device")
    detectors, scaler, pca = t.create_anomaly_detector(w.encoder_half(), cells, autoencoder=w)
    assert pca.n_components_ == 100 and pca.components_.shape == (100, 32768)
    assert np.isclose(pca.explained_variance_ratio_.sum() + pca.noise_variance_ * (min(3000, 32768) - 100) /
                      (pca.explained_variance_ / pca.explained_variance_ratio_)[0], 1.0, rtol=1e-6)
    test = synth.blob_crops(22, 600, hw=LARGE_HW)
    test[::5] = synth.synth_crops(23, 0, 120, hw=LARGE_HW)                      # some crops unlike the training set
    s = ProductionMutantScreening(out)
    r = s.compute_anomaly_scores(list(test))
    tf = s.engine.encode(test, which=1)
    for name in ("scaler.pkl", "pca.pkl", "detector_conservative.pkl", "detector_moderate.pkl"):
        with open(os.path.join(out, name), "rb") as f:
            pickle.load(f)
    with open(os.path.join(out, "pca.pkl"), "rb") as f:
        pca_u = pickle.load(f)
    with open(os.path.join(out, "scaler.pkl"), "rb") as f:
        scaler_u = pickle.load(f)
    red = pca_u.transform(scaler_u.transform(tf.copy()))
    e0 = Engine.from_weights(w, None, None)
    feats = e0.encode(cells, which=0)
    e0.close()
    det_sk, objs_sk = df.fit_detector(feats, pca_random_state=0)
    red_sk = objs_sk["pca"].transform(objs_sk["scaler"].transform(tf.copy()))
    for name, key in (("Conservative", "conservative"), ("Moderate", "moderate")):
        with open(os.path.join(out, f"detector_{key}.pkl"), "rb") as f:
            det_u = pickle.load(f)
        dec = det_u.decision_function(red)
        mine = -r[f"{key}_scores"]
        assert np.abs(mine - dec).max() <= 1e-4 * max(1.0, np.abs(dec).max())
        d_sk = objs_sk["detectors"][name].decision_function(red_sk)
        rate_sk, rate = (d_sk < 0).mean(), (mine < 0).mean()
        agree = ((d_sk < 0) == (mine < 0)).mean()
        assert agree >= 0.97, f"{name}: flag agreement {agree:.3f}"
        assert abs(rate - rate_sk) <= 0.03, f"{name}: anomaly rate {rate:.3f} vs {rate_sk:.3f}"
        assert np.corrcoef(d_sk, mine)[0, 1] > 0.99
