"""The detector tail (csrc/detector.hip: scaler_pca_kernel, scaler_pca_x3_kernel<SPLIT>, ocsvm_mfma_kernel<KS, SPLIT> for one
or both detectors, the two range-sum kernels, finalize_kernel) at the shapes where such kernels go wrong: the case list
tests/detector_plans.py SWEEP_CASES (its CPU test proves that it reaches every instantiation and every partition class of
the fixed ranges), in both precisions, against the float64 restatement of tests/helpers.py at the existing bars.  The
float64 SVM runs on sampled cells (the first and last tiles, the ragged tail, a seeded sample); every other cell is tied
to those by the bit identities the code promises: split = unsplit, a cell alone = inside a larger call, cs_screen's
pair-split decisions = cs_svm_decision's per-detector ones, an odd pass size, a repeat, device-resident input.  Plus two
detectors swapped, a one-hot PCA at a ragged width, a NaN feature, refusals, and a device-fitted detector at F < 100
screened against the scikit-learn objects it pickles."""
import copy
import pickle

import numpy as np
import pytest

import detector_plans as D
import helpers as H
from cellscreen import _lib as L
from cellscreen import synth
from cellscreen.engine import Engine

pytestmark = pytest.mark.gpu

PRECISIONS = ("split16", "fp32_exact")
WORST = {}           # (instantiation, precision, bar) -> largest observed error / its bar


def _note(kernel, prec, bar, ratio):
    k = (kernel, prec, bar)
    WORST[k] = max(WORST.get(k, 0.0), ratio)


def _crops(hw, n, seed):
    x = synth.synth_crops(seed, 0, n, hw=hw)
    x[1::2] = synth.blob_crops(seed, n // 2, hw=hw)
    return x


def _sample(n, seed):
    """The first and last 16-cell tiles, the cells past the last whole 64- and 256-cell workgroups, a seeded sample."""
    import random
    cells = set(range(min(16, n))) | set(range(max(0, n - 16), n))
    for wg in (D.PCA_CELLS, D.SVMM_CELLS):
        t = n // wg * wg
        if t < n:
            cells |= {t, (t + n - 1) // 2}
    cells |= set(random.Random(seed).sample(range(n), min(24, n)))
    return np.array(sorted(cells))


def _dev_scaler_pca(e, ft):
    import torch
    o = torch.empty((ft.shape[0], e.info.n_components), dtype=torch.float32, device=ft.device)
    L.order_after_torch(e._lib.cs_model_wait_stream, e._h, ft, o)
    L.check(e._lib.cs_scaler_pca(e._h, ft.data_ptr(), ft.shape[0], L.CS_MEM_DEVICE, o.data_ptr(), L.CS_MEM_DEVICE))
    return o.cpu().numpy()


def _dev_svm_decision(e, pt):
    import torch
    c = torch.empty(pt.shape[0], dtype=torch.float64, device=pt.device)
    m = torch.empty_like(c)
    L.order_after_torch(e._lib.cs_model_wait_stream, e._h, pt, c, m)
    L.check(e._lib.cs_svm_decision(e._h, pt.data_ptr(), pt.shape[0], L.CS_MEM_DEVICE, c.data_ptr(), m.data_ptr(), L.CS_MEM_DEVICE))
    return c.cpu().numpy(), m.cpu().numpy()


def _same(a, b, what):
    """Bit for bit (NaNs in the same places count as equal)."""
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), f"{what}: {k}"


def _tail(e, x, feats):
    pca = e.scaler_pca(feats)
    dc, dm = e.svm_decision(pca)
    return pca, dc, dm, e.screen(x)


@pytest.mark.parametrize("case", D.SWEEP_CASES, ids=[c.id for c in D.SWEEP_CASES])
def test_detector_sweep(case):
    import torch
    F, C, n = case.F, case.C, case.n
    arch = D.arch_for_width(F)
    hw, ch, ne = arch
    w = synth.random_cae(seed=F + C, hw=hw, channels=ch, n_enc=ne)
    e0 = Engine.from_weights(w)
    try:
        assert e0.info.feature_dim == F
        train = e0.encode(_crops(hw, 512, seed=1))
        x = _crops(hw, n, seed=2)
        feats = e0.encode(x)
    finally:
        e0.close()
    det = H.random_detector(F, C, case.n_sv, case.gamma_mult, seed=C, cells=train)
    pca64 = H.pca_ref(det, feats)
    cells = _sample(n, seed=F)
    dets = (("cons", det.conservative), ("mod", det.moderate))
    report = {}
    for prec in PRECISIONS:
        e = Engine.from_weights(w, None, det, precision=prec)
        try:
            prof = e.profile()["scaler_pca"]
            assert (prof["mfma_per_cell"], prof["bf16_mfma_per_cell"]) == D.mfma_per_cell(prec, F, C), prof
            pk = D.call_kernels("scaler_pca", prec, C, n)[0]
            sk = D.call_kernels("svm_decision", prec, C, n)[0]
            ek = D.call_kernels("screen", prec, C, n)
            ek = [k for k in ek if k.startswith("ocsvm")][0]
            pca, dc, dm, res = _tail(e, x, feats)
            r = H.assert_close_scaled(pca, pca64, H.TOL_STAGE, f"{prec} scaler_pca ({pk})") / H.TOL_STAGE
            _note(pk, prec, "TOL_STAGE", r)
            report[(prec, "pca")] = round(r, 3)
            for (name, p), d in zip(dets, (dc, dm)):
                tol = H.TOL_DEC_STAGE * np.abs(p.dual_coef).sum()
                ref = H.ocsvm_ref(p, pca[cells])
                err = np.abs(d[cells] - ref).max()
                assert err <= tol, f"{prec} {name} decision ({sk}): {err:.3e} > {tol:.3e}"
                _note(sk, prec, "TOL_DEC_STAGE", err / tol)
                H.flags_agree(d[cells], np.where(d[cells] > 0, 1, -1), ref, np.where(ref > 0, 1, -1), tol, f"{prec} {name}")
                # cs_screen: the pair-split launch (or the unsplit pair) gives the per-detector decisions bit for bit, and
                # finalize reports score = -dec, flag = sign rule (detector.hip:497-506)
                assert np.array_equal(res[f"{name}_score"], -d), f"{prec} {name}: screen score != -svm_decision"
                assert np.array_equal(res[f"{name}_pred"], np.where(d > 0, 1, -1).astype(np.int8)), f"{prec} {name} flags"
                tol_e = H.TOL_DEC_E2E * np.abs(p.dual_coef).sum()
                ref64 = H.ocsvm_ref(p, pca64[cells])
                err = np.abs(-res[f"{name}_score"][cells] - ref64).max()
                assert err <= tol_e, f"{prec} {name} end to end: {err:.3e} > {tol_e:.3e}"
                _note(ek, prec, "TOL_DEC_E2E", err / tol_e)
                H.flags_agree(-res[f"{name}_score"][cells], res[f"{name}_pred"][cells], ref64, np.where(ref64 > 0, 1, -1), tol_e,
                              f"{prec} {name} end to end")
                report[(prec, name)] = round(err / tol_e, 3)
            want = dict(pca=pca, dc=dc, dm=dm, **res)

            def check(got, what):
                _same({k: got[k] for k in want if k in got}, {k: want[k] for k in want if k in got}, f"{prec} {what}")

            a, b = n // 3, min(n, n // 3 + 77)                        # cells alone = the same cells inside the larger call
            sub = dict(pca=e.scaler_pca(feats[a:b]), **dict(zip(("dc", "dm"), e.svm_decision(pca[a:b]))), **e.screen(x[a:b]))
            _same(sub, {k: v[a:b] for k, v in want.items()}, f"{prec} cells {a}:{b} alone")
            p2, c2, m2, r2 = _tail(e, x, feats)                       # a repeat
            check(dict(pca=p2, dc=c2, dm=m2, **r2), "repeat")
            xd, fd, pd = (torch.from_numpy(v).cuda() for v in (x, feats, pca))     # device-resident input and output
            rd = {k: v.cpu().numpy() for k, v in e.screen(xd).items()}
            cd, md = _dev_svm_decision(e, pd)
            check(dict(pca=_dev_scaler_pca(e, fd), dc=cd, dm=md, **rd), "device input")
            del xd, fd, pd
            e.set_chunk(n // 3 | 1)                                   # an odd pass size: other passes, other ragged tails
            check(dict(pca=e.scaler_pca(feats), **e.screen(x)), f"chunk {n // 3 | 1}")
            if n > D.DET_SPLIT_MAX_CELLS:                             # one pass of n cells: the unsplit kernels
                e.set_chunk(n)
                check(dict(pca=e.scaler_pca(feats), **e.screen(x)), f"chunk {n} (unsplit)")
            e.set_chunk(0)
        finally:
            e.close()
        e1 = Engine.from_weights(w, None, det, precision=prec, debug_flags=L.DEBUG_NO_SMALL_SPLIT)
        try:                                                          # the one-workgroup kernels at every pass size
            p1, c1, m1, r1 = _tail(e1, x, feats)
            check(dict(pca=p1, dc=c1, dm=m1, **r1), "CS_DEBUG_NO_SMALL_SPLIT")
        finally:
            e1.close()
    print(f"\n{case.id} ({case.why}) arch {arch}: error / bar", report)


def test_swapped_detectors_give_swapped_outputs():
    """Distinct n_sv (17 and 129: nsv_pad 32 and 144), gamma (x1, x30) and rho: an engine with the two detectors exchanged
    reports the exchanged scores and flags bit for bit, in the pair-split launch, the per-detector launches and the unsplit
    kernels."""
    F = 544
    hw, ch, ne = D.arch_for_width(F)
    w = synth.random_cae(seed=5, hw=hw, channels=ch, n_enc=ne)
    x = _crops(hw, 300, seed=3)
    e0 = Engine.from_weights(w)
    try:
        train, feats = e0.encode(_crops(hw, 512, seed=4)), e0.encode(x)
    finally:
        e0.close()
    det = H.random_detector(F, 59, (17, 129), (1.0, 30.0), seed=9, cells=train)
    assert det.conservative.rho != det.moderate.rho
    swapped = copy.deepcopy(det)
    swapped.conservative, swapped.moderate = swapped.moderate, swapped.conservative
    for prec in PRECISIONS:
        for flags in (0, L.DEBUG_NO_SMALL_SPLIT):
            ea = Engine.from_weights(w, None, det, precision=prec, debug_flags=flags)
            eb = Engine.from_weights(w, None, swapped, precision=prec, debug_flags=flags)
            try:
                ra, rb = ea.screen(x), eb.screen(x)
                pca = ea.scaler_pca(feats)
                da, db = ea.svm_decision(pca), eb.svm_decision(pca)
            finally:
                ea.close()
                eb.close()
            for k in ("score", "pred"):
                assert np.array_equal(ra[f"cons_{k}"], rb[f"mod_{k}"]) and np.array_equal(ra[f"mod_{k}"], rb[f"cons_{k}"]), (prec, flags, k)
            assert np.array_equal(da[0], db[1]) and np.array_equal(da[1], db[0]), (prec, flags)
            for d, p in zip(da, (det.conservative, det.moderate)):
                tol = H.TOL_DEC_STAGE * np.abs(p.dual_coef).sum()
                assert np.abs(d[:40] - H.ocsvm_ref(p, pca[:40])).max() <= tol, (prec, flags)


def test_one_hot_pca_reproduces_the_scaled_feature_at_a_ragged_width():
    """F = 1344 (fpad 1536, 12 chunks: ragged ranges): with one-hot component rows and a zero mean projection the output IS
    the scaled feature, bit for bit with numpy's float32((x - center) / float64 scale), in both precisions, split and
    unsplit.  The columns read include the last feature and the first feature of every range."""
    F, C = D.ONE_HOT_F, D.ONE_HOT_C
    hw, ch, ne = D.arch_for_width(F)
    w = synth.random_cae(seed=6, hw=hw, channels=ch, n_enc=ne)
    rng = np.random.default_rng(77)
    det = H.random_detector(F, C, (20, 40), seed=3)
    det.scaler_center = rng.normal(0.3, 0.2, F).astype(np.float32)
    det.scaler_scale = np.exp(rng.normal(0.0, 2.0, F)) * (1.0 + 2.0 ** -30)
    det.scaler_scale[:8] = [1.0, 3.0, 0.1, 7.0, 1e-3, 1e3, 1.0 / 3.0, 2.0 ** -20]
    firsts = [b for b, e in D.pca_ranges(F) if b < e]
    must = sorted(set(firsts) | {F - 1, 1279, 1280, 1151} | set(range(8)))
    rest = rng.choice(np.setdiff1d(np.arange(F), must), C - len(must), replace=False)
    cols = np.concatenate([must, rest])
    comps = np.zeros((C, F), np.float32)
    comps[np.arange(C), cols] = 1.0
    det.pca_components, det.pca_mean, det.pca_mean_proj = comps, np.zeros(F, np.float32), np.zeros(C, np.float32)
    x = rng.normal(0.3, 1.0, (3001, F)).astype(np.float32)
    x[:50, :8] = det.scaler_center[:8]                        # exact zeros after centring
    x[50:60, F - 1] = det.scaler_center[F - 1]
    want = H.scaled_features(det, x)[:, cols]
    for prec in PRECISIONS:
        for flags in (0, L.DEBUG_NO_SMALL_SPLIT):
            e = Engine.from_weights(w, None, det, precision=prec, debug_flags=flags)
            try:
                got = e.scaler_pca(x)
            finally:
                e.close()
            assert np.array_equal(got, want), f"{prec} flags {flags}: {(got != want).sum()} of {got.size} scaled values differ"


def test_a_nan_feature_touches_only_its_cell():
    """One NaN feature (the last of a ragged width) in one cell: that cell's PCA row and decisions are NaN; every other
    cell, including the rest of its 16-cell tile, is bitwise unchanged."""
    F, C, n, bad = 2112, 101, 300, 77
    hw, ch, ne = D.arch_for_width(F)
    w = synth.random_cae(seed=8, hw=hw, channels=ch, n_enc=ne)
    rng = np.random.default_rng(8)
    f = np.maximum(rng.normal(0.2, 1.0, (n, F)), 0).astype(np.float32)
    det = H.random_detector(F, C, (40, 17), seed=11, cells=f[100:])
    fn = f.copy()
    fn[bad, F - 1] = np.nan
    ok = np.arange(n) != bad
    for prec in PRECISIONS:
        for flags in (0, L.DEBUG_NO_SMALL_SPLIT):
            e = Engine.from_weights(w, None, det, precision=prec, debug_flags=flags)
            try:
                pca, pn = e.scaler_pca(f), e.scaler_pca(fn)
                d, dn = e.svm_decision(pca), e.svm_decision(pn)
            finally:
                e.close()
            assert np.isnan(pn[bad]).all() and not np.isnan(pca).any(), (prec, flags)
            assert np.array_equal(pn[ok], pca[ok]), (prec, flags)
            for a, b in zip(d, dn):
                assert np.isnan(b[bad]) and np.array_equal(b[ok], a[ok]), (prec, flags)


def test_detector_refusals():
    """api.hip:777-786, 378-381: n_features other than the encoder's width, n_components outside 1..128, n_sv = 0."""
    F = 96
    hw, ch, ne = D.arch_for_width(F)
    w = synth.random_cae(seed=1, hw=hw, channels=ch, n_enc=ne)
    det = H.random_detector(F, 8, (5, 5), seed=1)
    wide = H.random_detector(F + 1, 8, (5, 5), seed=1)
    many = H.random_detector(F, 129, (5, 5), seed=1)
    none = copy.deepcopy(det)
    none.moderate.support_vectors, none.moderate.dual_coef = det.moderate.support_vectors[:0], det.moderate.dual_coef[:0]
    for d, rule, text in ((wide, "n_features", "n_features=97"), (many, "n_components", "n_components=129"),
                          (none, "n_sv", "n_sv=0")):
        assert D.accept(F, d.n_features, d.n_components, (d.conservative.n_sv, d.moderate.n_sv)) == rule
        with pytest.raises(L.CellScreenError) as ei:
            Engine.from_weights(w, None, d)
        assert ei.value.status == -1 and text in str(ei.value), str(ei.value)
    e = Engine.from_weights(w, None, det)
    e.close()


def test_device_fitted_detector_below_100_features_scores_like_its_sklearn_objects(tmp_path):
    """The real path at F = 96 < 100: fit_detector_device keeps C = F components, cs_screen with its DetectorParams
    agrees with the unpickled scikit-learn scaler / PCA / OneClassSVMs (improved_detection.py:134-142), as
    test_gpu_fit.py checks at F = 2048."""
    from cellscreen import detector_fit as df
    F = 96
    hw, ch, ne = D.arch_for_width(F)
    w = synth.random_cae(seed=42, hw=hw, channels=ch, n_enc=ne)
    e0 = Engine.from_weights(w)
    try:
        feats = e0.encode(synth.blob_crops(7, 1500, hw=hw))
        test = synth.blob_crops(8, 600, hw=hw)
        test[::5] = synth.synth_crops(9, 0, 120, hw=hw)
        tf = e0.encode(test)
    finally:
        e0.close()
    det, _ = df.fit_detector_device(feats, output_dir=str(tmp_path))
    assert det.n_components == F and det.conservative.n_sv > 0 and det.moderate.n_sv > 0
    with open(tmp_path / "scaler.pkl", "rb") as fh:
        scaler = pickle.load(fh)
    with open(tmp_path / "pca.pkl", "rb") as fh:
        pca = pickle.load(fh)
    red = pca.transform(scaler.transform(tf))
    for prec in PRECISIONS:
        e = Engine.from_weights(w, None, det, precision=prec)
        try:
            res = e.screen(test)
        finally:
            e.close()
        for key, name in (("cons", "conservative"), ("mod", "moderate")):
            with open(tmp_path / f"detector_{name}.pkl", "rb") as fh:
                dec = pickle.load(fh).decision_function(red)
            scale = max(1.0, np.abs(dec).max())
            err = np.abs(-res[f"{key}_score"] - dec).max()
            assert err <= 1e-4 * scale, f"{prec} {name}: {err:.3e}"
            ek = [k for k in D.call_kernels("screen", prec, F, len(test)) if k.startswith("ocsvm")][0]
            _note(ek, prec, "fit e2e 1e-4", err / (1e-4 * scale))


def test_zz_worst_error_per_instantiation():
    """Printed for the record: the largest error seen per (instantiation, precision, bar), as a fraction of the bar."""
    for (k, prec, bar), r in sorted(WORST.items()):
        print(f"{k:36s} {prec:10s} {bar:14s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
