"""The detector tail (csrc/detector.hip) on the CPU: the restatement in tests/detector_plans.py is self-consistent, the GPU
sweep's case list (test_gpu_detector_sweep.py) reaches every kernel instantiation and every partition class of the
fixed feature / support-vector ranges, and the float64 restatement of the tail that the sweep measures against
(tests/helpers.py) is pinned to the C oracle at the sweep's shapes and to scikit-learn at C = 1 and C = 128 on a width
that is not a multiple of 512.  No GPU needed."""
import numpy as np
import pytest

import detector_plans as D
import helpers as H
from oracle import oracle


def test_the_gpu_sweep_reaches_every_instantiation():
    seen = D.sweep_kernels()
    assert set(seen) == D.ALL_KERNELS, sorted(D.ALL_KERNELS - set(seen))
    for k, where in sorted(seen.items()):
        print(f"{k:36s} {where}")


def test_the_gpu_sweep_reaches_every_partition_class():
    cases = D.SWEEP_CASES
    nch = {D.pca_chunks(c.F) for c in cases}
    assert {D.pca_class(c.F) for c in cases} == {"empty", "even", "ragged"}
    assert 4 in nch and {12, 20} <= nch and any(k % 8 == 0 and k > 8 for k in nch)
    svm = {D.svm_class(s) for c in cases for s in c.n_sv}
    assert svm == {"1", "<8", "=8", ">8 ragged", ">8 even"}, svm
    assert {D.tiles(c.C) for c in cases} == set(range(1, 9))
    assert {c.C % 4 for c in cases} == {0, 1, 2, 3}
    assert {100, 101} <= {c.C for c in cases} and {D.ks(c.C) for c in cases} == {25, 32}
    assert 1 in {c.C for c in cases} and 128 in {c.C for c in cases}
    ragged = [c.n for c in cases if c.n % 16 and c.n % 64 and c.n % 256]
    assert any(n < D.DET_SPLIT_MAX_CELLS for n in ragged) and any(n > D.DET_SPLIT_MAX_CELLS for n in ragged)
    assert any(c.F % 512 for c in cases) and 1 in {c.n for c in cases}
    assert {g for c in cases for g in c.gamma_mult} >= {1e-3, 1.0, 30.0}
    assert any(c.C > c.F for c in cases)
    for c in cases:
        assert D.accept(c.F, c.F, c.C, c.n_sv) is None, c
        assert D.encoder_width(*D.arch_for_width(c.F)) == c.F, c


def test_the_restated_partitions():
    """The ranges tile [0, fpad) and [0, nblk) in ascending order; each pass of a call takes min(n, chunk) cells."""
    for F in (1, 32, 480, 512, 513, 1344, 2048, 2112, 2560, 32768):
        r = D.pca_ranges(F)
        assert r[0][0] == 0 and r[-1][1] == D.fpad(F) and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(e - b in (0, (D.pca_chunks(F) // 8) * D.PX_KC, (D.pca_chunks(F) // 8 + 1) * D.PX_KC) for b, e in r)
    assert [b for b, e in D.pca_ranges(1344)] == [0, 128, 384, 512, 768, 896, 1152, 1280]
    assert sum(1 for b, e in D.pca_ranges(480) if b == e) == 4
    for nsv in (1, 16, 17, 113, 128, 129, 256, 1000):
        r = D.svm_ranges(nsv)
        assert r[0][0] == 0 and r[-1][1] == D.nblk(nsv) and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert D.svm_ranges(1) == [(0, 0)] * 7 + [(0, 1)]
    assert D.passes(17391) == [16384, 1007] and D.passes(17391, chunk=17391) == [17391]
    assert D.passes(17391, "device", arch=D.arch_for_width(2112)) == [17391]
    assert D.call_kernels("screen", "split16", 100, 300) == ["scaler_pca_x3_kernel<true>", "pca_split_sum_kernel",
                                                            "ocsvm_mfma_kernel<25,true>[z=2]", "svm_split_sum_kernel[y=2]",
                                                            "finalize_kernel"]
    assert D.mfma_per_cell("fp32_exact", 2048, 100) == (224.0, 0.0) and D.mfma_per_cell("split16", 2048, 100) == (0.0, 168.0)


# ---- the float64 restatement against the C oracle and scikit-learn
PIN_SHAPES = sorted({(c.F, c.C) for c in D.SWEEP_CASES if c.F <= 4096})


@pytest.mark.parametrize("F,C", PIN_SHAPES, ids=[f"F{F}-C{C}" for F, C in PIN_SHAPES])
def test_float64_tail_equals_the_c_oracle(F, C):
    rng = np.random.default_rng(F + C)
    det = H.random_detector(F, C, (37, 129), (1.0, 30.0), seed=F * 7 + C)
    f = np.maximum(rng.normal(0.2, 1.0, (67, F)), 0).astype(np.float32)
    f[3] = det.scaler_center                                         # a cell that centres to exact zeros
    scaled, pca_o = oracle.scaler_pca(det, f, acc64=True)
    assert np.array_equal(H.scaled_features(det, f), scaled)
    ref = H.pca_ref(det, f)
    H.assert_close_scaled(pca_o, ref, 1e-6, "oracle pca (float32 result of a float64 sum)")
    p = det.moderate                                                 # a cell equal to a support vector at 100x the norm
    big = (np.asarray(ref[5], np.float64) * 100.0).astype(np.float32)
    p.support_vectors[0] = big
    x = pca_o.copy()
    x[5] = big
    for q in (det.conservative, p):
        got, pred = oracle.ocsvm_decision(q, x)
        want = H.ocsvm_ref(q, x)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(q.dual_coef).sum()
        assert np.array_equal(pred, np.where(want > 0, 1, -1))
    assert abs(H.ocsvm_ref(p, x[5:6])[0] - (p.dual_coef[0] - p.rho)) <= 1e-12 * np.abs(p.dual_coef).sum()


@pytest.mark.parametrize("C", [1, 128])
def test_float64_tail_equals_sklearn(C):
    """RobustScaler.transform bit for bit, PCA.transform (float32 GEMM) within TOL_STAGE / 10, OneClassSVM.decision_function
    (libsvm in float64) within 1e-11 sum|alpha|, at F = 544."""
    from cellscreen import detector_fit as df
    F = 544
    rng = np.random.default_rng(C)
    det = H.random_detector(F, C, (17, 129), (1.0, 1e-3), seed=C)
    f = np.maximum(rng.normal(0.3, 1.0, (301, F)), 0).astype(np.float32)
    sk_s = df._sklearn_scaler(det.scaler_center, det.scaler_scale)
    s = sk_s.transform(f)
    assert s.dtype == np.float32 and np.array_equal(s, H.scaled_features(det, f))
    ev = np.linspace(2.0, 1.0, C)
    sk_p = df._sklearn_pca(det.pca_components, det.pca_mean, ev, ev.sum() * 2, 1000)
    red = sk_p.transform(s)
    ref = H.pca_ref(det, f)
    H.assert_close_scaled(red, ref, H.TOL_STAGE / 10, "sklearn PCA.transform")
    for p in (det.conservative, det.moderate):
        o = df.sklearn_ocsvm(p.support_vectors, p.dual_coef, p.rho, p.gamma, 0.1)
        want = o.decision_function(red)
        got = H.ocsvm_ref(p, red)
        assert np.abs(got - want).max() <= 1e-11 * np.abs(p.dual_coef).sum()


def test_random_detector_means_something():
    """Positive coefficients, gamma = mult / (C var), unit scales for the constant columns, and flags that split at the
    median on the cells the detector was built from."""
    cells = np.maximum(np.random.default_rng(1).normal(0.2, 1.0, (400, 1344)), 0).astype(np.float32)
    det = H.random_detector(1344, 18, (7, 100), (30.0, 1.0), seed=5, cells=cells)
    red = H.pca_ref(det, cells).astype(np.float32)
    var = red.astype(np.float64).var()
    for p, m in ((det.conservative, 30.0), (det.moderate, 1.0)):
        assert (p.dual_coef > 0).all() and p.support_vectors.shape[1] == 18
        assert p.gamma == pytest.approx(m / (18 * var))
        assert abs((H.ocsvm_ref(p, red) > 0).mean() - 0.5) <= 0.01
    assert (det.scaler_scale == 1.0).sum() >= 1344 // 64
