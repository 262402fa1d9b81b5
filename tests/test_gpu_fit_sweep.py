"""The detector fit (csrc/fit.hip: cs_fit_scaler, cs_fit_pca_moments, cs_fit_project, cs_fit_ocsvm) at the shapes where
such kernels go wrong -- the case lists of tests/fit_plans.py, whose CPU test proves that they reach every slice
boundary, tile count, loop trip and acceptance rule the code has -- each against the plain reference of the same
operation:

* scaler: bit for bit RobustScaler().fit.
* PCA moments, exact family: integer-valued rows whose scatter matrix is exact in fp64 in any summation order, so
  np.array_equal, no tolerance: an indexing error cannot hide.
* PCA moments, general family: mean_ bit for bit; the scatter matrix entry by entry within 2 n 2^-53 (|xc|^T |xc|)
  of the float64 product (fit_plans.scatter_bound has the derivation; no measured constant).
* projection: helpers.pca_ref under TOL_STAGE, the bar the same kernel has in the detector sweep; one-hot components
  reproduce the scaled features bit for bit.
* one-class SVM: libsvm's own trajectory for points in general position (test_gpu_fit's bar), the solver's tolerance for
  degenerate data, libsvm's iterates at max_iter next to the host's launch batch, and a refusal where scikit-learn
  refuses (nu = 1).

One Fitter serves the whole file, so every device buffer is asked to grow, shrink and grow again; the last test repeats
cases on a fresh handle and wants the same bits."""
import types
import warnings

import numpy as np
import pytest

import fit_plans as P
import helpers as H
from cellscreen import detector_fit as df

pytestmark = pytest.mark.gpu

WALK = {}            # (stage, case) -> what the shared handle returned, for the cases fit_plans.REPLAY repeats


@pytest.fixture(scope="module")
def fitter():
    f = df.Fitter(0)
    yield f
    f.close()


def _same(a, b, what):
    """Bit for bit."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def _keep(stage, case, result):
    if case in P.REPLAY[stage]:
        WALK[(stage, case)] = result
    return result


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _det(center, scale, comps=None, mean_proj=None):
    return types.SimpleNamespace(scaler_center=center, scaler_scale=scale, pca_components=comps, pca_mean_proj=mean_proj)


# ---------------------------------------------------------------- what each stage runs (also on the fresh handle)
def _run_scaler(f, case):
    center, scale = f.scaler(P.scaler_data(*case))
    return dict(center=center, scale=scale)


def _run_moments_exact(f, case):
    n, F = case
    mean, scatter = f.pca_moments(P.exact_moment_rows(n, F), np.zeros(F, np.float32), np.ones(F))
    return dict(mean=mean, scatter=scatter)


def _general_inputs(case):
    from sklearn.preprocessing import RobustScaler
    n, F = case
    x = P.encoder_like_features(n, F, seed=n + F)
    sc = RobustScaler().fit(x)
    return x, sc


def _run_moments_general(f, case):
    x, sc = _general_inputs(case)
    mean, scatter = f.pca_moments(x, sc.center_, sc.scale_)
    return dict(mean=mean, scatter=scatter)


def _run_project(f, case):
    return dict(out=f.project(*P.project_data(*case)))


def _gamma_scale(x):
    """sklearn/svm/_base.py:244-247, gamma='scale'."""
    v = x.var()
    return 1.0 / (x.shape[1] * v) if v != 0 else 1.0


def _run_svm(f, case, as_float32=None):
    as_float32 = P.svm_variants(case)[0] if as_float32 is None else as_float32
    x = P.svm_data(case, as_float32)
    gamma = _gamma_scale(x) if case.gamma is None else case.gamma
    got = f.ocsvm(x, gamma, case.nu, max_iter=case.max_iter)
    return {k: np.asarray(v) for k, v in got.items()}


RUN = {"scaler": _run_scaler, "moments_exact": _run_moments_exact, "moments_general": _run_moments_general,
       "project": _run_project, "svm": _run_svm}


# ---------------------------------------------------------------- RobustScaler.fit
@pytest.mark.parametrize("case", P.SCALER_CASES, ids=_ids(P.SCALER_CASES))
def test_scaler_sweep(fitter, case):
    from sklearn.preprocessing import RobustScaler
    want = RobustScaler().fit(P.scaler_data(*case))
    got = _keep("scaler", case, _run_scaler(fitter, case))
    assert got["center"].dtype == want.center_.dtype == np.float32 and got["scale"].dtype == want.scale_.dtype == np.float64
    assert np.array_equal(got["center"], want.center_), P.scaler_class(*case)
    assert np.array_equal(got["scale"], want.scale_), P.scaler_class(*case)


@pytest.mark.parametrize("name,column", P.SCALER_VALUE_CASES, ids=[c[0] for c in P.SCALER_VALUE_CASES])
def test_scaler_at_the_ends_of_the_float_range(fitter, name, column):
    """+-FLT_MAX next to each other in the order (their float32 difference overflows inside numpy's interpolation), a
    denormal, both zeros.  scikit-learn returns on each (test_fit_envelope_cpu.py); what it returns is the expectation."""
    from sklearn.preprocessing import RobustScaler
    x = np.array(column, np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = RobustScaler().fit(x)
    center, scale = fitter.scaler(x)
    print(name, center, scale, want.center_, want.scale_)
    assert np.array_equal(center, want.center_, equal_nan=True)
    assert np.array_equal(scale, want.scale_, equal_nan=True)


def test_scaler_refuses_non_finite_features(fitter):
    """RobustScaler.fit refuses +-inf; the device refuses NaN as well (nanmedian semantics are not implemented)."""
    for name, v, sklearn_refuses in P.SCALER_NON_FINITE:
        for shape, at in (((10, 8), (3, 2)), ((65, 33), (64, 32)), ((1, 1), (0, 0))):
            x = np.zeros(shape, np.float32)
            x[at] = v
            with pytest.raises(RuntimeError, match="NaN"):
                fitter.scaler(x)
    case = P.SCALER_CASES[3]                                  # the handle stays usable
    _same(_run_scaler(fitter, case), _run_scaler(fitter, case), "scaler after a refusal")
    from sklearn.preprocessing import RobustScaler
    want = RobustScaler().fit(P.scaler_data(*case))
    assert np.array_equal(_run_scaler(fitter, case)["center"], want.center_)


# ---------------------------------------------------------------- PCA moments
def _where(scatter, ref):
    bad = np.argwhere(scatter != ref)
    if not len(bad):
        return "equal"
    a, b = bad[0]
    return f"{len(bad)} entries differ, first at [{a}][{b}] (tile {a // P.COV_T}, {b // P.COV_T}): {scatter[a, b]!r} vs {ref[a, b]!r}"


@pytest.mark.parametrize("case", P.EXACT_MOMENT_CASES, ids=_ids(P.EXACT_MOMENT_CASES))
def test_moments_exact_family(fitter, case):
    n, F = case
    x64 = P.exact_moment_rows(n, F).astype(np.float64)
    ref = x64.T @ x64
    got = _keep("moments_exact", case, _run_moments_exact(fitter, case))
    assert got["mean"].dtype == np.float32 and not got["mean"].any()
    assert np.array_equal(got["scatter"], ref), (P.moments_class(n, F), P.slices(n, F), _where(got["scatter"], ref))
    assert np.array_equal(got["scatter"], got["scatter"].T)


@pytest.mark.parametrize("case", P.EXACT_SHIFTED_CASES, ids=_ids(P.EXACT_SHIFTED_CASES))
def test_moments_exact_family_through_the_scaler(fitter, case):
    """The same rows as x * scale + center with a power-of-two scale and an integer centre: exact in float32, and
    (x' - center) / scale gives x back bit for bit."""
    n, F = case
    x64 = P.exact_moment_rows(n, F).astype(np.float64)
    center, scale = P.exact_shift(F)
    assert center.any() and (scale != 1).any()
    mean, scatter = fitter.pca_moments((x64 * scale + center).astype(np.float32), center, scale)
    ref = x64.T @ x64
    assert not mean.any()
    assert np.array_equal(scatter, ref), _where(scatter, ref)
    assert np.array_equal(scatter, scatter.T)


@pytest.mark.parametrize("case", P.GENERAL_MOMENT_CASES, ids=_ids(P.GENERAL_MOMENT_CASES))
def test_moments_general_family(fitter, case):
    import torch
    n, F = case
    x, sc = _general_inputs(case)
    xs = H.scaled_features(_det(sc.center_, sc.scale_), x)
    assert np.array_equal(xs, sc.transform(x))
    got = _keep("moments_general", case, _run_moments_general(fitter, case))
    mean_ref = xs.mean(axis=0)
    assert mean_ref.dtype == np.float32 and np.array_equal(got["mean"], mean_ref)
    xc = (xs - mean_ref).astype(np.float64)                 # PCA centres in float32
    ref = xc.T @ xc
    bound = P.scatter_bound(xc, n)
    err = np.abs(got["scatter"] - ref)
    live = bound > 0
    print(f"n {n} F {F}: max |err| / bound = {(err[live] / bound[live]).max() if live.any() else 0.0:.3g}")
    assert (err <= bound).all(), (P.moments_class(n, F), float((err - bound).max()))
    assert np.array_equal(got["scatter"], got["scatter"].T)
    assert not got["scatter"][:4].any() and not got["scatter"][:, :4].any()          # dead columns: exact zeros
    if n == 1:
        assert not got["scatter"].any()
    mean_d, scatter_d = fitter.pca_moments(torch.from_numpy(x).cuda(), sc.center_, sc.scale_)
    _same(dict(mean=mean_d, scatter=scatter_d), got, "device-resident features")


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("case", P.PROJECT_CASES, ids=_ids(P.PROJECT_CASES))
def test_project_sweep(fitter, case):
    n, F, C = case
    f, center, scale, comps, mean_proj = P.project_data(n, F, C)
    ref = H.pca_ref(_det(center, scale, comps, mean_proj), f)
    got = _keep("project", case, _run_project(fitter, case))["out"]
    assert got.dtype == np.float32 and got.shape == (n, C)
    rel = H.assert_close_scaled(got, ref, H.TOL_STAGE, f"project {case} {P.project_class(*case)}")
    print(f"n {n} F {F} C {C}: max err / scale = {rel:.3g}")
    # mean_proj is subtracted once, in float32, after the sum
    plain = fitter.project(f, center, scale, comps, np.zeros(C, np.float32))
    assert np.array_equal(got, plain - mean_proj)
    assert mean_proj.all() and not np.array_equal(got, plain)


def test_project_one_hot_components_give_the_scaled_features(fitter):
    n, F, C = P.ONE_HOT_CASE
    f, center, scale, _, _ = P.project_data(n, F, C)
    picks = np.array([0, F - 1, 255, 253, 1, 128, 31, 32, 33, 63, 64, 127, 129, 200, 254, 17, 100][:C])
    assert len(set(picks)) == C == len(picks)
    comps = np.zeros((C, F), np.float32)
    comps[np.arange(C), picks] = 1.0
    out = fitter.project(f, center, scale, comps, np.zeros(C, np.float32))
    want = H.scaled_features(_det(center, scale), f)[:, picks]
    assert out.tobytes() == want.tobytes()


def test_project_refusals_and_device_memory(fitter):
    import torch
    for C in (0, 129):
        with pytest.raises(RuntimeError, match="n_components"):
            fitter.project(np.zeros((4, 8), np.float32), np.zeros(8, np.float32), np.ones(8), np.zeros((C, 8), np.float32),
                           np.zeros(C, np.float32))
    case = P.PROJECT_CASES[4]
    f, center, scale, comps, mean_proj = P.project_data(*case)
    host = fitter.project(f, center, scale, comps, mean_proj)
    dev = fitter.project(torch.from_numpy(f).cuda(), center, scale, comps, mean_proj)
    assert host.tobytes() == dev.tobytes()


# ---------------------------------------------------------------- one-class SVM
def _libsvm(case, x):
    from sklearn.svm import OneClassSVM
    est = OneClassSVM(kernel="rbf", gamma="scale" if case.gamma is None else case.gamma, nu=case.nu, max_iter=case.max_iter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(x)
    alpha = np.zeros(len(x))
    alpha[est.support_] = est.dual_coef_.ravel()
    if case.gamma is None:
        assert est._gamma == _gamma_scale(x)
    return est, alpha


def _follows_libsvm(fitter, case, as_float32):
    """The bar of test_gpu_fit.test_ocsvm_fit_follows_libsvm."""
    x = P.svm_data(case, as_float32)
    want, alpha = _libsvm(case, x)
    got = _run_svm(fitter, case, as_float32)
    print(f"{case.id} f32={as_float32}: n_iter {got['n_iter']} vs libsvm {want.n_iter_}; max |d alpha| "
          f"{np.abs(got['alpha'] - alpha).max():.3g}; rho {float(got['rho'])!r} vs {-want.intercept_[0]!r}; {P.svm_class(case)}")
    assert got["status"] == 0 and want.fit_status_ == 0
    assert got["n_iter"] == want.n_iter_
    assert np.abs(got["alpha"] - alpha).max() <= 1e-9
    assert np.array_equal(np.flatnonzero(got["alpha"] > 0), want.support_)
    assert abs(got["rho"] + want.intercept_[0]) <= 1e-9 * max(1.0, abs(want.intercept_[0]))
    assert abs(got["alpha"].sum() - case.nu * case.n) <= 1e-9 * case.n
    return got


SVM_GENERAL_RUNS = [(c, f) for c in P.SVM_GENERAL for f in P.svm_variants(c)]


@pytest.mark.parametrize("case,as_float32", SVM_GENERAL_RUNS, ids=[f"{c.id}-{'f32' if f else 'f64'}" for c, f in SVM_GENERAL_RUNS])
def test_ocsvm_general_position_follows_libsvm(fitter, case, as_float32):
    """The last case, 65,537 points, is the only one with 257 workgroups: the loops over the per-workgroup partials
    (smo_row_i_kernel, smo_update_kernel) take their second trip, and workgroup 256 holds one point, which ends as a
    support vector.  fit_plans.SVM_GENERAL says why its seed is the recipe's plus 3."""
    got = _follows_libsvm(fitter, case, as_float32)
    if as_float32 == P.svm_variants(case)[0]:
        _keep("svm", case, got)


@pytest.mark.parametrize("case", P.SVM_DEGENERATE, ids=[c.id for c in P.SVM_DEGENERATE])
def test_ocsvm_degenerate_cases(fitter, case):
    """The bar of test_gpu_fit.test_ocsvm_fit_degenerate_data_agrees_to_solver_tolerance; a single point and gamma = 0
    (every kernel value 1) both stop before the first iteration, in libsvm and here."""
    x = P.svm_data(case, False)
    want, alpha = _libsvm(case, x)
    got = _run_svm(fitter, case)
    gamma = want._gamma
    n, d, nu, eps = case.n, case.d, case.nu, df.SVM_TOL
    assert got["status"] == 0 and got["n_iter"] == want.n_iter_ == 0
    assert abs(got["alpha"].sum() - nu * n) <= 1e-9 * n and got["alpha"].min() >= 0 and got["alpha"].max() <= 1
    assert abs(got["rho"] + want.intercept_[0]) <= 2 * eps
    if n == 1:
        assert got["rho"] == 0.5 == -want.intercept_[0]
    rebuilt = df.sklearn_ocsvm(x, got["alpha"], float(got["rho"]), gamma, nu, int(got["n_iter"]))
    rng = np.random.default_rng(n + d)
    y = np.concatenate([x[:200], rng.normal(size=(100, d)) * 2])
    assert np.abs(rebuilt.decision_function(y) - want.decision_function(y)).max() <= 4 * eps
    k = np.exp(-gamma * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    obj_ref = 0.5 * alpha @ k @ alpha
    assert abs(got["obj"] - obj_ref) <= eps * max(1.0, abs(obj_ref))


@pytest.mark.parametrize("case", P.SVM_MAX_ITER, ids=[c.id for c in P.SVM_MAX_ITER])
def test_ocsvm_max_iter_next_to_the_launch_batch(fitter, case):
    """test_gpu_fit.test_ocsvm_max_iter_stops_like_libsvm's data and assertions, stopping just below, on and just above
    the 256 iterations the host enqueues between two polls."""
    x = P.svm_data(case, False)
    want, alpha = _libsvm(case, x)
    got = _run_svm(fitter, case)
    assert got["status"] == 1 and got["n_iter"] == case.max_iter == want.n_iter_
    assert np.abs(got["alpha"] - alpha).max() <= 1e-9
    assert abs(got["rho"] + want.intercept_[0]) <= 1e-9 * abs(want.intercept_[0])


@pytest.mark.parametrize("case", P.SVM_REFUSED, ids=[c.id for c in P.SVM_REFUSED])
def test_ocsvm_nu_one_is_refused_as_sklearn_refuses_it(fitter, case):
    """nu = 1 starts every alpha at its bound; libsvm stops at once with rho = +inf and scikit-learn raises.  The device
    must return an error, not a non-finite rho, and the handle must go on working."""
    from sklearn.svm import OneClassSVM
    x = P.svm_data(case, False)
    with pytest.raises(ValueError, match="not finite"):
        OneClassSVM(kernel="rbf", gamma="scale", nu=case.nu).fit(x)
    with pytest.raises(RuntimeError, match="rho is not finite"):
        fitter.ocsvm(x, _gamma_scale(x), case.nu)
    _follows_libsvm(fitter, P.SVM_GENERAL[1], False)


# ---------------------------------------------------------------- refusals
def _call_refused(f, entry, kw):
    n, F = kw.get("n"), kw.get("F")
    if entry == "scaler":
        x = np.zeros((n, F), np.float32)
        if kw.get("non_finite"):
            x[3, 2] = np.inf
        return f.scaler(x)
    if entry == "moments":
        return f.pca_moments(np.zeros((n, F), np.float32), np.zeros(F, np.float32), np.ones(F))
    if entry == "project":
        C = kw["C"]
        return f.project(np.zeros((n, F), np.float32), np.zeros(F, np.float32), np.ones(F), np.zeros((C, F), np.float32),
                         np.zeros(C, np.float32))
    x = np.random.default_rng(0).normal(size=(n, kw["D"]))
    if not kw.get("finite", True):
        x[4, 1] = np.inf
    return f.ocsvm(x, kw.get("gamma", 1.0), kw["nu"], tol=kw.get("eps", df.SVM_TOL))


def test_every_acceptance_rule_refuses(fitter):
    ran = 0
    for entry, kw, rule, runnable in P.REFUSED:
        if not runnable:                                      # a row count past 2^28 / 2^30 cannot be allocated to be refused
            continue
        with pytest.raises(RuntimeError):
            _call_refused(fitter, entry, kw)
        ran += 1
    assert ran >= sum(len(v) for v in P.RULES.values())
    case = P.SCALER_CASES[2]
    _same(_run_scaler(fitter, case), _run_scaler(fitter, case), "after the refusals")


# ---------------------------------------------------------------- one handle, many sizes
def test_a_fresh_handle_gives_the_same_bits(fitter):
    """The first case of every stage and one from the middle of its list, on a handle that has seen nothing larger:
    stale contents of part, keys or xT left by a larger call would show as a difference."""
    with df.Fitter(0) as fresh:
        for stage, cases in P.REPLAY.items():
            for case in cases:
                walked = WALK.get((stage, case))
                if walked is None:                            # this test run on its own
                    walked = RUN[stage](fitter, case)
                _same(RUN[stage](fresh, case), walked, f"{stage} {case}")
