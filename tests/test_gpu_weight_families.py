"""The inference kernels on weights as a trained checkpoint holds them (tests/weight_families.py): a non-zero bias in every
conv, dead and never-clipped filters, BN gains of either sign over orders of magnitude, gamma = 0, variance 0 -- where
every other GPU test of the inference path draws synth.random_cae's zero biases and gains near 1.  Everything against
oracle.cae_forward(acc64=True) at the standing bars of tests/helpers.py, in both precisions; plus each channel against its
own magnitude budget, and the fp16 split's envelope for a channel far below its cell's maximum.
Small cell counts: the persistent loops and ragged grids are test_gpu_parity.py's and test_gpu_generic_sweep.py's."""
import numpy as np
import pytest

import generic_plans as G
import helpers as H
import test_gpu_generic_sweep as S
import weight_families as WF
from cellscreen import _lib as L
from cellscreen import synth
from cellscreen.engine import Engine
from oracle import oracle

pytestmark = pytest.mark.gpu

PRECISIONS = ["split16", "fp32_exact"]
K_INSIDE = (6, 12)          # compensated channels inside the split's envelope (the issue's derivation: up to k = 17)
K_OUTSIDE = 24              # outside it: measured, printed, not asserted for split16

_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _weights(k=0):
    w = _memo("w", lambda: WF.trained_like(WF.REF_SEED))
    return w if k == 0 else _memo(("w", k), lambda: WF.compensated(w, k, seed=k))


def _x():
    return _memo("x", lambda: WF.edge_crops((64, 64), 12))


def _ref(k=0):
    """The oracle on the 12 crops, computed once per weight set and never written to."""
    return _memo(("ref", k), lambda: oracle.cae_forward(_weights(k), _x(), acc64=True, layers=True))


@pytest.fixture(scope="module")
def det(golden_det):
    return H.det_from_golden(golden_det)


def _run(det, prec, k=0, flags=0):
    """Every entry point of the reference graph once per (weights, precision, debug flags)."""
    def make():
        x = _x()
        e = Engine.from_weights(_weights(k), None, det, precision=prec, debug_flags=flags)
        try:
            assert e.precision == prec and e.info.debug_flags == flags
            r = dict(layers=[e.layer_output(x, l) for l in range(7)], features=e.encode(x, which=0))
            r["recon"], r["mse_two"], r["mae_two"] = e.reconstruct(x)                   # conv6 and conv7 as two kernels
            _, r["mse_fused"], r["mae_fused"] = e.reconstruct(x, want_recon=False)      # conv6 + conv7 + errors as one
            s = e.screen(x)
            r["mse_screen"], r["mae_screen"] = s["mse"], s["mae"]
        finally:
            e.close()
        return r
    return _memo(("run", prec, k, flags), make)


def _check_standing(r, ref, what):
    """The standing bars: 1e-5 of the range per layer, TOL_FEATURES, TOL_RECON, TOL_ERR_REL."""
    worst = {}
    for l in range(6):
        worst[l] = H.assert_close_scaled(r["layers"][l], ref["layers"][l], 1e-5, f"{what}: layer {l}")
    got7 = r["layers"][6].reshape(ref["recon"].shape).astype(np.float64)
    assert np.abs(got7 - ref["recon"]).max() <= H.TOL_RECON, f"{what}: layer 6"
    H.assert_close_scaled(r["features"], ref["features"], H.TOL_FEATURES, f"{what}: features")
    assert np.abs(r["recon"].astype(np.float64) - ref["recon"]).max() <= H.TOL_RECON, f"{what}: reconstruction"
    for path in ("two", "fused", "screen"):
        H.assert_rel(r[f"mse_{path}"], ref["mse"], H.TOL_ERR_REL, f"{what}: mse ({path})")
        H.assert_rel(r[f"mae_{path}"], ref["mae"], H.TOL_ERR_REL, f"{what}: mae ({path})")
    return worst


# ---------------------------------------------------------------- a. the reference graph on trained_like weights
@pytest.mark.parametrize("prec", PRECISIONS)
def test_reference_graph_on_trained_like_weights(det, prec):
    """All seven layer outputs, the features, the reconstruction from the two-kernel conv6 / conv7, the error sums from those,
    from the fused conv6 + conv7 kernel and from cs_screen."""
    worst = _check_standing(_run(det, prec), _ref(), prec)
    print(f"\n{prec}: max err / range per layer", " ".join(f"{worst[l]:.2e}" for l in range(6)))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_unfused_forms_on_trained_like_weights(det, prec):
    """CS_DEBUG_NO_FUSE45: a4, a5 and the reconstruction bit-identical to the fused conv4 + conv5 (the standing claim of
    test_fused_conv4_conv5_equals_the_two_kernels).  NO_FUSE12: p2 of the two-kernel path inside the layer bar, and other
    bits than the fused kernel's.  NO_FUSE67: the error sums within the standing 1e-6 of the fused kernel's."""
    base, ref = _run(det, prec), _ref()
    r45 = _run(det, prec, flags=L.DEBUG_NO_FUSE45)
    assert np.array_equal(r45["layers"][3], base["layers"][3]) and np.array_equal(r45["layers"][4], base["layers"][4])
    for key in ("recon", "mse_two", "mae_two", "mse_fused", "mae_fused"):
        assert np.array_equal(r45[key], base[key]), key
    r12 = _run(det, prec, flags=L.DEBUG_NO_FUSE12)
    H.assert_close_scaled(r12["layers"][1], ref["layers"][1], 1e-5, "p2 of the two-kernel conv1, conv2")
    assert not np.array_equal(r12["layers"][1], base["layers"][1]), "the debug flag did not select another kernel"
    _check_standing(r12, ref, f"{prec}, NO_FUSE12")
    r67 = _run(det, prec, flags=L.DEBUG_NO_FUSE67)
    for key in ("mse", "mae"):
        for path in ("fused", "screen"):
            got, want = r67[f"{key}_{path}"], base[f"{key}_{path}"]
            assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (key, path)
    _check_standing(r67, ref, f"{prec}, NO_FUSE67")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_separate_encoder_set_on_trained_like_weights(det, prec):
    """Features from the encoder set (perturbed_encoder of a second draw), errors from the autoencoder set."""
    w, x = _weights(), _x()
    enc = synth.perturbed_encoder(WF.trained_like(WF.REF_SEED + 1))
    e = Engine.from_weights(w, enc, det, precision=prec)
    try:
        assert e.info.shared_encoder == 0
        f_enc, f_ae, s = e.encode(x, which=1), e.encode(x, which=0), e.screen(x)
    finally:
        e.close()
    fe = oracle.cae_forward(enc, x, acc64=True, want=("features",))["features"]
    H.assert_close_scaled(f_enc, fe, H.TOL_FEATURES, "features (encoder set)")
    H.assert_close_scaled(f_ae, _ref()["features"], H.TOL_FEATURES, "features (autoencoder half)")
    assert np.abs(fe - _ref()["features"]).max() > 1e-2 * np.abs(fe).max(), "the two sets must tell apart"
    H.assert_rel(s["mse"], _ref()["mse"], H.TOL_ERR_REL, "mse (autoencoder set)")
    H.assert_rel(s["mae"], _ref()["mae"], H.TOL_ERR_REL, "mae (autoencoder set)")


# ---------------------------------------------------------------- b. each channel against its own magnitude budget
def _per_channel_ratios(r, w, ref):
    """Per hidden layer: max over channels of max|got - ref| / B_c (WF.channel_budget from the oracle's input to the layer)."""
    prev, out = _x(), []
    for l in range(6):
        B = WF.channel_budget(w, l, prev)
        err = np.abs(r["layers"][l].astype(np.float64) - ref["layers"][l]).reshape(-1, len(B)).max(axis=0)
        out.append((float((err / B).max()), int((err / B).argmax())))
        prev = ref["layers"][l]
    return out


@pytest.mark.parametrize("prec", PRECISIONS)
def test_every_channel_within_its_own_budget(det, prec):
    """The whole-tensor bar is relative to the largest channel and blind to one 2^-8 below it.  Here every channel c of every
    hidden layer: |got - ref| <= WF.PER_CHANNEL_TOL * B_c, B_c = |bn_scale_c| max_pixels(sum |a||w| + |b_c|) + |bn_shift_c|.
    Plain float32 numpy sits at 1.0e-7 .. 1.6e-7 of B_c on every layer (test_weight_families_cpu.py), so the bar is 1e-5
    on all of them."""
    ratios = _per_channel_ratios(_run(det, prec), _weights(), _ref())
    print(f"\n{prec}: worst |err| / B_c per layer", " ".join(f"{v:.2e} (ch {c})" for v, c in ratios))
    for l, (v, c) in enumerate(ratios):
        assert v <= WF.PER_CHANNEL_TOL, f"{prec} layer {l}: channel {c} off by {v:.3e} of its budget"


# ---------------------------------------------------------------- c, d. channels 2^-k below their cell's maximum
def _same_bits_as_uncompensated(r, base, k):
    w = _weights()
    for l in range(6):
        assert np.array_equal(WF.uncompensate(r["layers"][l], l, w, k, seed=k), base["layers"][l]), f"k {k}: layer {l}"
    assert np.array_equal(r["layers"][6], base["layers"][6]), f"k {k}: layer 6"
    f = WF.uncompensate(r["features"].reshape(-1, 8, 8, 32), 2, w, k, seed=k).reshape(r["features"].shape)
    assert np.array_equal(f, base["features"]), f"k {k}: features"
    for key in ("recon", "mse_two", "mae_two", "mse_fused", "mae_fused", "mse_screen", "mae_screen"):
        assert np.array_equal(r[key], base[key]), f"k {k}: {key}"


@pytest.mark.parametrize("k", K_INSIDE)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_compensated_channels_inside_the_envelope(det, prec, k):
    """compensated(w, k): a third of every layer's channels 2^-k below their neighbours, the next conv's weights for them 2^k
    above the rest.  A scaled value 2^-k below a maximum in [2^14, 2^15) has a low term whose quantum, 2^(14-k-21), is no
    smaller than fp16's 2^-24 up to k = 17, so k = 6 and 12 are inside the split's envelope: the standing bars against the
    oracle of the compensated weights.  On the fp32 path every operation commutes with an exact power of two: bit-identical
    to the uncompensated weights."""
    r = _run(det, prec, k=k)
    worst = _check_standing(r, _ref(k), f"{prec}, k {k}")
    print(f"\n{prec}, k {k}: max err / range per layer", " ".join(f"{worst[l]:.2e}" for l in range(6)))
    if prec == "fp32_exact":
        _same_bits_as_uncompensated(r, _run(det, prec), k)


def test_compensated_channels_outside_the_envelope(det):
    """k = 24, beyond the k = 17 of the derivation: the fp32 path is still bit-identical to the uncompensated weights and
    within the standing bars; the split path must stay finite, and its error per layer is printed (DESIGN.md section 3h
    holds the table), not asserted."""
    k = K_OUTSIDE
    r = _run(det, "fp32_exact", k=k)
    _check_standing(r, _ref(k), f"fp32_exact, k {k}")
    _same_bits_as_uncompensated(r, _run(det, "fp32_exact"), k)
    s, ref = _run(det, "split16", k=k), _ref(k)
    for key, v in s.items():
        assert all(np.isfinite(a).all() for a in (v if key == "layers" else [v])), key
    rows = []
    for l in range(6):
        # relative to the layer's range at w's scale: the moved channels brought back, as the next layer reads them
        got = WF.uncompensate(s["layers"][l], l, _weights(), k, seed=k).astype(np.float64)
        want = WF.uncompensate(ref["layers"][l], l, _weights(), k, seed=k).astype(np.float64)
        rows.append(np.abs(got - want).max() / np.abs(want).max())
    rows.append(np.abs(s["recon"] - ref["recon"]).max())
    rel = lambda a, b: float((np.abs(a - b) / np.abs(b)).max())
    print(f"\nsplit16, k {k}: max err / range per layer " + " ".join(f"{v:.2e}" for v in rows[:6]) +
          f"; reconstruction max abs {rows[6]:.2e}; mse rel {rel(s['mse_fused'], ref['mse']):.2e}, mae rel {rel(s['mae_fused'], ref['mae']):.2e}")


# ---------------------------------------------------------------- e. the run-time-shaped kernels
WORST = {}


def _generic(case, k):
    hw, ch, ne = case
    w = WF.trained_like(100 + hw[0] + len(ch), hw, ch, ne)
    if k:
        w = WF.compensated(w, k, seed=k)
    x = S._crops(hw, 3, seed=hw[1] + len(ch))
    ref = oracle.cae_forward(w, x, acc64=True, layers=True)
    a = G.describe_arch(hw, ch, ne)
    for prec in PRECISIONS:
        plans = G.plan(hw, ch, ne, prec)
        e = Engine.from_weights(w, precision=prec)
        try:
            S._check_profile(e, plans, a)
            for lp in plans:
                l = lp.layer
                got = e.layer_output(x, l)
                tol = H.TOL_FEATURES if l < a.n_conv - 1 else H.TOL_RECON
                r = H.assert_close_scaled(got, ref["layers"][l].reshape(got.shape), tol, f"{prec} layer {l} ({lp.kernel})")
                WORST[(lp.kernel, prec)] = max(WORST.get((lp.kernel, prec), 0.0), r / tol)
            rec, mse, mae = e.reconstruct(x)
            assert np.abs(rec - ref["recon"].reshape(rec.shape)).max() <= H.TOL_RECON, prec
            H.assert_rel(mse, ref["mse"], H.TOL_ERR_REL, f"{prec} mse")
            H.assert_rel(mae, ref["mae"], H.TOL_ERR_REL, f"{prec} mae")
            H.assert_close_scaled(e.encode(x), ref["features"].reshape(len(x), -1), H.TOL_FEATURES, f"{prec} features")
        finally:
            e.close()


@pytest.mark.parametrize("case", WF.GENERIC_CASES, ids=[S._id(c + (None,)) for c in WF.GENERIC_CASES])
def test_generic_kernels_on_trained_like_weights(case):
    """Every instantiation of the run-time-shaped kernels (WF.GENERIC_CASES: the covering subset of the sweep's cases),
    3 cells, both precisions: every layer, the reconstruction, mse / mae and the features at the sweep's bars."""
    _generic(case, 0)


@pytest.mark.parametrize("case", WF.GENERIC_COMPENSATED, ids=[S._id(c + (None,)) for c in WF.GENERIC_COMPENSATED])
def test_generic_split_kernels_on_compensated_channels(case):
    """compensated(k = 12) where conv_generic_x3_kernel (plain and folded) and conv_last_x3_kernel<32>, <64> run."""
    _generic(case, 12)


def test_zz_worst_error_per_generic_instantiation():
    for (kern, prec), r in sorted(WORST.items()):
        print(f"{kern:40s} {prec:10s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())


# ---------------------------------------------------------------- f. the trainer's inference epilogues
@pytest.mark.parametrize("shape", [((64, 64), (32, 64, 32, 32, 64, 32, 1), 3), ((64, 128), (8, 16, 32, 32, 16, 8, 1), 3)],
                         ids=["reference", "64x128-8-16-32-32-16-8-1"])
def test_trainer_evaluate_on_trained_like_moving_statistics(shape):
    """Trainer.evaluate runs the inference graph on the moving statistics with the trainer's own epilogues: loss and MAE
    against the means of the oracle's per-cell mse / mae."""
    from cellscreen.trainer import Trainer
    hw, ch, ne = shape
    w = WF.trained_like(31 + hw[1], hw, ch, ne)
    x = WF.edge_crops(hw, 12)
    ref = oracle.cae_forward(w, x, acc64=True, want=("mse", "mae"))
    tr = Trainer(w)
    try:
        loss, mae = tr.evaluate(x, x)
    finally:
        tr.close()
    want_loss, want_mae = ref["mse"].astype(np.float64).mean(), ref["mae"].astype(np.float64).mean()
    print(f"\nevaluate {hw}: loss err / bar {abs(loss - want_loss) / want_loss / H.TOL_ERR_REL:.3f}, MAE {abs(mae - want_mae) / want_mae / H.TOL_ERR_REL:.3f}")
    assert abs(loss - want_loss) <= H.TOL_ERR_REL * want_loss and abs(mae - want_mae) <= H.TOL_ERR_REL * want_mae
