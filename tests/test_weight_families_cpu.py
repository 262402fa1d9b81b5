"""The weight families of tests/weight_families.py are what they claim to be (checked by the float64 forward and the C
oracle, no GPU), compensation preserves the function, and the run-time-shaped cases the GPU file runs reach every kernel
instantiation of generic_plans.SWEEP_CASES."""
import numpy as np
import pytest

import generic_plans as G
import helpers as H
import weight_families as WF
from oracle import oracle

REF = ((64, 64), (32, 64, 32, 32, 64, 32, 1), 3)
SHAPES = [REF, ((64, 128), (8, 16, 32, 32, 16, 8, 1), 3), ((48, 64), (64, 32, 1), 1)]
_ids = [f"{hw[0]}x{hw[1]}-{'-'.join(map(str, ch))}" for hw, ch, _ in SHAPES]


@pytest.fixture(scope="module", params=SHAPES, ids=_ids)
def drawn(request):
    hw, ch, ne = request.param
    seed = 11 + ne
    w, info = WF.trained_like(seed, hw, ch, ne, with_info=True)
    x = WF.calibration_crops(seed, hw)
    return w, info, x, WF.forward64(w, x)


def test_trained_like_is_seeded():
    a, b, c = WF.trained_like(3), WF.trained_like(3), WF.trained_like(4)
    for f in ("kernels", "biases", "bn_gamma", "bn_beta", "bn_mean", "bn_var"):
        assert all(np.array_equal(p, q) for p, q in zip(getattr(a, f), getattr(b, f))), f
    assert not np.array_equal(a.biases[0], c.biases[0])


def test_generator_conditions(drawn):
    w, info, x, fwd = drawn
    nh = w.n_conv - 1
    for l in range(w.n_conv):
        b = w.biases[l].astype(np.float64)
        assert (b != 0).all(), f"conv {l}: a zero bias"
        rms, top = info.response_rms[l], info.response_max[l]
        # the response statistics the generator recorded are those of the float64 forward
        resp = fwd[l]["z"] - b
        assert np.allclose(np.sqrt((resp * resp).mean(axis=(0, 1, 2))), rms, rtol=1e-9, atol=0)
        special = np.concatenate([info.dead[l], info.never_clipped[l]]) if l < nh else np.zeros(0, int)
        plain = np.setdiff1d(np.arange(len(b)), special)
        ratio = np.abs(b[plain]) / rms[plain]
        assert ratio.min() >= 0.05 * (1 - 1e-6) and ratio.max() <= 1 + 1e-6, (l, ratio.min(), ratio.max())
        if len(plain) >= 8:
            assert (b[plain] > 0).any() and (b[plain] < 0).any(), f"conv {l}: biases of one sign"
    for l in range(nh):
        c = w.channels[l]
        z = fwd[l]["z"]
        assert len(info.dead[l]) == 2 and len(info.never_clipped[l]) == 2, "the CPU shapes are wide enough for every role"
        roles = np.concatenate([info.dead[l], info.never_clipped[l], info.gamma_zero[l], info.var_zero[l], info.var_tiny[l]])
        assert len(np.unique(roles)) == 7
        s, t = w.bn_scale_shift()
        for f in info.dead[l]:
            assert w.biases[l][f] <= -WF.DEAD_MARGIN * info.response_max[l][f]
            assert z[..., f].max() < 0
            assert np.array_equal(fwd[l]["out"][..., f], np.full_like(fwd[l]["out"][..., f], np.float64(t[l][f])))
        for f in info.never_clipped[l]:
            assert w.biases[l][f] >= WF.DEAD_MARGIN * info.response_max[l][f]
            assert z[..., f].min() > 0
        assert w.bn_gamma[l][info.gamma_zero[l][0]] == 0 and (np.delete(w.bn_gamma[l], info.gamma_zero[l]) != 0).all()
        assert w.bn_var[l][info.var_zero[l][0]] == 0 and w.bn_var[l][info.var_tiny[l][0]] == np.float32(1e-6)
        g = np.abs(np.delete(w.bn_gamma[l].astype(np.float64), info.gamma_zero[l]))
        assert (w.bn_gamma[l] > 0).any() and (w.bn_gamma[l] < 0).any()
        assert g.max() / g.min() <= 2.0 ** 8 * (1 + 1e-6)
        if c >= 32:
            assert g.max() / g.min() >= 2.0 ** 4, "the gains of a wide layer span orders of magnitude"
        assert w.bn_var[l].max() <= 1e2 and np.delete(w.bn_var[l], [info.var_zero[l][0], info.var_tiny[l][0]]).min() >= 1e-4 * (1 - 1e-6)
        assert (np.abs(w.bn_mean[l]) <= 2 * info.response_rms[l] * (1 + 1e-6)).all()
        out = fwd[l]["out"]
        rms = np.sqrt((out * out).mean())
        assert 0.5 <= rms < 2.0, f"layer {l}: output RMS {rms}"
        print(f"layer {l}: RMS {rms:.3f}, max {np.abs(out).max():.2f}, |bn scale| {np.abs(s[l]).min():.2e} .. {np.abs(s[l]).max():.2e}")
    assert np.abs(fwd[-1]["z"]).max() <= WF.Z7_MAX
    # the C oracle agrees with the float64 forward that calibrated (it rounds every layer to float32 on the way)
    ref = oracle.cae_forward(w, x, acc64=True, layers=True)["layers"]
    for l in range(w.n_conv):
        H.assert_close_scaled(ref[l], fwd[l]["out"].reshape(ref[l].shape), 2e-6, f"layer {l}")


def test_kernel_filters_carry_powers_of_two():
    from cellscreen import synth
    w, base = WF.trained_like(5), synth.random_cae(5)
    for l in range(6):
        r = w.kernels[l].astype(np.float64) / base.kernels[l]
        per = r.reshape(-1, r.shape[-1])
        assert (per == per[0]).all() and set(np.log2(per[0])) <= set(range(-4, 3)), l
        assert len(set(per[0])) >= 4, l


@pytest.mark.parametrize("k", [6, 12, 24])
def test_compensation_preserves_the_function(k):
    """Only float64 rounding may differ -- and does not: the moved channels come out scaled by exactly 2^-k, everything
    else bit for bit."""
    w = WF.trained_like(21)
    c = WF.compensated(w, k, seed=k)
    ch = WF.compensated_channels(w, k)
    assert all(len(i) == max(1, n // 3) for i, n in zip(ch, w.channels[:-1]))
    for l in range(6):
        rest = np.setdiff1d(np.arange(w.channels[l]), ch[l])
        assert np.array_equal(c.bn_gamma[l][ch[l]], w.bn_gamma[l][ch[l]] * np.float32(2.0 ** -k))
        assert np.array_equal(c.bn_gamma[l][rest], w.bn_gamma[l][rest])
        assert np.array_equal(c.kernels[l + 1][:, :, ch[l], :], w.kernels[l + 1][:, :, ch[l], :] * np.float32(2.0 ** k))
        # the boosted weights are the layer's largest, the moved channels far below their cell's maximum
        assert np.abs(c.kernels[l + 1][:, :, ch[l], :]).max() == np.abs(c.kernels[l + 1]).max()
    x = WF.edge_crops()
    a = oracle.cae_forward(w, x, acc64=True, layers=True)
    b = oracle.cae_forward(c, x, acc64=True, layers=True)
    for l in range(7):
        got = WF.uncompensate(b["layers"][l], l, w, k, seed=k) if l < 6 else b["layers"][l]
        H.assert_close_scaled(got, a["layers"][l], 1e-12, f"k {k}, layer {l}")
        err = np.abs(got.astype(np.float64) - a["layers"][l])
        assert (err <= 1e-12 * np.abs(a["layers"][l])).all(), f"k {k}, layer {l}: element-wise"
    for key in ("features", "recon", "mse", "mae"):
        got = WF.uncompensate(b[key].reshape(len(x), 8, 8, 32), 2, w, k, seed=k).reshape(len(x), -1) if key == "features" else b[key]
        H.assert_rel(got, a[key], 1e-12, f"k {k}, {key}")
    # ... and in the float64 forward of this file
    fa, fb = WF.forward64(w, x), WF.forward64(c, x)
    for l in range(7):
        got = WF.uncompensate(fb[l]["out"], l, w, k, seed=k) if l < 6 else fb[l]["out"]
        H.assert_close_scaled(got, fa[l]["out"], 1e-12, f"float64 forward, k {k}, layer {l}")


def test_generic_cases_reach_every_instantiation():
    chosen, full = WF.greedy_cover(G.SWEEP_CASES)
    sweep = [tuple(c[:3]) for c in G.SWEEP_CASES]
    assert all(c in sweep for c in WF.GENERIC_CASES)
    got = G.instantiations(points=WF.GENERIC_CASES)
    reached = {(k, prec) for prec in ("split16", "fp32_exact") for k in G.instantiations(points=WF.GENERIC_CASES, precisions=(prec,))}
    assert full == {(k, prec) for prec in ("split16", "fp32_exact") for k in G.instantiations(points=sweep, precisions=(prec,))}
    missing = sorted(full - reached)
    assert not missing, f"not reached: {missing}"
    assert reached == full and set(got) == set(G.instantiations(points=sweep))
    assert WF.GENERIC_CASES == chosen, "the committed list is the greedy choice"
    for name, where in sorted(got.items()):
        print(f"{name:40s} {where}")
    # the compensated cases: both forms of the x3 split kernel and both conv_last_x3
    x3 = set(G.instantiations(points=WF.GENERIC_COMPENSATED, precisions=("split16",)))
    assert {"conv_last_x3_kernel<32>", "conv_last_x3_kernel<64>"} <= x3
    assert any("x3_kernel" in k and "plain" in k for k in x3) and any("x3_kernel" in k and "fold" in k for k in x3)
    assert all(c in WF.GENERIC_CASES for c in WF.GENERIC_COMPENSATED)


def test_plain_float32_meets_the_per_channel_bar():
    """The per-channel bar of test_gpu_weight_families.py, 1e-5 B_c, is one plain float32 arithmetic meets with room: each
    layer in float32 numpy from the oracle's input to it."""
    w = WF.trained_like(WF.REF_SEED)
    x = WF.edge_crops()
    ref = oracle.cae_forward(w, x, acc64=True, layers=True)["layers"]
    prev = x
    for l in range(6):
        B = WF.channel_budget(w, l, prev)
        rng = np.abs(ref[l]).reshape(-1, ref[l].shape[-1]).max(axis=0)
        assert (B >= rng * (1 - 1e-6)).all(), f"layer {l}: a budget below the channel's range"
        err = np.abs(WF.plain32_layer(w, l, prev).astype(np.float64) - ref[l]).reshape(-1, len(B)).max(axis=0)
        worst = (err / B).max()
        print(f"layer {l}: plain float32 worst |err| / B_c = {worst:.2e}")
        assert worst <= WF.PER_CHANNEL_TOL
        prev = ref[l]
