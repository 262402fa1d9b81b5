"""The run-time-shaped conv path (csrc/conv_generic.hip, conv_generic_x3.hip) on the CPU: the library accepts exactly the
shapes that tests/generic_plans.py says it does, the GPU sweep's case list reaches every kernel instantiation of the
enumerated envelope, and the fp64 references (oracle.cae_forward, oracle/train_oracle.py) are pinned to torch at the
shapes that sweep uses.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import generic_plans as G
import helpers as H
from cellscreen import _lib as L
from cellscreen import synth
from cellscreen.engine import _fill_cae
from oracle import oracle


def _shape_only(hw, channels, n_enc, dummy):
    """A cs_cae_weights whose every array is one shared buffer: describe_arch judges shapes and NULLs only."""
    s = L.CSCaeWeights()
    s.height, s.width = hw
    s.n_conv, s.n_enc, s.bn_eps = len(channels), n_enc, 1e-3
    p = dummy.ctypes.data
    for l, c in enumerate(channels):
        s.channels[l] = c
        s.kernel[l] = s.bias[l] = p
        if l < len(channels) - 1:
            s.bn_gamma[l] = s.bn_beta[l] = s.bn_mean[l] = s.bn_var[l] = p
    return s


def test_acceptance_equals_the_library_over_the_envelope():
    """cs_model_from_arrays runs describe_arch before it looks for a device (api.hip:735-739): a refused shape is -6 on any
    machine.  device_id -1 makes an accepted one stop right after (-4 without a GPU, -1 with one: no model is built)."""
    lib = L.load_library()
    dummy = np.zeros(1, np.float32)
    h = C.c_void_p()
    n = n_acc = 0
    bad = []
    for hw, ch, ne in G.envelope():
        want = G.describe_arch(hw, ch, ne)
        rc = lib.cs_model_from_arrays(C.byref(_shape_only(hw, ch, ne, dummy)), None, None, -1, None, C.byref(h))
        n += 1
        if isinstance(want, G.Refused):
            ok = rc == -6 and (want.layer < 0 or f"conv {want.layer}:".encode() in lib.cs_last_error())
        else:
            n_acc += 1
            ok = rc in (-4, -1) and b"device" in lib.cs_last_error()
        if not ok:
            bad.append((hw, ch, ne, want, rc, lib.cs_last_error()))
    assert not bad, f"{len(bad)} of {n} points disagree, e.g. {bad[:3]}"
    assert n == len(G.EXTRA) + len(G.HW_STEPS) ** 2 * sum(len(G.channel_sets(e)) for e in G.N_ENCS) and n_acc > 5000


def test_accepted_shapes_build_a_model_when_a_device_is_visible():
    """A few accepted points with real (zero) weights on device 0: -4 without a GPU, a model with one (freed)."""
    lib = L.load_library()
    keep, h = [], C.c_void_p()
    for hw, ch, ne, _why in G.SWEEP_CASES[:6]:
        w = synth.random_cae(seed=1, hw=hw, channels=ch, n_enc=ne)
        for arr in w.kernels + w.biases:
            arr[...] = 0
        rc = lib.cs_model_from_arrays(C.byref(_fill_cae(w, keep)), None, None, 0, None, C.byref(h))
        assert rc == (-4 if lib.cs_device_count() <= 0 else 0), (hw, ch, ne, rc)
        if rc == 0:
            lib.cs_model_free(h)


def test_the_restatement_is_the_envelope_it_claims():
    """The accept / refuse rules of the grid, each with a witness, so that a restatement that accepts everything (or
    nothing) cannot pass the test above by accident."""
    rules = {}
    for hw, ch, ne in G.envelope():
        a = G.describe_arch(hw, ch, ne)
        rules.setdefault("accepted" if isinstance(a, G.Arch) else a.rule, (hw, ch, ne))
    assert {"accepted", "grid", "cin", "lds", "divisible", "grammar", "last"} <= set(rules), rules
    # the largest accepted cin per grid width (conv_generic.hip:720)
    for W, cmax in ((16, 564), (32, 296), (48, 200), (64, 148), (96, 100), (128, 72)):
        assert G.conv_generic_supported(16, W, cmax, 16) is None and G.conv_generic_supported(16, W, cmax + 4, 16) == "lds"


def _sweep_instantiations():
    got = {}
    for hw, ch, ne, _ in G.SWEEP_CASES:
        for prec in ("split16", "fp32_exact"):
            for lp in G.plan(hw, ch, ne, prec):
                got.setdefault((lp.kernel, prec), (hw, ch, ne, lp.layer))
    return got


def test_the_gpu_sweep_reaches_every_instantiation():
    """Every (kernel instantiation, precision) that some point of the enumerated grid reaches is run by at least one case
    of test_gpu_generic_sweep.py.  A plan change that moves a shape to another kernel fails here and names it."""
    pts = [p for p in G.envelope() if isinstance(G.describe_arch(*p), G.Arch)]
    sweep = _sweep_instantiations()
    for prec in ("split16", "fp32_exact"):
        reach = G.instantiations(pts, precisions=(prec,))
        missing = {k: v for k, v in reach.items() if (k, prec) not in sweep}
        assert not missing, f"{prec}: no sweep case runs {sorted(missing)}; e.g. {next(iter(missing.values()))}"
    names = {k for k, _ in sweep}
    # the kernel families of both files, at every template width the grid reaches
    assert len(names) == 29, sorted(names)
    for fam in ("conv_generic_kernel<", "conv_generic2_kernel<", "conv_generic_c1_kernel<", "conv_generic2f_kernel<",
                "conv_last_folded_kernel", "conv_last_generic_kernel", "conv_generic_x3_kernel<", "conv_last_x3_kernel<"):
        assert any(k.startswith(fam) for k in names), fam


def test_sweep_cases_have_a_persistent_loop_and_a_ragged_tail():
    for hw, ch, ne, _ in G.SWEEP_CASES:
        assert isinstance(G.describe_arch(hw, ch, ne), G.Arch), (hw, ch, ne)
        n = G.persistent_n(hw, ch, ne)
        for prec in ("split16", "fp32_exact"):
            for lp in G.plan(hw, ch, ne, prec):
                items = n * lp.items_per_cell
                assert items >= 3 * lp.grid(n) and items % lp.grid(n), (hw, ch, ne, prec, lp)
                assert G.final_round_cells(lp, n)[-1] == n - 1
        cells = G.oracle_cells(hw, ch, ne, n)
        assert 0 in cells and n - 1 in cells and len(cells) >= 5
    for hw, ch, ne, rule in G.ENGINE_REFUSALS:
        assert G.describe_arch(hw, ch, ne).rule == rule
    for hw, ch, ne, rule in G.TRAINER_REFUSALS:
        assert G.describe_trainer(hw, ch, ne).rule == rule


def test_trainer_acceptance_restatement():
    """train_api.hip:70-115 over the grid: every rule it has is reached, and a trainer-accepted shape is engine-accepted."""
    rules = {}
    for hw, ch, ne in G.envelope():
        r = G.describe_trainer(hw, ch, ne)
        if r is None:
            assert isinstance(G.describe_arch(hw, ch, ne), G.Arch), (hw, ch, ne)
        rules.setdefault("ok" if r is None else r.rule, (hw, ch, ne))
    assert {"ok", "grid", "pow2", "lds", "wgrad-lds", "backward-data lds"} <= set(rules), rules
    assert {ne for hw, ch, ne, _ in G.SWEEP_CASES if G.describe_trainer(hw, ch, ne) is None} == {1, 2, 3}


# ---- the fp64 references at the sweep's shapes -------------------------------------------------------------------
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

PIN_SHAPES = [
    ((32, 64), (8, 12, 1), 1),                    # n_enc 1, non-square
    ((48, 64), (12, 20, 1), 1),                   # H not a power of two
    ((32, 32), (8, 16, 1, 12, 1), 2),             # n_enc 2 with a 1-filter bottleneck
    ((16, 32), (1, 8, 1), 1),                     # a 1-filter first conv
    ((32, 128), (16, 296, 564, 16, 16, 16, 1), 3),   # more than 256 filters (the sweep's widest case)
]


def _torch_forward(w, x):
    T = lambda a: torch.from_numpy(np.asarray(a)).double()
    h = T(x)[:, None]
    out = []
    for l in range(w.n_conv):
        if l > w.n_enc:
            h = F.interpolate(h, scale_factor=2, mode="nearest")
        h = F.conv2d(h, T(w.kernels[l]).permute(3, 2, 0, 1), T(w.biases[l]), padding=1)
        if l < w.n_conv - 1:
            h = F.batch_norm(F.relu(h), T(w.bn_mean[l]), T(w.bn_var[l]), T(w.bn_gamma[l]), T(w.bn_beta[l]), False, 0.0, w.bn_eps)
            if l < w.n_enc:
                h = F.max_pool2d(h, 2)
        else:
            h = torch.sigmoid(h)
        out.append(h.permute(0, 2, 3, 1).numpy())
    return out


@pytest.mark.parametrize("hw,channels,n_enc", PIN_SHAPES)
def test_oracle_vs_torch_at_generic_shapes(hw, channels, n_enc):
    w = synth.random_cae(seed=21, hw=hw, channels=channels, n_enc=n_enc)
    for l in range(n_enc):
        w.bn_gamma[l][::3] *= -1.0                 # the pool must see BN's output
    x = np.concatenate([synth.synth_crops(4, 10, 2, hw=hw), synth.blob_crops(3, 2, hw=hw)])
    r = oracle.cae_forward(w, x, acc64=True, layers=True)
    want = _torch_forward(w, x)
    for l in range(w.n_conv):
        H.assert_close_scaled(r["layers"][l], want[l], 2e-6, f"layer {l}")
    feat = want[n_enc - 1].reshape(len(x), -1)
    H.assert_close_scaled(r["features"].reshape(feat.shape), feat, 2e-6, "features (h,w,c)")
    err = ((want[-1][..., 0] - x.astype(np.float64)) ** 2).reshape(len(x), -1).mean(axis=1)
    H.assert_rel(r["mse"], err, 1e-6, "mse")


def _torch_train_loss(w, x, y):
    P = lambda a: torch.nn.Parameter(torch.from_numpy(np.array(a, dtype=np.float64)))
    params = []
    h = torch.from_numpy(x).double()[:, None]
    for l in range(w.n_conv):
        k, b = P(w.kernels[l]), P(w.biases[l])
        params += [k, b]
        if l > w.n_enc:
            h = F.interpolate(h, scale_factor=2, mode="nearest")
        h = F.conv2d(h, k.permute(3, 2, 0, 1), b, padding=1)
        if l < w.n_conv - 1:
            g, be = P(w.bn_gamma[l]), P(w.bn_beta[l])
            params += [g, be]
            h = F.relu(h)
            mu, var = h.mean(dim=(0, 2, 3)), h.var(dim=(0, 2, 3), unbiased=False)
            h = (h - mu[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + w.bn_eps) * g[None, :, None, None] + be[None, :, None, None]
            if l < w.n_enc:
                h = F.max_pool2d(h, 2)
        else:
            h = torch.sigmoid(h)
    loss = ((h[:, 0] - torch.from_numpy(y).double()) ** 2).mean()
    loss.backward()
    return loss.item(), [p.grad.numpy() for p in params]


@pytest.mark.parametrize("hw,channels,n_enc", [((32, 64), (8, 12, 1), 1), ((16, 32), (4, 8, 16, 8, 1), 2)])
def test_train_oracle_vs_torch_autograd_at_generic_shapes(hw, channels, n_enc):
    from oracle import train_oracle as T
    w = synth.random_cae(seed=8, hw=hw, channels=channels, n_enc=n_enc)
    x = synth.blob_crops(5, 3, hw=hw)
    y = np.clip(x + 0.02 * np.random.default_rng(1).standard_normal(x.shape).astype(np.float32), 0, 1)
    r = T.forward_backward(T.TrainState(w), x, y)
    loss, grads = _torch_train_loss(w, x, y)
    assert abs(r["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert len(r["grads"]) == len(grads)
    for i, (g, tg) in enumerate(zip(r["grads"], grads)):
        assert g.shape == tg.shape, i
        assert np.linalg.norm(g - tg) <= 1e-9 * max(np.linalg.norm(tg), 1e-30), i
