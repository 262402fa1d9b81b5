"""Every run-time-shaped conv kernel instantiation (csrc/conv_generic.hip, conv_generic_x3.hip) at the shapes where such
kernels go wrong: the case list tests/generic_plans.py SWEEP_CASES (its CPU test proves that it reaches every
instantiation of the enumerated envelope), in both precisions, against the fp64 oracle at the existing bars.  Each case
runs at a cell count where every launch loops over its persistent grid at least three times and ends on a ragged round;
the cells only such a last round reaches are among those checked against the oracle, and all cells are checked bit for
bit against an odd pass size, a repeat and device-resident input.  Plus the trainer (csrc/train_generic.hip) at the
trainer-accepted cases, and refusals just outside both envelopes."""
import numpy as np
import pytest

import generic_plans as G
import helpers as H
from cellscreen import _lib as L
from cellscreen import synth
from cellscreen.engine import Engine
from oracle import oracle

pytestmark = pytest.mark.gpu

PRECISIONS = ("split16", "fp32_exact")
WORST = {}           # (instantiation, precision) -> largest observed error / its bar


def _id(c):
    hw, ch, ne, _ = c
    return f"{hw[0]}x{hw[1]}-{'-'.join(map(str, ch))}"


def _crops(hw, n, seed):
    x = synth.synth_crops(seed, 0, n, hw=hw)
    x[1::2] = synth.blob_crops(seed, n // 2, hw=hw)
    return x


def _note(lp, prec, ratio):
    k = (lp.kernel, prec)
    WORST[k] = max(WORST.get(k, 0.0), ratio)


def _check_profile(e, plans, a):
    """The library took the restated path: per position l < 6, the split counter (which reads the library's own
    gae.x3[l], api.hip:1349-1357) is > 0 exactly where a split kernel is restated, the fp32-MFMA one exactly where not.
    The fp32 counter of the 1-filter last convs on the vector unit is a formula (api.hip:1320-1325), checked as one."""
    prof = e.profile()
    names = list(prof)
    for lp in plans:
        l = lp.layer
        if l >= 6:                                        # n_enc 3's sigmoid conv: the conv7 bucket, no split counter
            continue
        bf, mf = prof[names[l]]["bf16_mfma_per_cell"], prof[names[l]]["mfma_per_cell"]
        assert (bf > 0) == lp.split and (mf > 0) == (not lp.split), (lp, bf, mf)
        gh, gw = lp.grid_hw
        cpad = (lp.cout + 15) // 16 * 16
        if lp.split:
            last = l == a.n_conv - 1
            taps = 4.0 if l > a.n_enc else 9.0
            assert bf == gh * gw / 16 * (cpad // 16) * taps * (lp.cin / 32) * (6.0 if last else 3.0), (lp, bf)
        else:
            assert mf == gh * gw / 16 * (cpad // 16) * (9.0 * lp.cin / 4.0), (lp, mf)


@pytest.mark.parametrize("case", G.SWEEP_CASES, ids=[_id(c) for c in G.SWEEP_CASES])
def test_generic_sweep(case):
    import torch
    hw, ch, ne, _why = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w = synth.random_cae(seed=len(ch) * 1000 + hw[0] + hw[1], hw=hw, channels=ch, n_enc=ne)
    a = G.describe_arch(hw, ch, ne)
    n = G.persistent_n(hw, ch, ne, cus)
    cells = G.oracle_cells(hw, ch, ne, n, seed=hw[0], cus=cus)
    x = _crops(hw, n, seed=hw[1] + len(ch))
    ref = oracle.cae_forward(w, x[cells], acc64=True, layers=True)
    xs = x[cells]
    report = {}
    for prec in PRECISIONS:
        plans = G.plan(hw, ch, ne, prec, cus)
        e = Engine.from_weights(w, precision=prec)
        try:
            _check_profile(e, plans, a)
            for lp in plans:                                  # every layer on the oracle's cells
                l = lp.layer
                got = e.layer_output(xs, l)
                tol = H.TOL_FEATURES if l < a.n_conv - 1 else H.TOL_RECON
                r = H.assert_close_scaled(got, ref["layers"][l].reshape(got.shape), tol, f"{prec} layer {l} ({lp.kernel})")
                _note(lp, prec, r / tol)
                report[(prec, l)] = f"{lp.kernel} {r / tol:.2f}"
            # all n cells: the persistent grid-stride loop and its ragged last round, in every layer
            rec, mse, mae = e.reconstruct(x)
            f = e.encode(x)
            assert np.abs(rec[cells] - ref["recon"].reshape(rec[cells].shape)).max() <= H.TOL_RECON, prec
            H.assert_rel(mse[cells], ref["mse"], H.TOL_ERR_REL, f"{prec} mse")
            H.assert_rel(mae[cells], ref["mae"], H.TOL_ERR_REL, f"{prec} mae")
            H.assert_close_scaled(f[cells], ref["features"].reshape(len(cells), -1), H.TOL_FEATURES, f"{prec} features (h,w,c)")
            r2 = e.reconstruct(x)                             # determinism
            assert all(np.array_equal(p, q) for p, q in zip(r2, (rec, mse, mae))), f"{prec}: a repeat differs"
            assert np.array_equal(e.encode(x), f), f"{prec}: a repeat's features differ"
            xd = torch.from_numpy(x).cuda()                   # device-resident input
            rd = [t.cpu().numpy() for t in e.reconstruct(xd)]
            assert all(np.array_equal(p, q) for p, q in zip(rd, (rec, mse, mae))), f"{prec}: device input differs"
            assert np.array_equal(e.encode(xd).cpu().numpy(), f), f"{prec}: device input's features differ"
            del xd
            e.set_chunk(n // 3 | 1)                           # an odd pass size: other grids, other ragged rounds
            r3 = e.reconstruct(x)
            assert all(np.array_equal(p, q) for p, q in zip(r3, (rec, mse, mae))), f"{prec}: chunk {n // 3 | 1} differs"
            assert np.array_equal(e.encode(x), f), f"{prec}: chunk {n // 3 | 1}'s features differ"
        finally:
            e.close()
    print(f"\n{_id(case)} n={n} oracle cells={cells}: error / bar per layer", report)


def test_generic_engine_refusals():
    for hw, ch, ne, rule in G.ENGINE_REFUSALS:
        with pytest.raises(L.CellScreenError) as ei:
            Engine.from_weights(synth.random_cae(seed=2, hw=hw, channels=ch, n_enc=ne))
        assert ei.value.status == -6, (hw, ch, ne)
        assert f"conv {G.describe_arch(hw, ch, ne).layer}:" in str(ei.value), (hw, ch, ne, str(ei.value))


# ---- the trainer on the run-time-shaped kernels ----------------------------------------------------------------
TRAIN_CASES = [c for c in G.SWEEP_CASES if G.describe_trainer(*c[:3]) is None]


@pytest.mark.parametrize("batch", [3, 32])
@pytest.mark.parametrize("case", TRAIN_CASES, ids=[_id(c) for c in TRAIN_CASES])
def test_generic_trainer_sweep(case, batch):
    """Gradients at <= 1e-5 relative L2 against oracle/train_oracle.py on the trainer's own activation pattern, the moving
    statistics, and forward_backward + apply == step bit for bit."""
    from cellscreen.trainer import Trainer, param_layout, split_flat
    from oracle import train_oracle as T
    hw, ch, ne, _ = case
    w = synth.random_cae(seed=17 + ne, hw=hw, channels=ch, n_enc=ne)
    y = synth.blob_crops(23, batch, hw=hw)
    x = np.clip(y + np.random.default_rng(4).normal(0, 0.02, y.shape), 0, 1).astype(np.float32)
    tr = Trainer(w)
    a = b = None
    try:
        loss, mae = tr.forward_backward(x, y)
        masks, args = H.activation_pattern(tr, w, batch)
        st = T.TrainState(w, dtype=np.float64)
        ref = T.forward_backward(st, x, y, relu_masks=masks, pool_args=args)
        assert abs(loss - ref["loss"]) <= 1e-5 * ref["loss"] and abs(mae - ref["mae"]) <= 1e-5 * ref["mae"]
        _, mov, g = tr.export_flat(grads=True)
        got = split_flat(g, param_layout(ch))
        errs = {name: np.linalg.norm(got[name].astype(np.float64) - gr) / max(np.linalg.norm(gr), 1e-30)
                for (name, _s), gr in zip(param_layout(ch), ref["grads"])}
        print(f"\n{_id(case)} batch {batch}: worst gradient relative L2 {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
        assert max(errs.values()) <= 1e-5, max(errs, key=errs.get)
        o = 0
        for l in range(w.n_conv - 1):
            c = ch[l]
            assert np.allclose(mov[o:o + c], st.mov_mean[l], rtol=1e-5, atol=1e-7); o += c
            assert np.allclose(mov[o:o + c], st.mov_var[l], rtol=1e-5, atol=1e-7); o += c
        a, b = Trainer(w), Trainer(w)
        for s in range(2):
            la, _ = a.forward_backward(x, y)
            a.apply(1e-3)
            lb, _ = b.step(x, y, 1e-3)
            assert la == lb, s
        pa, ma = a.export_flat()
        pb, mb = b.export_flat()
        assert np.array_equal(pa, pb) and np.array_equal(ma, mb)
    finally:
        tr.close()
        if a is not None:
            a.close()
        if b is not None:
            b.close()


def test_generic_trainer_refusals():
    from cellscreen.trainer import Trainer
    assert isinstance(G.describe_arch(*G.TRAINER_REFUSALS[0][:3]), G.Arch)      # the engine serves what the trainer refuses
    for hw, ch, ne, rule in G.TRAINER_REFUSALS:
        with pytest.raises(L.CellScreenError) as ei:
            Trainer(synth.random_cae(seed=3, hw=hw, channels=ch, n_enc=ne))
        assert ei.value.status == -6, (hw, ch, ne)
        assert {"pow2": "powers of two", "wgrad-lds": "weight gradient"}[rule] in str(ei.value), str(ei.value)


def test_zz_worst_error_per_instantiation():
    """Printed for the record: the largest error seen per (instantiation, precision), as a fraction of its bar."""
    for (k, prec), r in sorted(WORST.items()):
        print(f"{k:40s} {prec:10s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
