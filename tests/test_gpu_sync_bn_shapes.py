"""Synchronised BatchNormalization for run-time-shaped trainers, through the blocking all-gather hook (cs_train_set_sync_bn) and
the stream-ordered one (cs_train_set_sync_bn_stream) alike.

Inputs: case i of train_plans.GENERIC_CASES with the base batch tests/test_gpu_train_batches.py already uses for it (3 cells), as
8 shuffled copies -- 24 cells, split in rank order over 2, 4 or 8 ranks.  A batch of shuffled copies has the base batch's step
(tests/test_sync_bn_shapes_cpu.py, 1e-10), so the float64 oracle (oracle/train_oracle.py) on the 3 base cells is the exact
reference for the loss, the MAE, the moving statistics and every gradient of the whole batch.  The rank compositions are uneven
(at 2 ranks the base cells are held (3, 3, 6) and (5, 5, 2) times, at 8 some ranks lack a base cell altogether), so per-rank
statistics give another gradient: the unsynchronised control asserts that, once per case.

Bars (as tests/test_gpu_train_batches.py applies them): 1e-5 relative L2 per gradient tensor, 1e-5 relative
on loss and MAE, rtol 1e-5 / atol 1e-7 on the moving statistics; each side (the ranks' mean, the single handle on the 24 cells)
against the oracle on its OWN ReLU / pooling decisions, the share of decisions that differ from the free float64 oracle, and
between the two sides, at most 1e-5.

Every rank is a thread with its own trainer; a rank that fails aborts the barrier the fake communicators meet at, and every join
has a timeout: a mistake fails, it does not hang."""
import ctypes as C
import functools
import os
import socket
import threading
import warnings

import numpy as np
import pytest

import helpers as H
import train_plans as TP
from cellscreen import _lib as L
from cellscreen import synth
from cellscreen.trainer import Trainer, param_layout, split_flat
from oracle import train_oracle as T

pytestmark = pytest.mark.gpu
TOL = 1e-5
COPIES = 8
HOOKS = ("blocking", "stream")
CONFIG4_CASE = len(TP.GENERIC_CASES) - 1
RECT_CASE = next(i for i, c in enumerate(TP.GENERIC_CASES) if c[0] == (64, 128) and len(c[1]) == 7)      # 64 x 128, seven convs
SPLITS = [(i, 4) for i in range(len(TP.GENERIC_CASES))] + [(i, wd) for i in (RECT_CASE, CONFIG4_CASE) for wd in (2, 8)]


# ------------------------------------------------------------------------------------------------ the fake communicators
class Exchange:
    """The all-gather of `world` ranks living in one process, in both forms of the hook."""

    def __init__(self, world, timeout):
        self.world, self.timeout = world, timeout
        self.barrier = threading.Barrier(world)
        self.bufs, self.written, self.copied = {}, {}, {}

    def blocking(self, rank):
        """cs_train_set_sync_bn's contract: the library has drained its stream; return when the buffer is complete on the device."""
        import torch

        def all_gather(buf, fpr):
            self.bufs[rank] = buf
            self.barrier.wait(self.timeout)                  # every slot is written
            for o in range(self.world):
                if o != rank:
                    buf[o * fpr:(o + 1) * fpr].copy_(self.bufs[o][o * fpr:(o + 1) * fpr])
            torch.cuda.synchronize()
            self.barrier.wait(self.timeout)                  # nobody rewrites its slot before the others have copied it
        return all_gather

    def stream(self, rank):
        """cs_train_set_sync_bn_stream's contract, with no wait for the device anywhere: events order the ranks' streams; the host
        barriers only publish the events (a stream wait on an event nobody has recorded yet is a no-op: record, then meet)."""
        import torch

        def all_gather(buf, fpr, stream):
            s = torch.cuda.ExternalStream(stream, device=buf.device)
            written = torch.cuda.Event()
            written.record(s)                                # this rank's slot is written
            self.bufs[rank], self.written[rank] = buf, written
            self.barrier.wait(self.timeout)
            with torch.cuda.stream(s):
                for o in range(self.world):
                    if o != rank:
                        s.wait_event(self.written[o])
                        buf[o * fpr:(o + 1) * fpr].copy_(self.bufs[o][o * fpr:(o + 1) * fpr], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(s)
            self.copied[rank] = copied
            self.barrier.wait(self.timeout)
            for o in range(self.world):                      # this rank's next write to its slot comes after every peer has read it
                if o != rank:
                    s.wait_event(self.copied[o])
        return all_gather

    def register(self, tr, rank, hook):
        if hook == "blocking":
            tr.set_sync_bn(self.blocking(rank), rank, self.world)
        else:
            tr.set_sync_bn_stream(self.stream(rank), rank, self.world)


def ranks_step(w, x, y, world, keep, hook, timeout=300):
    """`world` trainers in one process, rank r given cells [r n / world, (r + 1) n / world), one forward_backward each on its own
    thread.  hook: "blocking", "stream", or None (no exchange: per-rank statistics).  Returns ([(loss, mae)] per rank,
    [export_flat(grads=True)] per rank, the relu tensors of the cells in `keep` per layer)."""
    tr = [Trainer(w) for _ in range(world)]
    ex = Exchange(world, timeout)
    out, errors = [None] * world, []
    per = len(x) // world
    assert per * world == len(x)

    def run(rank):
        try:
            if hook is not None:
                ex.register(tr[rank], rank, hook)
            out[rank] = tr[rank].forward_backward(x[per * rank:per * (rank + 1)], y[per * rank:per * (rank + 1)])
        except BaseException as e:  # noqa: BLE001 - reported by the caller's thread
            errors.append((rank, e))
            ex.barrier.abort()
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    try:
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=timeout)
        assert not any(t.is_alive() for t in th), "a rank did not return"
        assert not errors, errors
        relus = [np.concatenate([t.tensor(0, l, per) for t in tr])[keep] for l in range(w.n_conv - 1)] if keep is not None else None
        return out, [t.export_flat(grads=True) for t in tr], relus
    finally:
        if not any(t.is_alive() for t in th):
            for t in tr:
                t.close()


# ------------------------------------------------------------------------------------------------ inputs and the reference
@functools.lru_cache(maxsize=None)
def case(i):
    hw, ch, ne, _why = TP.GENERIC_CASES[i]
    w = TP.weights(TP.WSEED + ne, hw=hw, channels=ch, n_enc=ne)
    x, y = TP.mixed_batch(TP.GENERIC_BASE, 40 + i, hw)
    free = T.forward_backward(T.TrainState(w, dtype=np.float64), x, y, update_moving=False)
    return w, x, y, [r > 0 for r in free["relu"][:w.n_conv - 1]]


@functools.lru_cache(maxsize=None)
def split(i, world):
    w, x, y, _ = case(i)
    xb, yb, idx = TP.replicate(x, y, COPIES, seed=world)
    first = np.array([int(np.flatnonzero(idx == j)[0]) for j in range(len(x))])
    return xb, yb, idx, first


def grads_by_name(w, flat):
    return split_flat(np.asarray(flat, np.float64), param_layout(w.channels))


def rel_errors(got, want):
    return {k: np.linalg.norm(got[k] - want[k]) / max(np.linalg.norm(want[k]), 1e-30) for k in want}


def against_the_oracle(i, who, masks, args, loss, mae, grads, moving):
    """One side on its own decisions against the float64 oracle on the base batch; returns what missed its bar."""
    w, x, y, free = case(i)
    nl = w.n_conv - 1
    st = T.TrainState(w, dtype=np.float64)
    ref = T.forward_backward(st, x, y, relu_masks=masks, pool_args=args)
    share = sum(int(np.sum(m != f)) for m, f in zip(masks[:nl], free)) / sum(m.size for m in masks[:nl])
    want = {name: np.asarray(g, np.float64) for (name, _s), g in zip(param_layout(w.channels), ref["grads"])}
    errs = rel_errors(grads, want)
    worst = max(errs, key=errs.get)
    figures = {"decisions": share / 1e-5, "loss": abs(loss - ref["loss"]) / ref["loss"] / TOL, "mae": abs(mae - ref["mae"]) / ref["mae"] / TOL,
               "gradient": errs[worst] / TOL}
    print(f"  {who} vs the float64 oracle, error / bar:", {k: float("%.2e" % v) for k, v in figures.items()}, "worst gradient:", worst)
    bad = [f"{who}: {k} at {v:.3f} of its bar" for k, v in figures.items() if not v <= 1.0]
    o = 0
    for l in range(nl):
        c = w.channels[l]
        for what, m in (("mean", st.mov_mean[l]), ("variance", st.mov_var[l])):
            if not np.allclose(moving[o:o + c], m, rtol=1e-5, atol=1e-7):
                bad.append(f"{who}: moving {what} of layer {l}: max abs error {np.abs(moving[o:o + c] - m).max():.3e}")
            o += c
    return bad


@functools.lru_cache(maxsize=None)
def single_handle(i, world):
    """One handle's step on the whole 24 cells (the order of split(i, world)), held to the oracle on its own decisions."""
    w = case(i)[0]
    xb, yb, _idx, first = split(i, world)
    one = Trainer(w)
    try:
        loss, mae = one.forward_backward(xb, yb)
        _, mov, g = one.export_flat(grads=True)
        masks, args = H.pattern_of_relus([one.tensor(0, l, int(first.max()) + 1)[first] for l in range(w.n_conv - 1)], w)
    finally:
        one.close()
    bad = against_the_oracle(i, "one handle", masks, args, loss, mae, grads_by_name(w, g), mov)
    return g, masks, args, bad


@functools.lru_cache(maxsize=None)
def synchronised(i, world, hook):
    w = case(i)[0]
    xb, yb, _idx, first = split(i, world)
    out, ex, relus = ranks_step(w, xb, yb, world, first, hook)
    masks, args = H.pattern_of_relus(relus, w)
    return out, ex, masks, args


def case_id(i):
    hw, ch = TP.GENERIC_CASES[i][:2]
    return "%dx%d-%s" % (hw + ("_".join(map(str, ch)),))


# ------------------------------------------------------------------------------------------------ 1. the whole batch, any shape
@pytest.mark.parametrize("hook", HOOKS)
@pytest.mark.parametrize("i,world", SPLITS, ids=[f"{case_id(i)}-world{wd}" for i, wd in SPLITS])
def test_sync_bn_of_a_run_time_shaped_trainer_is_the_whole_batch(i, world, hook):
    """test_sync_bn_over_many_ranks_is_the_whole_batch for every run-time-shaped case: the mean of the ranks' losses and gradients
    and their ONE set of moving statistics are the whole batch's.  On the parent commit cs_train_set_sync_bn answered
    CS_ERR_UNSUPPORTED for these handles."""
    w = case(i)[0]
    nl, ne = w.n_conv - 1, w.n_enc
    g1, masks1, args1, bad1 = single_handle(i, world)
    out, ex, masks, args = synchronised(i, world, hook)
    total = sum(m.size for m in masks[:nl])
    differ = sum(int(np.sum(m != m1)) for m, m1 in zip(masks[:nl], masks1[:nl])) + sum(int(np.sum(a != a1)) for a, a1 in zip(args[:ne], args1[:ne]))
    print(f"sync-BN ({hook}) {case_id(i)}, {world} ranks x {COPIES * TP.GENERIC_BASE // world} cells: {differ} of {total} decisions differ from the single handle's")
    loss = float(np.mean([o[0] for o in out])); mae = float(np.mean([o[1] for o in out]))
    mean_g = grads_by_name(w, np.mean([e[2].astype(np.float64) for e in ex], axis=0))
    bad = against_the_oracle(i, "ranks", masks, args, loss, mae, mean_g, ex[0][1])
    assert not bad1, bad1
    assert not bad, bad
    assert differ <= 1e-5 * total
    for r in range(1, world):
        assert np.array_equal(ex[0][1], ex[r][1]), f"rank {r} exports other moving statistics than rank 0"
    if differ == 0:
        errs = rel_errors(mean_g, grads_by_name(w, g1))
        assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("i,world", SPLITS, ids=[f"{case_id(i)}-world{wd}" for i, wd in SPLITS])
def test_without_the_exchange_the_ranks_compute_another_gradient(i, world):
    """The control: per-rank statistics over these uneven splits are 6e-2 .. 8.5e-1 relative L2 away from the whole batch's gradient
    in the float64 oracle; anything above 1e-3 shows that the synchronised tests could have failed."""
    w = case(i)[0]
    xb, yb, _idx, _first = split(i, world)
    g1 = single_handle(i, world)[0]
    _out, ex, _ = ranks_step(w, xb, yb, world, None, None)
    errs = rel_errors(grads_by_name(w, np.mean([e[2].astype(np.float64) for e in ex], axis=0)), grads_by_name(w, g1))
    print(f"no exchange, {case_id(i)}, {world} ranks: worst gradient deviation {max(errs.values()):.3e}")
    assert max(errs.values()) > 1e-3, errs


# ------------------------------------------------------------------------------------------------ 2. the two hooks are one arithmetic
def same_bits(a, b):
    (out_a, ex_a), (out_b, ex_b) = a, b
    assert out_a == out_b, (out_a, out_b)                                   # the ranks' (loss, mae)
    for r, (p, q) in enumerate(zip(ex_a, ex_b)):
        for what, u, v in zip(("parameters", "moving statistics", "gradients"), p, q):
            assert np.array_equal(u, v), f"rank {r}: {what} differ between the hooks, max {np.abs(u - v).max():.3e}"


@pytest.mark.parametrize("i,world", SPLITS, ids=[f"{case_id(i)}-world{wd}" for i, wd in SPLITS])
def test_blocking_and_stream_ordered_hooks_give_the_same_bits(i, world):
    """Same kernels in the same order; only the host's waiting differs."""
    a, b = synchronised(i, world, "blocking"), synchronised(i, world, "stream")
    same_bits((a[0], a[1]), (b[0], b[1]))
    assert np.abs(a[1][0][2]).max() > 0


def test_blocking_and_stream_ordered_hooks_give_the_same_bits_on_the_reference_graph():
    w = TP.weights(TP.WSEED)
    x, y = TP.mixed_batch(32, TP.BASE_SEED[32])
    got = [ranks_step(w, x, y, 4, None, hook)[:2] for hook in HOOKS]
    same_bits(*got)
    assert np.abs(got[0][1][0][2]).max() > 0


# ------------------------------------------------------------------------------------------------ 3. the stream-ordered hook is that
def delay_cycles(torch, ms=60.0):
    """Cycles of torch's device-side sleep for about `ms` milliseconds (bounded: at most four times that), measured."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)                                                # loads the kernel
    probe = 1_000_000
    a.record(); torch.cuda._sleep(probe); b.record()
    torch.cuda.synchronize()
    per_ms = probe / max(a.elapsed_time(b), 1e-3)
    return int(min(ms * per_ms, 4 * ms * 2.5e6))                           # no clock behind the sleep runs faster than 2.5 GHz


@pytest.mark.parametrize("hook", HOOKS)
def test_the_library_does_not_drain_its_stream_before_the_stream_ordered_hook(hook):
    """A device-side delay of some tens of milliseconds sits in front of the handle's work (cs_train_wait_stream on the stream
    that sleeps), and the first hook call of the step looks whether the event behind the delay has completed.  Under the
    stream-ordered entry point it has not: the library only enqueued.  Under the blocking entry point it has (the library drains
    its stream first), which shows that the probe tells the two apart."""
    import torch
    hw, ch, ne = (32, 64), (16, 64, 32, 16, 1), 2
    w = TP.weights(TP.WSEED + ne, hw=hw, channels=ch, n_enc=ne)
    x, y = TP.mixed_batch(6, 77, hw)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    tr = Trainer(w)
    try:
        tr.forward_backward(xd, yd)                      # buffers of this batch size and the reduction descriptors exist
        side, after = torch.cuda.Stream(), torch.cuda.Event()
        seen = []

        def look(*_):
            if not seen:
                seen.append(after.query())
        if hook == "blocking":
            tr.set_sync_bn(lambda buf, fpr: look(), 0, 1)
        else:
            tr.set_sync_bn_stream(lambda buf, fpr, stream: look(), 0, 1)
        cycles = delay_cycles(torch)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            after.record(side)
        L.check(tr._lib.cs_train_wait_stream(tr._h, C.c_void_p(side.cuda_stream)))
        loss, _ = tr.forward_backward(xd, yd)
        assert np.isfinite(loss) and after.query()       # the step's own read-back waited for everything
        assert seen == [hook == "blocking"], f"{hook} hook: the delay in front of the step had {'completed' if seen[0] else 'not completed'} at the first call"
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------ 4. failures
def test_a_rank_whose_stream_ordered_hook_raises_fails_every_rank():
    """test_sync_bn_rank_that_raises_fails_the_step_instead_of_hanging with the stream-ordered hook on a run-time shape."""
    hw, ch, ne = (32, 64), (16, 64, 32, 16, 1), 2
    w = TP.weights(TP.WSEED + ne, hw=hw, channels=ch, n_enc=ne)
    x, y = TP.mixed_batch(8, 78, hw)
    tr = [Trainer(w) for _ in range(2)]
    ex = Exchange(2, 60)
    seen = []

    def failing(buf, fpr, stream):
        ex.barrier.abort()
        raise RuntimeError("rank 1 lost its peer")

    def run(rank):
        try:
            tr[rank].set_sync_bn_stream(failing if rank == 1 else ex.stream(rank), rank, 2)
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
    by_rank = dict(seen)
    assert isinstance(by_rank[1], L.CellScreenError) and by_rank[1].status == -1 and isinstance(by_rank[1].__cause__, RuntimeError)
    assert isinstance(by_rank[0].__cause__, threading.BrokenBarrierError)
    for t in tr:
        t.close()


@pytest.mark.parametrize("hook", HOOKS)
def test_a_buffer_sized_for_64_filters_is_refused_by_a_handle_with_128(hook):
    import torch
    w = TP.weights(TP.WSEED + 3, hw=TP.CONFIG4[0], channels=TP.CONFIG4[1], n_enc=TP.CONFIG4[2])
    world = 4
    tr = Trainer(w)
    try:
        buf = torch.zeros(world * 3 * 128, dtype=torch.float32, device="cuda")
        if hook == "blocking":
            cb, fn = L.ALLGATHER_FN(lambda ctx, fpr: 0), tr._lib.cs_train_set_sync_bn
        else:
            cb, fn = L.ALLGATHER_STREAM_FN(lambda ctx, fpr, s: 0), tr._lib.cs_train_set_sync_bn_stream
        assert fn(tr._h, C.cast(cb, C.c_void_p), None, buf.data_ptr(), world * 3 * 64, 0, world) == -1      # CS_ERR_INVALID
        assert str(world * 3 * 128).encode() in tr._lib.cs_last_error(), tr._lib.cs_last_error()
        assert fn(tr._h, C.cast(cb, C.c_void_p), None, buf.data_ptr(), world * 3 * 128, 0, world) == 0
        assert fn(tr._h, None, None, None, 0, 0, 1) == 0
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------ 5. over RCCL, world size 1
@pytest.fixture(scope="module")
def nccl_world1():
    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def test_training_class_data_parallel_world1_on_64x128_crops(nccl_world1, tmp_path):
    """ImprovedAnomalyDetectionTraining(data_parallel=True) on 64 x 128 crops trains without a warning, and at world size 1 its
    history is the single-process run's."""
    from cellscreen.training import ImprovedAnomalyDetectionTraining
    cells = synth.blob_crops(23, 160, hw=(64, 128))
    t1 = ImprovedAnomalyDetectionTraining(str(tmp_path / "dp"), epochs=2, verbose=0, augment=None, data_parallel=True)
    t2 = ImprovedAnomalyDetectionTraining(str(tmp_path / "sp"), epochs=2, verbose=0, augment=None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a1, _, h1 = t1.train_autoencoder(cells)
    a2, _, h2 = t2.train_autoencoder(cells)
    assert h1.history["loss"] == h2.history["loss"] and h1.history["val_loss"] == h2.history["val_loss"]
    assert all(np.array_equal(p, q) for p, q in zip(a1.kernels, a2.kernels))


def test_enable_sync_bn_over_rccl_on_a_run_time_shape(nccl_world1):
    """Trainer.enable_sync_bn (all_gather_into_tensor issued under the handle's stream, no synchronize) at world size 1 on 64 x 128
    crops: the one rank's triples go through the collective and the second merge (a float rounding of M2 and of the two backward
    sums in between), so the step is the unsynchronised step at the bar -- its gradients where the two runs took the same ReLU
    decisions -- and the blocking form of the same hook gives the same bits."""
    import torch
    hw = (64, 128)
    w = TP.weights(TP.WSEED + 3, hw=hw)
    x, y = TP.mixed_batch(8, 79, hw)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    got = {}
    for how in ("off", "stream", "blocking"):
        tr = Trainer(w)
        try:
            if how != "off":
                tr.enable_sync_bn(nccl_world1, 0, 1, blocking=how == "blocking")
            got[how] = (tr.forward_backward(xd, yd),) + tr.export_flat(grads=True) + ([tr.tensor(0, l, 8) > 0 for l in range(6)],)
        finally:
            tr.close()
    assert got["stream"][0] == got["blocking"][0] and all(np.array_equal(p, q) for p, q in zip(got["stream"][1:4], got["blocking"][1:4]))
    (l0, m0), (l1, m1) = got["off"][0], got["stream"][0]
    assert abs(l1 - l0) <= TOL * l0 and abs(m1 - m0) <= TOL * m0
    assert np.allclose(got["stream"][2], got["off"][2], rtol=1e-5, atol=1e-7)
    errs = rel_errors(grads_by_name(w, got["stream"][3]), grads_by_name(w, got["off"][3]))
    differ = sum(int(np.sum(a != b)) for a, b in zip(got["stream"][4], got["off"][4]))
    print(f"enable_sync_bn at world size 1 vs no exchange: {differ} decisions differ, worst gradient error / bar", max(errs.values()) / TOL)
    assert differ <= 1e-5 * sum(a.size for a in got["off"][4])
    if differ == 0:
        assert max(errs.values()) <= TOL, errs
