"""Synchronised BatchNormalization for run-time-shaped trainers, the parts that need no GPU: the new entry point's place in the
ABI, the training class asking for the exchange whatever the crop size, and the identity tests/test_gpu_sync_bn_shapes.py stands
on (a batch of shuffled copies has the base batch's step) for the run-time shapes it uses."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import helpers as H  # noqa: F401
import train_plans as TP
from cellscreen import _lib as L
from oracle import train_oracle as T
from test_dist_cpu import _RankTrainer, _free_port


def test_the_stream_ordered_entry_point_is_part_of_the_abi():
    """cs_train_set_sync_bn_stream is exported, bound with the blocking entry point's arguments, and refuses a NULL handle with
    CS_ERR_INVALID; so does the blocking one, and neither needs a device for that."""
    lib = L.load_library()
    assert "cs_train_set_sync_bn_stream" in L.SIGNATURES and hasattr(lib, "cs_train_set_sync_bn_stream")
    assert L.SIGNATURES["cs_train_set_sync_bn_stream"] == L.SIGNATURES["cs_train_set_sync_bn"]
    cb = L.ALLGATHER_STREAM_FN(lambda ctx, fpr, stream: 0)
    for fn in (None, C.cast(cb, C.c_void_p)):
        assert lib.cs_train_set_sync_bn_stream(None, fn, None, None, 0, 0, 1) == -1          # CS_ERR_INVALID
        assert b"NULL" in lib.cs_last_error()
    assert lib.cs_train_set_sync_bn(None, None, None, None, 0, 0, 1) == -1
    assert lib.cs_abi_version() == 2


def _train_worker(rank, world, port, outdir, q):
    import torch.distributed as dist
    from cellscreen import training
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    training.Trainer = _RankTrainer
    _RankTrainer.rank = rank
    _RankTrainer.script = {0: [1.0, 0.9, 0.8], 1: [1.0, 0.95, 0.9]}
    t = training.ImprovedAnomalyDetectionTraining(os.path.join(outdir, f"r{rank}"), epochs=3, verbose=0, augment=None, data_parallel=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        t.train_autoencoder(np.zeros((100, 64, 128), np.float32))
    tr = _RankTrainer.instances[-1]
    q.put((rank, getattr(tr, "sync", None), [str(w.message) for w in seen if "BatchNormalization" in str(w.message) or "sync_bn" in str(w.message)]))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_training_synchronises_batchnorm_for_64x128_crops(tmp_path):
    """World 2 on gloo, 64 x 128 training cells: the training class asks its trainer for the exchange with (rank, 2) on both ranks
    and raises no warning about per-rank statistics (it did both only for the 64 x 64 reference graph before)."""
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_train_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in range(2)])
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    assert [g[1] for g in got] == [(0, 2), (1, 2)], got
    assert [g[2] for g in got] == [[], []], got


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("i", [6, len(TP.GENERIC_CASES) - 1], ids=["32x64", "config4"])
def test_eight_shuffled_copies_of_a_run_time_shaped_base_batch_have_its_step(i):
    """What the GPU test takes its exact reference from: the float64 oracle on k = 8 shuffled copies of the 3 base cells of a
    run-time-shaped case against the float64 oracle on the 3 cells -- loss, MAE, batch statistics and every gradient at 1e-10
    relative (the same bar as the reference graph's identity in tests/test_train_plans_cpu.py)."""
    hw, ch, ne, _why = TP.GENERIC_CASES[i]
    assert i < len(TP.GENERIC_CASES) - 1 or (hw, ch, ne) == TP.CONFIG4
    w = TP.weights(TP.WSEED + ne, hw=hw, channels=ch, n_enc=ne)
    x, y = TP.mixed_batch(TP.GENERIC_BASE, 40 + i, hw)
    xb, yb, idx = TP.replicate(x, y, 8, seed=4)
    assert len(xb) == 24 and sorted(idx.tolist()) == sorted(np.repeat(np.arange(3), 8).tolist())
    base = T.forward_backward(T.TrainState(w), x, y)
    big = T.forward_backward(T.TrainState(w), xb, yb)
    figures = {"loss": abs(big["loss"] - base["loss"]) / base["loss"], "mae": abs(big["mae"] - base["mae"]) / base["mae"]}
    for j, (a, c) in enumerate(zip(big["grads"], base["grads"])):
        figures[f"gradient {j}"] = _rel(a, c)
    for l in range(w.n_conv - 1):
        figures[f"mean {l}"] = _rel(big["batch_mean"][l], base["batch_mean"][l])
        figures[f"variance {l}"] = _rel(big["batch_var"][l], base["batch_var"][l])
    worst = max(figures, key=figures.get)
    print(f"replication identity, {hw} {ch}: worst", worst, figures[worst])
    assert figures[worst] <= 1e-10, (worst, figures[worst])
