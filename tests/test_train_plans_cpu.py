"""What tests/test_gpu_train_batches.py stands on, checked without a GPU: the replicated-batch identity at float64 rounding,
and that its batch list gives every training launch an uncapped grid and a grid that goes round at least three times with a
ragged last round (tests/train_plans.py)."""
import numpy as np
import pytest

import generic_plans as GP
import helpers as H  # noqa: F401
import train_plans as TP
from oracle import train_oracle as T


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


def _mx(a, b):
    return float(np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("b,k", [(7, 5), (5, 13)])
def test_a_batch_of_shuffled_copies_has_the_base_batch_step(b, k):
    """The float64 oracle on k shuffled copies of b cells against the float64 oracle on the b cells: loss, MAE, batch statistics, all
    26 gradients, k dz, k da, relu and the output per copy, at 1e-10 relative (measured: 2.5e-12 and 5.7e-12 at worst)."""
    w = TP.weights(TP.WSEED)
    x, y = TP.mixed_batch(b, 100 + b)
    xb, yb, idx = TP.replicate(x, y, k, seed=b)
    assert sorted(idx.tolist()) == sorted(np.repeat(np.arange(b), k).tolist()) and not np.array_equal(idx, np.tile(np.arange(b), k))
    base = T.forward_backward(T.TrainState(w), x, y)
    big = T.forward_backward(T.TrainState(w), xb, yb)
    figures = {"loss": abs(big["loss"] - base["loss"]) / base["loss"], "mae": abs(big["mae"] - base["mae"]) / base["mae"]}
    for i, (a, c) in enumerate(zip(big["grads"], base["grads"])):
        figures[f"gradient {i}"] = _rel(a, c)
    for l in range(6):
        figures[f"mean {l}"] = _mx(big["batch_mean"][l], base["batch_mean"][l])
        figures[f"variance {l}"] = _mx(big["batch_var"][l], base["batch_var"][l])
        figures[f"relu {l}"] = _mx(big["relu"][l], base["relu"][l][idx])
        figures[f"k da {l}"] = _mx(k * big["da"][l], base["da"][l][idx])
    for l in range(7):
        figures[f"k dz {l}"] = _mx(k * big["dz"][l], base["dz"][l][idx])
    figures["out"] = _mx(big["out"], base["out"][idx])
    worst = max(figures, key=figures.get)
    print("replication identity, worst:", worst, figures[worst])
    assert figures[worst] <= 1e-10, (worst, figures[worst])


def test_the_restated_thresholds():
    """The restatement against the figures the kernels' comments and launchers state."""
    L = {l.name: l for l in TP.reference_launches()}
    second_item = lambda l: next(b for b in range(1, 10000) if l.rounds(b, l.caps[0]) >= 2)
    assert [second_item(L[n]) for n in ("wgrad_first_kernel", "wgrad_mfma_kernel<WgL2>", "wgrad_mfma_kernel<WgL3>", "wgrad_mfma_kernel<WgL4>",
                                        "wgrad_mfma_kernel<WgL5>", "wgrad_mfma_kernel<WgL6>", "wgrad_last_kernel")] == [33, 33, 65, 129, 65, 33, 33]
    # the BatchNormalization backward grids reach BN_MAX_PARTS at 128 / 512 / 2,048 cells on the 32 / 16 / 8 grids
    capped_from = lambda l: next(b for b in range(1, 10000) if l.grid(b, l.caps[0]) == l.caps[0])
    assert [capped_from(L[f"bn_bwd_dz_kernel[{l}]"]) for l in range(6)] == [128, 512, 2048, 2048, 512, 128]
    assert [capped_from(L[f"bn_apply_kernel[{l}]"]) for l in (0, 5)] == [128, 128]
    # the forward convs: at most BN_MAX_PARTS * 64 / COUT partials, whatever the occupancy
    assert max(L["conv_mfma_kernel<CfgF1>"].caps) == 2048 and max(L["conv_mfma_kernel<CfgF2>"].caps) == 1024
    assert max(L["conv_mfma_kernel<CfgF4>"].caps) == 2048          # one strip per cell: 6,149 cells are more than three rounds
    assert TP.bias7_partials(TP.TRAIN_MAX_BATCH) == TP.BN_MAX_PARTS * 64 // 2      # train_api.hip:31: the buffer's capacity exactly
    assert TP.TRAIN_MAX_BATCH in TP.BATCHES and TP.TRAIN_MAX_BATCH + 1 not in TP.BATCHES


def test_the_batch_list_reaches_every_training_launch_uncapped_and_looping():
    """Every launch of the reference graph's step, under every occupancy the bound allows: (a) some batch of the list leaves its
    grid uncapped, (b) some batch makes it go round at least three times with a ragged last round."""
    launches = TP.reference_launches()
    assert len(launches) == 6 + 6 + 1 + 6 + 12 + 7
    for L in launches:
        a, b = TP.coverage(L, TP.BATCHES)
        assert a, f"{L.name}: no batch of {TP.BATCHES} leaves the grid uncapped under every cap of {L.caps}"
        assert b, f"{L.name}: no batch of {TP.BATCHES} gives three rounds and a ragged last one under every cap of {L.caps}"
    # ragged rounds are impossible only where a cell's pixels are a multiple of the grid cap
    assert sorted(L.name for L in launches if not L.ragged_possible) == sorted(f"{k}[{l}]" for k in ("bn_bwd_reduce_kernel", "bn_bwd_dz_kernel") for l in (0, 5))
    # bn_stats_final merges as many partials as the forward conv has workgroups: the list reaches both ends of that too
    for l in range(6):
        for cap in launches[l].caps:
            g = [TP.stats_partials(l, b, cap) for b in TP.BATCHES]
            assert min(g) < 256 and max(g) == cap
    # the sequence of test_batch_size_changes_on_one_handle grows, shrinks, grows and returns
    s = TP.RESIZE_SEQUENCE
    assert s[1] > s[0] and s[2] < s[0] and s[3] > s[1] and s[4] == s[0]


def test_every_generic_training_case_has_a_looping_batch():
    """The run-time-shaped trainer: for each trainer-accepted sweep case and BASELINE configs[4]'s shape, the batch train_plans
    picks makes the forward, backward-data and weight-gradient launches go round at least three times with a ragged end, within
    4 GB of batch buffers."""
    assert len(TP.TRAIN_CASES) >= 5 and TP.GENERIC_CASES[-1][:3] == TP.CONFIG4
    assert GP.describe_trainer(*TP.CONFIG4) is None
    for hw, ch, ne, _why in TP.GENERIC_CASES:
        b, k = TP.generic_batch(hw, ch, ne)
        launches = TP.generic_launches(hw, ch, ne)
        assert len(launches) == 3 * len(ch) - 1
        for L in launches:
            (cap,) = L.caps
            assert L.rounds(b * k, cap) >= 3 and L.ragged(b * k, cap), (hw, ch, L.name, b * k)
        assert TP.generic_train_bytes(hw, ch, ne, b * k) <= 4 << 30, (hw, ch, b * k)
        assert (hw, ch) in TP.GENERIC_FP32_ORACLE
    # the 128 x 128 / 128-filter shape: above every layer's weight-gradient part count
    b, k = TP.generic_batch(*TP.CONFIG4)
    assert all(L.items(b * k) > L.caps[0] for L in TP.generic_launches(*TP.CONFIG4) if L.kind == "chunked")


@pytest.mark.parametrize("b", sorted(TP.BASE_SEED))
def test_the_base_batches_keep_their_decisions_in_float32(b):
    """The float32 numpy oracle against the float64 one on each base batch: the share of ReLU decisions on which they differ.  The
    GPU tests cap the TRAINER's share at 1e-5; the base batches of 7, 8 and 13 cells are chosen (seeds fixed in train_plans) so that
    even numpy's float32 evaluation, whose batch statistics add the rows one after another in float32, stays within it.  No 32-cell
    batch does (28 weight / batch seeds tried: 1.8e-5 .. 5.9e-5; the share grows with the rows summed, 1.5e-4 at 161 cells): for
    that base the figure is held below 3e-5 here and the 1e-5 cap is the GPU test's own assertion on the trainer.  The recorded
    dz / da figures (FP32_ORACLE, the GPU tests' bars over 4) are this evaluation's."""
    x, y = TP.mixed_batch(b, TP.BASE_SEED[b])
    dz, da, share = TP.fp32_oracle_figures(TP.weights(TP.WSEED), x, y)
    print(f"base batch of {b} cells: float32 / float64 oracle decisions differ on a share of {share:.2e}")
    assert share <= (1e-5 if b < 32 else 3e-5)
    assert np.allclose(dz, TP.FP32_ORACLE[b][0], rtol=0.06) and np.allclose(da, TP.FP32_ORACLE[b][1], rtol=0.06), (dz, da)
