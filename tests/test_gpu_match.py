"""The label scoring on the device (cs_label_match through cellscreen.score, and ThresholdSegmenter.score_batch) against the CPU
restatement of tests/match_reference.py, which tests/test_match_cpu.py holds to a brute force and to an assignment solver.

Every output is an integer table, so every comparison is np.array_equal: no tolerances.

The counting pass tiles as ex_label_pass does: a lane owns 4 columns, a wave 256 columns x 16 rows, a workgroup 64 rows; a width
that is no multiple of 4 takes the scalar loads.  PAIRS crosses each of these one short, equal and one past.  Its table in LDS
holds 1024 pairs per tile (16 probes), the many-pairs field overfills it and sends the rest to the global table directly."""
import numpy as np
import pytest

import match_reference as MR
import segment_reference as R
from cellscreen import _lib as L
from cellscreen import score as SC
from cellscreen import segment as S

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260]
HEIGHTS = [65, 64, 63, 17, 16, 15, 2, 1, 17, 65, 63]    # every height of {1, 2, 15, 16, 17, 63, 64, 65}; no pair is square
PAIRS = list(zip(HEIGHTS, WIDTHS))


@pytest.fixture(scope="module")
def matcher():
    m = SC.LabelMatcher(0)
    yield m
    m.close()


def as_tensor(a):
    import torch
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def contents(shape, seed):
    """(pred [6,H,W], truth [6,H,W]): Voronoi labels against a shifted copy, identical images, pred all 0, truth all 0, ids with
    gaps (whose largest is the batch's max exactly), and disconnected objects."""
    H, W = shape
    n = max(1, min(24, H * W // 6))
    a = MR.voronoi(shape, n, seed, 0.25)
    b = MR.shifted(a, 1 if H > 1 else 0, -2 if W > 2 else 0)
    z = np.zeros_like(a)
    gaps_p, gaps_t = (b * 5).astype(np.int32), (a * 3).astype(np.int32)
    fold = max(1, n // 2)
    disc = np.where(a > fold, a - fold, a).astype(np.int32)             # two cells far apart share a label
    return np.stack([b, a, z, a, gaps_p, disc]), np.stack([a, a.copy(), a, z, gaps_t, b])


def check(m, pred, truth, mp, mt):
    pt, tt, n = MR.tables(pred, truth, mp, mt)
    assert m.pred.dtype == np.int32 and m.truth.dtype == np.int32 and m.n_pairs.dtype == np.int64
    assert np.array_equal(m.pred, pt) and np.array_equal(m.truth, tt) and np.array_equal(m.n_pairs, n)


@pytest.mark.parametrize("shape", PAIRS)
def test_tables_equal_the_restatement(matcher, shape):
    pred, truth = contents(shape, 7 * shape[0] + shape[1])
    mp, mt = max(1, int(pred.max())), max(1, int(truth.max()))
    m = matcher.match_batch(pred, truth)                                # the arrays' own maxima: a label equals its max exactly
    assert m.pred.shape == (6, mp, 4) and m.truth.shape == (6, mt, 4)
    check(m, pred, truth, mp, mt)
    assert not m.pred[2].any() and not m.truth[3].any()                 # rows of absent labels are all zeros
    check(matcher.match_batch(pred, truth, max_pred=mp + 3, max_truth=mt + 1), pred, truth, mp + 3, mt + 1)


def test_batch_equals_images_one_by_one(matcher):
    shape = (70, 130)
    pred = np.stack([MR.shifted(MR.voronoi(shape, n, n, 0.2), 1, 2) for n in (3, 17, 40)])
    truth = np.stack([MR.voronoi(shape, n, n, 0.2) for n in (3, 17, 40)])
    whole = matcher.match_batch(pred, truth, max_pred=40, max_truth=41)
    check(whole, pred, truth, 40, 41)
    for b in range(3):
        one = matcher.match_batch(pred[b:b + 1].copy(), truth[b:b + 1].copy(), max_pred=40, max_truth=41)
        assert np.array_equal(one.pred[0], whole.pred[b]) and np.array_equal(one.truth[0], whole.truth[b]) and one.n_pairs[0] == whole.n_pairs[b]
    assert len({int(v) for v in whole.n_pairs}) == 3


def many_pairs():
    yy, xx = np.mgrid[0:64, 0:64]
    pred = (yy * 64 + xx + 1).astype(np.int32)[None]                    # every pixel its own label
    truth = ((yy // 2) * 32 + xx // 2 + 1).astype(np.int32)[None]       # 2 x 2 blocks
    return pred, truth


def test_many_pairs_fill_the_lds_table_and_growth_gives_the_same(matcher):
    pred, truth = many_pairs()
    auto = matcher.match_batch(pred, truth)
    check(auto, pred, truth, 4096, 1024)
    assert int(auto.n_pairs[0]) == 4096 and matcher.last_table() == (16, 0)
    small = SC.LabelMatcher(0, extractor=matcher, table_log2=10)        # 1,024 slots for 4,096 pairs: must grow
    grown = small.match_batch(pred, truth)
    log2, grows = small.last_table()
    assert grows >= 1 and log2 == 10 + grows and log2 >= 13
    assert np.array_equal(grown.pred, auto.pred) and np.array_equal(grown.truth, auto.truth) and np.array_equal(grown.n_pairs, auto.n_pairs)


def test_same_call_twice_is_bit_identical_and_times_are_finite(matcher):
    pred, truth = contents((65, 257), 3)
    a, b = matcher.match_batch(pred, truth), matcher.match_batch(pred, truth)
    assert np.array_equal(a.pred, b.pred) and np.array_equal(a.truth, b.truth) and np.array_equal(a.n_pairs, b.n_pairs)
    t = matcher.last_timing()
    assert set(t) == {"match_count_ms", "match_reduce_ms"} and all(np.isfinite(v) and v >= 0.0 for v in t.values())


def test_input_kinds(matcher):
    pred, truth = contents((33, 260), 9)
    mp, mt = int(pred.max()), int(truth.max())
    for p, t in ((pred, truth), (as_tensor(pred), as_tensor(truth)), (pred, as_tensor(truth)), (as_tensor(pred), truth)):
        check(matcher.match_batch(p, t), pred, truth, mp, mt)
    import torch
    with pytest.raises(ValueError):
        matcher.match_batch(as_tensor(pred)[:, :, ::2], as_tensor(truth)[:, :, ::2])
    with pytest.raises(TypeError):
        matcher.match_batch(as_tensor(pred).to(torch.int64), truth)


def test_bad_labels_are_an_error_status_and_the_handle_stays_usable(matcher):
    pred, truth = contents((17, 65), 4)
    mp, mt = int(pred.max()), int(truth.max())
    for which, value in (("pred", mp + 1), ("pred", -1), ("truth", mt + 1), ("truth", -1)):
        p, t = pred.copy(), truth.copy()
        (p if which == "pred" else t)[1, 16, 64] = value
        with pytest.raises(L.CellScreenError) as ei:
            matcher.match_batch(p, t, max_pred=mp, max_truth=mt)
        assert ei.value.status == -1
        check(matcher.match_batch(pred, truth, max_pred=mp, max_truth=mt), pred, truth, mp, mt)


def test_score_batch_chains_on_the_segmenter_s_handle():
    rng = np.random.default_rng(2)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    imgs = np.empty((2, H, W), np.uint16)
    truth = np.zeros((2, H, W), np.int32)
    for b in range(2):
        f = 300.0 + rng.normal(0.0, 10.0, (H, W))
        for k, (y, x, r) in enumerate(((20, 25, 9), (30, 80, 12), (70, 40, 10), (72, 100, 7 + 4 * b), (50, 62, 5))):
            f += 4000.0 * np.exp(-(((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (r / 1.6) ** 2)) ** 2)
            if k < 4:                                                   # the fifth blob has no truth: a false positive
                truth[b][(yy - y - 1) ** 2 + (xx - x) ** 2 <= r * r] = k + 1
        imgs[b] = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
    truth[1][5:9, 5:9] = 5                                              # and a truth object nothing predicts
    seg = S.ThresholdSegmenter(0)
    want_lab, want_n, _ = R.segment_batch(imgs)
    want = MR.stats(MR.tables(want_lab, truth, int(want_n.max()), 5), (0.5, 0.7, 0.9))
    for images, tr in ((imgs, truth), (as_tensor(imgs.view(np.int16)), as_tensor(truth)), (imgs, as_tensor(truth))):
        labels, n_labels, _ = seg.segment_batch(images)
        assert "match_count_ms" not in seg.last_timing()
        stats, lab2, n2 = seg.score_batch(images, tr, thresholds=(0.5, 0.7, 0.9))
        to_np = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
        assert np.array_equal(to_np(lab2), to_np(labels)) and np.array_equal(to_np(labels), want_lab) and np.array_equal(n2, n_labels)
        assert stats == want
        t = seg.last_timing()
        assert {"match_count_ms", "match_reduce_ms", "threshold_ms", "label_ms"} <= set(t) and all(np.isfinite(v) and v >= 0.0 for v in t.values())
    assert want["total"]["by_threshold"][0]["tp"] == 8 and want["total"]["by_threshold"][0]["fp"] == 2 and want["total"]["by_threshold"][0]["fn"] == 1
    seg.close()
