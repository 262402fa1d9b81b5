"""bench.py's options and --dump-outputs writer, without a GPU: the arrays of the last step go out as float32 / float64, a
seeded sample of cells when they exceed the size limit, and --steps sets the timed steps."""
import os
import sys

import numpy as np
import pytest

import helpers as H

sys.path.insert(0, H.ROOT)
torch = pytest.importorskip("torch")
import bench  # noqa: E402


def _results(n):
    idx = np.arange(n)
    return dict(mse=torch.from_numpy((idx * 0.5).astype(np.float32)), mae=torch.from_numpy((idx * 0.25).astype(np.float32)),
                cons_score=torch.from_numpy(idx - 3.0), mod_score=torch.from_numpy(-idx.astype(np.float64)),
                cons_pred=torch.from_numpy(np.where(idx % 3 == 0, -1, 1).astype(np.int8)),
                mod_pred=torch.from_numpy(np.where(idx % 2 == 0, -1, 1).astype(np.int8)))


def test_dump_writes_every_result_of_the_step(tmp_path):
    res = _results(1000)
    bench.dump_outputs(str(tmp_path / "out"), res, 42)
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(k + ".npy" for k in res)
    for k, v in res.items():
        a = np.load(tmp_path / "out" / (k + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == (1000,)
        assert np.array_equal(a, v.numpy().astype(a.dtype)), k
    assert np.load(tmp_path / "out" / "cons_score.npy").dtype == np.float64


def test_dump_above_the_limit_is_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    res = _results(1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, 7)
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))      # 128-byte .npy headers
    assert total <= 4000
    idx = np.load(tmp_path / "a" / "cell_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 4000 // (32 + 8) and np.all(np.diff(idx) > 0)
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "mse.npy"), res["mse"].numpy()[i])
    assert np.array_equal(np.load(tmp_path / "a" / "mod_pred.npy"), res["mod_pred"].numpy()[i].astype(np.float32))


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + bad)
        with pytest.raises(SystemExit):
            bench.parse()
