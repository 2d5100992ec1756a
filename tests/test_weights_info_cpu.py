"""CPU: what Executor._run_training_loop writes for --enable_weights_info, with a stub engine whose weights_info returns a
fixed dict: the keys and cadence of train/weights.jsonl, histogram rows only at multiples of 50 * steps_per_execution,
nothing with the flag off, nothing on a rank that is not the chief, one warning for non-finite values.  The loop is the
real one; the model, the data and the device are stubs."""
import json
import logging
import os
from types import SimpleNamespace

import numpy as np
import torch

NAMES = ["conv2d/kernel", "batch_normalization/gamma", "box-head/box-predict/bias"]


class StubEngine:
    def __init__(self, nonfinite=(0, 0, 0)):
        self.calls = []
        self.nonfinite = nonfinite

    def weights_info(self, histogram=False, bucket_count=30):
        self.calls.append(histogram)
        counts = np.zeros((3, bucket_count), dtype=np.int32)
        counts[:, 0], counts[:, -1], counts[1, 4] = 2, 3, 7
        return {"names": list(NAMES), "norm": np.float32([1.5, 0.0, 2.25]), "min": np.float32([-1.0, 0.0, -0.5]),
                "max": np.float32([1.0, 0.0, 0.5]), "nonfinite": np.asarray(self.nonfinite, dtype=np.int32),
                "counts": counts if histogram else None}


def _executor(tmp_path, monkeypatch, *, flag, rank=0, train_steps=6, spe=2, engine=None):
    from retinanet.executor import Executor
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ex = Executor.__new__(Executor)
    ex.params = SimpleNamespace(training=SimpleNamespace(recovery=SimpleNamespace(use_inflection_detector=False)))
    ex.distribute_strategy = SimpleNamespace(rank=rank)
    ex.run_mode, ex.restore_checkpoint, ex.restore_status = "train", False, None
    ex.optimizer = SimpleNamespace(iterations=0, lr=lambda step: 0.01)
    ex.train_steps, ex.steps_per_execution, ex.val_freq = train_steps, spe, -1
    ex.save_every, ex._save_during_training, ex._run_evaluation_at_end = 0, False, False
    ex.model_dir, ex.summary_dir, ex.name = str(tmp_path / "model"), str(tmp_path / "tb"), "run"
    ex.batch_size = {"train": 4}
    ex.use_float16 = False
    ex._summary_writers, ex._current_trial, ex._max_trials = {}, 1, 1
    ex._model = SimpleNamespace(device="cpu")
    ex._train_dataset = lambda: iter(())
    ex._save = lambda name: None
    ex.enable_weights_info, ex._warned_nonfinite = flag, False
    ex._engine = engine or StubEngine()

    def step(iterator, n):
        ex.optimizer.iterations += int(n)
        return {"weighted-loss": 1.0, "l2-regularization": 0.5}
    ex.distributed_train_step = step
    return ex


def _rows(tmp_path, name):
    path = os.path.join(str(tmp_path), "tb", "run", "train", name)
    return [json.loads(l) for l in open(path)] if os.path.exists(path) else None


def test_weights_rows_follow_the_scalar_rows(tmp_path, monkeypatch):
    ex = _executor(tmp_path, monkeypatch, flag=True, train_steps=5, spe=2)
    assert ex._run_training_loop()
    scalars, weights = _rows(tmp_path, "scalars.jsonl"), _rows(tmp_path, "weights.jsonl")
    assert [r["step"] for r in scalars] == [r["step"] for r in weights] == [2, 4, 5]
    for r in weights:
        assert sorted(r) == sorted(["step"] + ["weights/%s_norm" % k for k in NAMES])
        assert r["weights/conv2d/kernel_norm"] == 1.5 and r["weights/batch_normalization/gamma_norm"] == 0.0
    assert sorted(scalars[0]) == sorted(["step", "weighted-loss", "l2-regularization", "execution-time", "learning-rate"])
    assert _rows(tmp_path, "histograms.jsonl") is None and ex._engine.calls == [False, False, False]


def test_histograms_only_at_multiples_of_50_executions(tmp_path, monkeypatch):
    ex = _executor(tmp_path, monkeypatch, flag=True, train_steps=202, spe=2)
    assert ex._run_training_loop()
    assert [r["step"] for r in _rows(tmp_path, "weights.jsonl")] == list(range(2, 203, 2))
    hist = _rows(tmp_path, "histograms.jsonl")
    assert [r["step"] for r in hist] == [100] * 3 + [200] * 3
    assert [r["name"] for r in hist[:3]] == NAMES
    assert sorted(hist[0]) == ["counts", "max", "min", "name", "nonfinite", "step"]
    r = hist[1]
    assert len(r["counts"]) == 30 and r["counts"][0] == 2 and r["counts"][4] == 7 and r["counts"][29] == 3
    assert r["min"] == 0.0 and r["max"] == 0.0 and r["nonfinite"] == 0
    assert all(isinstance(c, int) for c in r["counts"])
    assert ex._engine.calls == [s % 100 == 0 for s in range(2, 203, 2)]


def test_flag_off_writes_nothing_and_never_asks(tmp_path, monkeypatch):
    ex = _executor(tmp_path, monkeypatch, flag=False, train_steps=100, spe=1)
    assert ex._run_training_loop()
    assert len(_rows(tmp_path, "scalars.jsonl")) == 100
    assert _rows(tmp_path, "weights.jsonl") is None and _rows(tmp_path, "histograms.jsonl") is None
    assert ex._engine.calls == []


def test_only_the_chief_writes(tmp_path, monkeypatch):
    ex = _executor(tmp_path, monkeypatch, flag=True, rank=1, train_steps=50, spe=1)
    assert ex._run_training_loop()
    assert not os.path.exists(os.path.join(str(tmp_path), "tb")) and ex._engine.calls == []


def test_one_warning_names_the_variable(tmp_path, monkeypatch, caplog):
    ex = _executor(tmp_path, monkeypatch, flag=True, train_steps=3, spe=1, engine=StubEngine(nonfinite=(0, 0, 5)))
    with caplog.at_level(logging.WARNING):
        assert ex._run_training_loop()
    hits = [r for r in caplog.records if "Non-finite" in r.getMessage()]
    assert len(hits) == 1 and NAMES[2] in hits[0].getMessage()
