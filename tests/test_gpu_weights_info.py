"""TrainEngine.weights_info and the Executor's --enable_weights_info files on the GPU: ResNet-14 at 128 x 128, B = 2.
Engine level: names, norms and histogram counts against stats_ref.py on the engine's own master weights, before and after
a training step, with `resnet_initial` frozen, and the bits of a training step with and without a call in front of it.
Executor level: train/weights.jsonl next to scalars.jsonl, train/histograms.jsonl only when the step is a multiple of
50 * steps_per_execution, neither with the flag off."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import stats_ref as S

pytestmark = pytest.mark.gpu
SIZE, B = 128, 2


def _engine(cuda, freeze):
    from test_gpu_train_step import _setup
    p, model, eng, targets, images = _setup(cuda, SIZE, B, True, seed=7, depth=14, freeze=freeze)
    model.optimizer.lr = lambda step: 0.01
    return p, model, eng, targets, images.to(cuda)


@pytest.fixture(scope="module")
def shared(cuda):
    """one engine with every variable trainable, for the tests of this module"""
    return _engine(cuda, False)


def _check(eng, info, buckets=30):
    """info against the float64 reference of the engine's own P"""
    chunk = int(eng.lib.rn_optim_chunk())
    P = eng.P.cpu().numpy()
    assert info["names"] == list(eng.train_names) and len(info["names"]) == eng.n_segs
    assert info["norm"].dtype == np.float32 and info["nonfinite"].dtype == np.int32 and info["counts"].dtype == np.int32
    assert info["counts"].shape == (eng.n_segs, buckets)
    worst = 0.0
    for i, k in enumerate(info["names"]):
        off, n = eng.p_off[k]
        r = S.stats(P[off:off + n], buckets)
        bound, _ = S.norm_bound(n, chunk)
        err = abs(float(info["norm"][i]) - float(r["norm"]))
        assert err <= bound * float(r["norm"]), (k, info["norm"][i], r["norm"], bound)
        worst = max(worst, err / (bound * float(r["norm"])) if r["norm"] else 0.0)
        assert info["min"][i] == r["min"] and info["max"][i] == r["max"] and info["nonfinite"][i] == r["nonfinite"] == 0, k
        assert (info["counts"][i] == r["counts"]).all(), (k, info["counts"][i].tolist(), r["counts"].tolist())
        assert int(info["counts"][i].sum()) == n, k
    print(f"{len(info['names'])} variables, worst norm error / bound = {worst:.3g}")


def test_weights_info_matches_the_reference_before_and_after_a_step(cuda, shared):
    p, model, eng, targets, images = shared
    info0 = eng.weights_info(histogram=True)
    _check(eng, info0)
    plain = eng.weights_info()
    assert plain["counts"] is None and plain["names"] == info0["names"]
    for key in ("norm", "min", "max", "nonfinite"):
        assert plain[key].tobytes() == info0[key].tobytes(), key           # the same bits on every call
    w0 = eng.P.clone()
    eng.train_step(images, targets)
    torch.cuda.synchronize()
    info1 = eng.weights_info(histogram=True)
    _check(eng, info1)
    # a variable that trained reports another norm wherever the step moved its float64 norm by more than the two results'
    # error bounds together (a smaller move may round to the same float32)
    chunk, P1 = int(eng.lib.rn_optim_chunk()), eng.P.cpu().numpy()
    moved, told = 0, 0
    for i, k in enumerate(eng.train_names):
        off, n = eng.p_off[k]
        if torch.equal(eng.P[off:off + n], w0[off:off + n]):
            assert info1["norm"][i] == info0["norm"][i], k
            continue
        moved += 1
        r0, r1 = float(S.norm(w0[off:off + n].cpu().numpy())), float(S.norm(P1[off:off + n]))
        if abs(r1 - r0) > 2 * S.norm_bound(n, chunk)[0] * max(r0, r1):
            told += 1
            assert info1["norm"][i] != info0["norm"][i], (k, r0, r1)
    print(f"{moved} of {eng.n_segs} variables moved, {told} by more than the bounds")
    assert moved > 0 and told > 0
    info64 = eng.weights_info(histogram=True, bucket_count=64)
    _check(eng, info64, 64)
    with pytest.raises(ValueError):
        eng.weights_info(histogram=True, bucket_count=65)


def test_a_training_step_keeps_its_bits(cuda, shared, tmp_path):
    """two steps from a checkpoint, then the same two steps from the same checkpoint with a weights_info call in front of
    each: the same losses and the same bits in every arena"""
    p, model, eng, targets, images = shared
    prefix = str(tmp_path / "weights_step_0")
    eng.save_checkpoint(prefix)
    torch.cuda.synchronize()
    start = eng.P.clone()

    def two_steps(ask):
        eng.restore_checkpoint(prefix)
        losses = []
        for _ in range(2):
            if ask:
                arenas = [t.clone() for t in (eng.P, eng.G, eng.V, eng.E, eng.Pbf)]
                eng.weights_info(histogram=True)
                for t, was in zip((eng.P, eng.G, eng.V, eng.E, eng.Pbf), arenas):
                    assert torch.equal(t.view(torch.int16), was.view(torch.int16))      # every arena untouched
            losses.append(eng.train_step(images, targets)["weighted-loss"].item())
        torch.cuda.synchronize()
        return losses, [t.clone() for t in (eng.P, eng.V, eng.E, eng.Pbf)]

    want, state = two_steps(False)
    got, state2 = two_steps(True)
    assert got == want and not torch.equal(state[0], start)
    for x, y in zip(state, state2):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


def test_frozen_variables_are_not_reported(cuda, shared):
    from retinanet.model import ModelBuilder
    everything = shared[2].train_names
    p, model, eng, _, _ = _engine(cuda, True)
    assert list(p.training.freeze_variables) == ["resnet_initial"]
    rx = ModelBuilder.FREEZE_VARS_REGEX["resnet_initial"]
    info = eng.weights_info(histogram=True)
    assert info["names"] == list(eng.train_names) == [k for k in everything if not rx.search(k)]
    for k in ("conv2d/kernel", "batch_normalization/gamma", "conv2d_1/kernel", "conv2d_4/kernel", "batch_normalization_4/beta"):
        assert k in everything and k not in info["names"], k                 # the stem and block group 1
    assert not any(k.endswith(("moving_mean", "moving_variance")) for k in info["names"])
    _check(eng, info)


# ---- Executor -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from test_gpu_executor import _dataset
    tmp_path = tmp_path_factory.mktemp("weights_info")
    return tmp_path, _dataset(tmp_path)


def _run(cuda, data, tag, flag, train_steps, spe):
    from test_gpu_executor import _params
    from retinanet import Executor
    from retinanet.dataloader import InputPipeline
    from retinanet.distribute import get_strategy
    from retinanet.model import ModelBuilder
    tmp_path, ann = data
    p = copy.deepcopy(_params(tmp_path, ann))
    p.experiment.model_dir = str(tmp_path / tag / "model_files")
    p.experiment.tensorboard_dir = str(tmp_path / tag / "tensorboard")
    p.training.train_steps, p.training.steps_per_execution, p.training.save_every = train_steps, spe, 1000
    ex = Executor(params=p, strategy=get_strategy(p.training.strategy), run_mode="train",
                  model_builder=ModelBuilder(p, "train", device=cuda), train_input_fn=InputPipeline("train", p, False, 1, device=cuda),
                  enable_weights_info=flag)
    eng = ex._engine
    zero = {k for k in eng.train_names if not bool(eng._pview(k).any())}       # zero-initialised: gammas, biases
    ex.run()
    out = os.path.join(p.experiment.tensorboard_dir, "tiny", "train")
    rows = {}
    for name in ("scalars", "weights", "histograms"):
        path = os.path.join(out, name + ".jsonl")
        rows[name] = [json.loads(l) for l in open(path)] if os.path.exists(path) else None
    return ex, rows, zero


def test_executor_writes_a_weights_row_per_logging_point(cuda, data):
    ex, rows, zero = _run(cuda, data, "three", True, 3, 2)
    assert [r["step"] for r in rows["scalars"]] == [r["step"] for r in rows["weights"]] == [2, 3]
    names = ex._engine.train_names
    assert zero and len(zero) < len(names)
    for r in rows["weights"]:
        assert sorted(r) == sorted(["step"] + ["weights/%s_norm" % k for k in names])
        for k in names:
            v = r["weights/%s_norm" % k]
            assert np.isfinite(v) and v >= 0.0 and (v > 0.0 or k in zero), (k, v)
    assert rows["histograms"] is None                                        # step 3 is no multiple of 50 * 2
    assert "weights/" not in " ".join(rows["scalars"][0])                    # scalars.jsonl keeps its keys


def test_executor_writes_histograms_every_fifty_executions(cuda, data):
    ex, rows, _ = _run(cuda, data, "fifty", True, 50, 1)
    eng = ex._engine
    assert [r["step"] for r in rows["weights"]] == list(range(1, 51))
    hist = rows["histograms"]
    assert [r["name"] for r in hist] == list(eng.train_names) and {r["step"] for r in hist} == {50}
    P = eng.P.cpu().numpy()
    for r in hist:
        off, n = eng.p_off[r["name"]]
        assert len(r["counts"]) == 30 and sum(r["counts"]) + r["nonfinite"] == n, r["name"]
        want = S.stats(P[off:off + n])                                       # the weights the run ended with
        assert r["counts"] == want["counts"].tolist() and r["min"] == float(want["min"]) and r["max"] == float(want["max"])


def test_executor_flag_off_writes_neither_file(cuda, data):
    ex, rows, _ = _run(cuda, data, "off", False, 1, 1)
    assert [r["step"] for r in rows["scalars"]] == [1] and rows["weights"] is None and rows["histograms"] is None
    assert ex._engine._wi is None                                            # nothing allocated, nothing launched
