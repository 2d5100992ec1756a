"""CPU: `training.gradient_accumulation_steps` on the host side — how the key is read, the micro-batch the input pipeline and
the Executor derive from it, and the refusals."""
import glob
import os

import pytest
import torch

from conftest import ROOT


def _params(batch, steps=None):
    from retinanet.cfg import default_params
    p = default_params(input_size=128, batch_train=batch)
    if steps is not None:
        p.training.gradient_accumulation_steps = steps
    return p


def test_default_is_one_when_the_key_is_absent():
    from retinanet.cfg import Config, default_params, gradient_accumulation_steps
    assert "gradient_accumulation_steps" not in default_params().training
    assert gradient_accumulation_steps(default_params()) == 1
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_configs", "*", "*.json")))
    assert len(files) >= 10
    for f in files:                               # the reference's configs do not know the key
        p = Config(f).params
        assert "gradient_accumulation_steps" not in p.training and gradient_accumulation_steps(p) == 1, f
    assert gradient_accumulation_steps(_params(256, 4)) == 4


@pytest.mark.parametrize("bad", [0, -2, 2.0, "2", True])
def test_the_key_is_an_integer_of_at_least_one(bad):
    from retinanet.cfg import gradient_accumulation_steps
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        gradient_accumulation_steps(_params(256, bad))


def test_engine_refuses_a_count_below_one():
    from retinanet.model.train_engine import TrainEngine
    with pytest.raises(ValueError, match="accumulation_steps"):
        TrainEngine(None, 2, accumulation_steps=0)


@pytest.mark.parametrize("batch,replicas,steps", [(256, 3, 4), (6, 1, 4), (256, 2, 5), (2, 2, 2)])
def test_indivisible_batch_names_all_three_numbers(batch, replicas, steps):
    from retinanet import Executor
    from retinanet.cfg import micro_batch_size
    from retinanet.dataloader import InputPipeline
    from retinanet.dataloader.input_pipeline import InputContext
    for call in (lambda: micro_batch_size(batch, replicas, steps),
                 lambda: Executor.train_micro_batch_size(_params(batch, steps), replicas),
                 lambda: InputPipeline("train", _params(batch, steps), False, replicas).micro_batch_size(
                     InputContext(replicas, 0, replicas))):
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        if batch % replicas and "num_replicas_in_sync" in msg:      # the pipeline's own per-replica check came first
            continue
        assert str(batch) in msg and f"{replicas} replicas" in msg and f"{steps} gradient accumulation steps" in msg, msg


@pytest.mark.parametrize("batch,replicas,steps,micro", [(256, 2, 4, 32), (6, 1, 3, 2), (256, 8, 1, 32), (64, 1, 1, 64)])
def test_micro_batch_of_the_pipeline_and_the_executor(batch, replicas, steps, micro):
    from retinanet import Executor
    from retinanet.dataloader import InputPipeline
    from retinanet.dataloader.input_pipeline import InputContext
    p = _params(batch, steps if steps > 1 else None)
    ctx = InputContext(replicas, 0, replicas) if replicas > 1 else None
    assert Executor.train_micro_batch_size(p, replicas) == micro
    train = InputPipeline("train", p, False, replicas)
    assert train.accumulation_steps == steps and train.micro_batch_size(ctx) == micro
    # `val` is unchanged: the per-replica share of batch_size.val, whatever the key says
    val = InputPipeline("val", p, False, replicas)
    assert val.micro_batch_size(ctx) == p.training.batch_size["val"] // replicas


def test_train_step_on_an_accumulating_engine_raises():
    """train_step is one batch, one optimizer step: with N > 1 it refuses before it touches anything (no device needed to
    see that), and names the call to make instead"""
    from retinanet.model.train_engine import TrainEngine
    eng = object.__new__(TrainEngine)
    eng.accumulation_steps = 2
    with pytest.raises(RuntimeError, match="train_step_accumulated"):
        eng.train_step(torch.zeros((2, 128, 128, 3)), {})


def test_mean_loss_dict():
    from retinanet.model.train_engine import mean_loss_dict
    outs = [{"weighted-loss": torch.tensor(1.0), "l2-regularization": torch.tensor(5.0), "iou-prediction-loss": 0.0},
            {"weighted-loss": torch.tensor(2.0), "l2-regularization": torch.tensor(7.0), "iou-prediction-loss": 0.0},
            {"weighted-loss": torch.tensor(6.0), "l2-regularization": torch.tensor(9.0), "iou-prediction-loss": 0.0}]
    out = mean_loss_dict(outs)
    assert float(out["weighted-loss"]) == 3.0 and float(out["l2-regularization"]) == 9.0 and out["iou-prediction-loss"] == 0.0
