"""GPU: the Executor with `training.optimizer.name: adam` — the configuration file is all a user changes.  It trains,
writes `Adam/iter` and the `m` / `v` / `vhat` slots into its checkpoints, and a second Executor resumes from them on the same
bits."""
import copy
import os

import pytest
import torch

from test_gpu_executor import _dataset, _params

pytestmark = pytest.mark.gpu


def _executor(p, cuda):
    from retinanet import Executor
    from retinanet.dataloader import InputPipeline
    from retinanet.distribute import get_strategy
    from retinanet.model import ModelBuilder
    return Executor(params=p, strategy=get_strategy(p.training.strategy), run_mode="train",
                    model_builder=ModelBuilder(p, "train", device=cuda),
                    train_input_fn=InputPipeline("train", p, False, 1, device=cuda))


def test_executor_trains_and_resumes_with_adam(cuda, tmp_path):
    from retinanet import tf_checkpoint
    p = _params(tmp_path, _dataset(tmp_path))
    p.experiment.run_mode = "train"
    opt = p.training.optimizer
    for k in ("momentum", "nesterov"):            # Keras' Adam takes neither
        del opt[k]
    opt.name, opt.amsgrad = "Adam", True
    opt.lr_params.warmup_learning_rate = opt.lr_params.initial_learning_rate = 1e-3
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        ex = _executor(p, cuda)
        eng = ex._engine
        assert ex.optimizer.name == "adam" and eng.S1 is not None and eng.S2 is not None
        w0 = eng.P.clone()
        ex.run()
        assert int(ex.optimizer.iterations) == 3 and eng.step_count == 3
        assert not torch.equal(w0, eng.P) and torch.isfinite(eng.P).all() and eng.S1.any() and eng.S2.any()
        mdir = os.path.join(p.experiment.model_dir, p.experiment.name)
        prefix = tf_checkpoint.latest_checkpoint(mdir)
        assert prefix.endswith("final_weights_step_3")
        arrays, slots = tf_checkpoint.load_weights(prefix)
        assert int(arrays["Adam/iter"]) == 3 and "SGD/iter" not in arrays
        k0 = eng.train_names[0]
        assert {s for (k, s) in slots if k == k0} == {"m", "v", "vhat", "average"}
        p2 = copy.deepcopy(p)
        p2.training.train_steps = 4
        ex2 = _executor(p2, cuda)
        assert int(ex2.optimizer.iterations) == 3
        for a, b in ((ex2._engine.P, eng.P), (ex2._engine.V, eng.V), (ex2._engine.S1, eng.S1), (ex2._engine.S2, eng.S2),
                     (ex2._engine.E, eng.E)):
            assert torch.equal(a, b)
        ex2.run()
        assert int(ex2.optimizer.iterations) == 4 and torch.isfinite(ex2._engine.P).all()
    finally:
        os.chdir(cwd)
