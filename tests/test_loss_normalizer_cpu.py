"""CPU: the moving-average loss normaliser (loss.normalizer.use_moving_average) — known answers of the reference's
float32 arithmetic, proof that the restatement tells the fused form apart, and the construction of RetinaNetLoss."""
import logging

import numpy as np

import normalizer_ref as N


def test_known_answers_of_the_three_rounding_update():
    """From state 0 with momentum 0.99 and v = 8, 1, 33 (no zero-debias: the first normaliser is ~0.01 v)."""
    states = N.sequence([8.0, 1.0, 33.0], 0.99)
    assert [hex(b) for b in N.bits(states)] == ["0x3da3d700", "0x3db6ae72", "0x3ed62c6a"]
    assert abs(float(states[0]) - 0.0799999237) < 1e-9
    # d itself is a rounded float32 operation: 1 - f32(0.99) is not f32(0.01)
    assert np.float32(1.0) - np.float32(0.99) != np.float32(0.01)


def test_edge_momenta():
    """momentum 0: the normaliser is v itself whenever state - v is exact; momentum 1: the state never moves"""
    assert N.ema_step(0.0, 41.0, 0.0) == np.float32(41.0) and N.ema_step(7.0, 41.0, 0.0) == np.float32(41.0)
    assert N.ema_step(0.0, 41.0, 1.0) == np.float32(0.0) and N.ema_step(7.5, 41.0, 1.0) == np.float32(7.5)
    assert N.ema_step(0.0, 41.0, 0.5) == np.float32(20.5)


def test_value_is_the_exact_count_plus_one():
    assert N.value([0.0, 3.0, 15999.0]) == np.float32(16003.0)
    assert N.value([0.0]) == np.float32(1.0)


def test_the_reference_form_differs_from_the_fused_form():
    """2000 steps from state 0, v = f32(rng.integers(0, 20000) + 1), momentum 0.99: leaving the product unrounded in front
    of the last subtraction (float64 product, one rounding) gives other bits at some steps (5 of them, measured), so a
    kernel that contracts the update cannot pass the bit comparison of tests/test_gpu_loss_normalizer.py."""
    values = N.seed0_values(2000)
    state, differ = np.float32(0.0), 0
    for v in values:
        want = N.ema_step(state, v, 0.99)
        fused = N.ema_step_fused(state, v, 0.99)
        differ += int(want.view(np.uint32) != fused.view(np.uint32))
        state = want
    print("steps at which the fused form differs:", differ)
    assert differ >= 1


def test_retinanet_loss_constructs_with_the_option(caplog):
    """NotImplementedError before this feature"""
    from retinanet.cfg import default_params
    from retinanet.losses import RetinaNetLoss
    p = default_params()
    p.loss.normalizer.use_moving_average = True
    with caplog.at_level(logging.WARNING):
        loss = RetinaNetLoss(80, p.loss)
    assert loss.use_moving_average_normalizer and loss.normalizer_momentum == 0.99
    assert loss.moving_average_normalizer is None      # a device scalar: made by the first call, at 0.0
    assert "Using moving average loss normalizer with momentum: 0.99" in caplog.text
    off = RetinaNetLoss(80, default_params().loss)
    assert not off.use_moving_average_normalizer and off.moving_average_normalizer is None


def test_begin_step_can_leave_the_c2_slot_empty():
    """SmallMessages.begin_step(carry_normalizer=False) is the state has_carrier = False produces: nothing pending, nothing
    rode, and no launch (lib is None here: a launch would raise)"""
    import torch
    from retinanet.model.data_parallel import SmallMessages
    small = SmallMessages(None, torch.device("cpu"), None, 2, True)
    small._c2_local = small.c2_normalizer = torch.zeros(1)
    small.begin_step(torch.tensor([3.0, 4.0]), carry_normalizer=False)
    assert small._c2_local is None and small.c2_normalizer is None and small.count == 0
