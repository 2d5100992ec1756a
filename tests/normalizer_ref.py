"""float32 restatement of the moving-average loss normaliser (reference retinanet/losses/retinanet_loss.py:38-44):
Keras' moving_average_update under TF2, state.assign_sub((state - v) * (1 - momentum)) — three float32 operations, each
rounded on its own, no zero-debias.  numpy only: neither the package nor the oracle is imported here."""
import numpy as np

F32 = np.float32


def ema_step(state, v, momentum):
    """-> the new state = the normaliser of this call, as np.float32"""
    state, v = F32(state), F32(v)
    d = F32(F32(1.0) - F32(momentum))
    diff = F32(state - v)
    prod = F32(diff * d)
    return F32(state - prod)


def ema_step_fused(state, v, momentum):
    """The same update with the product left unrounded in front of the last subtraction, as a fused multiply-add leaves
    it: the float64 product of two float32 values is exact, and the difference is rounded to float32 once.  NOT the
    reference's arithmetic: the tests use it to show that the three-rounding form can be told from it."""
    state, v = F32(state), F32(v)
    d = F32(F32(1.0) - F32(momentum))
    diff = F32(state - v)
    return F32(np.float64(state) - np.float64(diff) * np.float64(d))


def value(counts):
    """sum(num-positives) + 1 as float32: exact in any order for integer-valued counts whose sum stays below 2^24"""
    total = int(np.asarray(counts, dtype=np.float64).sum())
    assert total + 1 < 1 << 24 and np.all(np.asarray(counts) == np.round(counts))
    return F32(total + 1)


def sequence(values, momentum, state=0.0):
    """the states after each of `values`, fed back"""
    out = []
    for v in values:
        state = ema_step(state, v, momentum)
        out.append(state)
    return np.asarray(out, dtype=F32)


def bits(x):
    return np.asarray(x, dtype=F32).reshape(-1).view(np.uint32)


def seed0_values(steps=2000):
    """the sequence both test files replay: v = f32(rng.integers(0, 20000) + 1), np.random.default_rng(0)"""
    rng = np.random.default_rng(0)
    return [F32(int(rng.integers(0, 20000)) + 1) for _ in range(steps)]
