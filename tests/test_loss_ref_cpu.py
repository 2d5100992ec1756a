"""No GPU: the float32 restatement of the focal kernels' formula (tests/loss_ref.py) against the float64 oracle — the
error it reaches is where the elementwise tolerance of tests/test_gpu_loss_edges.py comes from — and the proof that this
tolerance rejects the gradient term the kernels had before."""
import numpy as np
import pytest

import loss_ref as L


def test_restatement_reaches_float32_accuracy_on_the_whole_sweep():
    x = L.sweep_x()
    assert x.min() == -20.0 and x.max() == 20.0 and x.size > 30000
    for key, (loss_err, grad_err) in sorted(L.emu_table().items()):
        print("gamma %.1f ls %.1f pos %d: loss %.3g  gradient %.3g" % (key + (loss_err, grad_err)))
    worst = L.emu_worst()
    print("EMU_WORST %.4g  ELEM_RTOL %.4g" % (worst, L.elem_rtol()))
    # a handful of float32 roundings, and |x| 2^-24 carried into the exponent of e^-|x| (1.2e-6 at |x| = 20)
    assert 2.0 ** -24 < worst and L.elem_rtol() == 4 * worst <= L.ELEM_RTOL_LIMIT


@pytest.mark.parametrize("gamma", L.GAMMAS)
@pytest.mark.parametrize("pos", [False, True])
def test_label_smoothing_gradient_meets_the_mixed_bound(gamma, pos):
    """with ls != 0 the gradient's two terms have opposite signs over part of the range (p - ys < 0 < ce dmod for a
    confident negative, and the other way round for a positive), so its bound is the mixed one:
    |err| <= rtol |want| + 1e-6 max|want| — here at the restatement's own rtol"""
    x = L.sweep_x()
    m = np.full(x.shape, pos)
    _, got = L.focal_f32(x, m, gamma=gamma, ls=0.1)
    _, want = L.truth(x, m, gamma, 0.1)
    assert (np.abs(got - want) <= L.mixed_bound(want, L.emu_worst())).all()


@pytest.mark.parametrize("gamma", L.GAMMAS)
def test_old_gradient_form_misses_the_tolerance_for_confident_positives(gamma):
    """mod * (p - ys) in float32: p - 1 loses -(1 - p).  From x = 8 on the error is above ELEM_RTOL (on all but the few
    points where 1 - p happens to be a multiple of 2^-24), from x ~ 17 it is the whole term: 1 / (1 + gamma)."""
    x = L.sweep_x()
    x = x[x >= 8.0]
    m = np.ones(x.shape, bool)
    _, want = L.truth(x, m, gamma, 0.0)
    old = L.rel_err(L.focal_f32(x, m, gamma=gamma, form="old")[1], want)
    new = L.rel_err(L.focal_f32(x, m, gamma=gamma, form="fixed")[1], want)
    rtol = L.elem_rtol()
    print("gamma %.1f positives x >= 8: old form worst %.3g, above ELEM_RTOL at %.1f %%; fixed form worst %.3g"
          % (gamma, old.max(), 100 * (old > rtol).mean(), new.max()))
    assert new.max() <= L.emu_worst()
    assert (old > rtol).mean() > 0.95
    assert old[x >= 18.0].min() == pytest.approx(1.0 / (1.0 + gamma), rel=1e-3)
    # negatives never had the problem: the two forms agree bit for bit there
    xn = L.sweep_x()
    mn = np.zeros(xn.shape, bool)
    assert np.array_equal(L.focal_f32(xn, mn, gamma=gamma, form="old")[1], L.focal_f32(xn, mn, gamma=gamma)[1])


@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_fixed_form_keeps_the_bits_of_p_minus_ys_where_nothing_cancels(ls):
    """the new term replaces p - ys only for a positive with x > 4; every negative and every positive up to x = 4 keeps
    the bits of the old form, which is still as accurate there as the rest of the formula"""
    x = L.sweep_x()
    for gamma in L.GAMMAS:
        neg = np.zeros(x.shape, bool)
        assert np.array_equal(L.focal_f32(x, neg, gamma=gamma, ls=ls, form="old")[1], L.focal_f32(x, neg, gamma=gamma, ls=ls)[1])
        xn = x[x <= L.SWITCH_X]
        pos = np.ones(xn.shape, bool)
        assert np.array_equal(L.focal_f32(xn, pos, gamma=gamma, ls=ls, form="old")[1], L.focal_f32(xn, pos, gamma=gamma, ls=ls)[1])
    # and the old form is accurate there
    pos = np.ones(xn.shape, bool)
    _, want = L.truth(xn, pos, 1.5, 0.0)
    assert L.rel_err(L.focal_f32(xn, pos, form="old")[1], want).max() <= L.emu_worst()
