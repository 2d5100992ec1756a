"""accum_ref.py without a GPU: a known answer of the float64 reference, the margins of the micro-step inputs the GPU tests
use, and the acceptance rule against the float32 emulation of the accumulate stage — the right one is accepted, each of
four single faults is rejected by name."""
import numpy as np
import pytest
import torch

import accum_ref as A
import optim_ref as O


@pytest.fixture(scope="module")
def layouts():
    ch = O.chunk()
    return {"a": O.layout_a(ch), "b": O.layout_b(ch)}


def _emulate(lay, inps, faults=None):
    """the three micro-steps in float32: per micro-step (inputs, stage-1 arena, factors, metrics, accumulator before, after);
    faults: micro-step -> fault of emu_accumulate, or "stale_factors" (the factors of the micro-step before)"""
    faults = faults or {}
    acc, runs, last = A.fresh_accumulator(lay), [], None
    for i, inp in enumerate(inps):
        t = A.emu_stage1(lay, inp)
        factors, metrics = A.emu_factors(lay, t, inp)
        fault = faults.get(i)
        used = last if fault == "stale_factors" else factors
        new = A.emu_accumulate(lay, t, used, metrics, acc, i == 0, None if fault == "stale_factors" else fault)
        runs.append((inp, t, factors, metrics, acc, new))
        acc, last = new, factors
    return runs


def test_known_answer():
    """two tensors of two elements, clip 2: norms 5 and 1.25, per-tensor factors 0.4 and 1, global factor 2 / sqrt(5.5625)"""
    lay = O.build_layout([2, 2], [1, 0], [True, False], O.chunk())
    w = torch.full((lay.total,), O.SENTINEL)
    t = torch.full((lay.total,), O.SENTINEL)
    t[4:6], t[8:10], w[4:6], w[8:10] = torch.tensor([3.0, 4.0]), torch.tensor([0.75, 1.0]), 1.0, 9.0
    inp = O.Inputs(w, t, 2.0, 1.0, 0.0, 0.125)
    prev = torch.full((lay.total,), O.SENTINEL)
    prev[4:6], prev[8:10], prev[0:2] = torch.tensor([1.0, -1.0]), torch.tensor([0.5, 0.25]), torch.tensor([0.0, 0.0])
    F = 2.0 / np.sqrt(5.5625)
    ref, c = A.accumulated(lay, inp, t, prev, False)
    assert ref.value.tolist() == pytest.approx([1.0 + 1.2 * F, -1.0 + 1.6 * F, 0.5 + 0.75 * F, 0.25 + F], rel=1e-15)
    assert ref.terms.tolist() == pytest.approx([1.0 + 1.2 * F, 1.0 + 1.6 * F, 0.5 + 0.75 * F, 0.25 + F], rel=1e-15)
    assert ref.n.tolist() == [2.0] * 4 and A.flags_after(prev, c, False) == (1.0, 0.0)
    ref, _ = A.accumulated(lay, inp, t, prev, True)
    assert ref.value.tolist() == pytest.approx([1.2 * F, 1.6 * F, 0.75 * F, F], rel=1e-15) and ref.n.tolist() == [1.0] * 4
    # nothing fires: one rounding for the sum, none for a first micro-step
    off = inp._replace(clip=8.0)
    ref, c = A.accumulated(lay, off, t, prev, False)
    assert ref.value.tolist() == [4.0, 3.0, 1.25, 1.25] and ref.n.tolist() == [1.0] * 4 and not ref.extra.any()
    ref, _ = A.accumulated(lay, off, t, prev, True)
    assert ref.value.tolist() == [3.0, 4.0, 0.75, 1.0] and ref.bound(None).tolist() == [0.0] * 4
    prev[0:2] = torch.tensor([1.0, 1.0])
    assert A.flags_after(prev, c, False) == (1.0, 1.0) and A.flags_after(prev, c, True) == (0.0, 0.0)


@pytest.mark.parametrize("which", ["a", "b"])
def test_input_margins(layouts, which):
    """float32 and float64 agree on which factors fire in every micro-step; the per-tensor factors fire on the second one
    and every factor stays at 1 on the first and the third"""
    lay = layouts[which]
    inps = A.micro_inputs(lay)
    assert len(inps) == 3 and all(torch.equal(x.w, inps[0].w) for x in inps)
    fired = []
    for inp in inps:
        assert O.margins(lay, inp) > 1e-3
        t = O.stage1(lay, inp.g, inp.w, inp.wdc, inp.unscale).value
        c = O.clip_factors(lay, t, inp.w, inp.clip, inp.alpha)
        fired.append((int((c.f != 1.0).sum()), c.F != 1.0, bool((c.factor != 1.0).any())))
    assert fired[0] == (0, False, False) and fired[2] == (0, False, False)
    assert fired[1][0] >= 1 and fired[1][1] and fired[1][0] < lay.n_segs      # some tensors keep their own factor at 1
    assert not torch.equal(inps[0].g, inps[2].g)


@pytest.mark.parametrize("which", ["a", "b"])
def test_rule_accepts_the_float32_emulation(layouts, which):
    lay = layouts[which]
    runs = _emulate(lay, A.micro_inputs(lay))
    for i, (inp, t, factors, metrics, before, after) in enumerate(runs):
        r = A.verify(lay, inp, t, before, after, i == 0, factors, torch.tensor(metrics + [0.0, 0.0]))
        print(which, i, r)
        assert O.worst(r) <= 1.0, (i, r)
        assert bool(torch.isfinite(after[lay.elem]).all()) and bool((after[lay.untouched[2:]] == O.SENTINEL).all())
    assert torch.equal(runs[0][5][lay.elem], runs[0][1][lay.elem])           # first and every factor 1: a copy
    assert [tuple(r[5][0:2].tolist()) for r in runs] == [(0.0, 0.0), (1.0, 0.0), (1.0, 0.0)]
    # the emulated factors are the float64 ones within the chain's allowance
    inp, t, factors = runs[1][0], runs[1][1], runs[1][2]
    c = O.clip_factors(lay, O.pack(lay, t), inp.w, inp.clip, inp.alpha)
    want = c.factor[lay.seg]
    assert float(((factors[lay.elem].double() - want).abs() / want).max()) <= O.eps(lay.chunk).ft


def _not_finite(inps, lay, step=1):
    g = inps[step].g.clone()
    g[lay.rng(5)[0] + 1] = float("inf")
    out = list(inps)
    out[step] = inps[step]._replace(g=g)
    return out


# fault -> (micro-step it is planted in, check that must reject it, checks that must still pass)
FAULTS = {"first_ignored": (0, "A"), "stale_factors": (2, "A"), "flag_overwritten": (2, "A flags"),
          "double_product": (1, "A bits")}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_rule_rejects_fault(layouts, fault):
    lay = layouts["a"]
    at, where = FAULTS[fault]
    inps = A.micro_inputs(lay)
    if fault == "flag_overwritten":
        inps = _not_finite(inps, lay)           # micro-step 1 sets A[1]; micro-step 2 is finite and must keep it
    runs = _emulate(lay, inps, {at: fault})
    inp, t, factors, metrics, before, after = runs[at]
    if fault == "first_ignored":                # a finite stale accumulator, so that the miss is a value and not a NaN
        before = runs[2][5].clone()
        after = A.emu_accumulate(lay, t, factors, metrics, before, True, fault)
    r = A.verify(lay, inp, t, before, after, at == 0, factors, torch.tensor(metrics + [0.0, 0.0]))
    print(fault, r)
    assert r[where] > 1.0, (fault, r)
    if fault == "double_product":               # more exact than the header, not less: the bound alone cannot see it
        assert r["A"] <= 1.0 and r["A flags"] == 0.0
    if fault == "flag_overwritten":
        assert tuple(before[0:2].tolist()) == (1.0, 1.0) and tuple(after[0:2].tolist()) == (1.0, 0.0)
    # the same micro-step without the fault passes
    right = _emulate(lay, inps)[at]
    if fault == "first_ignored":
        good = A.emu_accumulate(lay, t, factors, metrics, before, True)
        ok = A.verify(lay, inp, t, before, good, True, factors, torch.tensor(metrics + [0.0, 0.0]))
    else:
        ok = A.verify(lay, right[0], right[1], right[4], right[5], at == 0, right[2], torch.tensor(right[3] + [0.0, 0.0]))
    if fault != "flag_overwritten":             # (with the planted inf the float64 norms are inf / NaN: only the flags are read)
        assert O.worst(ok) <= 1.0, (fault, ok)
    else:
        assert ok["A flags"] == 0.0


def test_rule_rejects_a_write_outside_the_tensors(layouts):
    lay = layouts["a"]
    inp, t, factors, metrics, before, after = _emulate(lay, A.micro_inputs(lay))[0]
    for idx in (2, 3, lay.rng(62)[1], lay.total - 1):
        bad = after.clone()
        bad[idx] = 0.0
        assert A.verify(lay, inp, t, before, bad, True)["A untouched"] > 1.0, idx
