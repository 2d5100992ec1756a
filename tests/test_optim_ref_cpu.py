"""optim_ref.py without a GPU: known answers of the float64 reference, the layout builder against the engine's rules, the
margins of every input set the GPU tests use, and the acceptance rule against a float32 emulation of rn_optim.hip — the
right one is accepted, each single fault is rejected by name."""
import math

import numpy as np
import pytest
import torch

import optim_ref as O

F32 = np.float32


@pytest.fixture(scope="module")
def chunk():
    return O.chunk()


@pytest.fixture(scope="module")
def lay_a(chunk):
    return O.layout_a(chunk)


@pytest.fixture(scope="module")
def lay_b(chunk):
    return O.layout_b(chunk)


# ---- known answers ------------------------------------------------------------------------------------------------------
def _tiny(chunk):
    lay = O.build_layout([2, 2], [1, 0], [True, False], chunk)
    w = torch.full((lay.total,), O.SENTINEL)
    g = torch.full((lay.total,), O.SENTINEL)
    w[4:6] = torch.tensor([1.0, 1.0])
    g[4:6] = torch.tensor([5.0, 7.0])
    w[8:10] = torch.tensor([9.0, 9.0])
    g[8:10] = torch.tensor([1.5, 2.0])
    return lay, O.Inputs(w, g, 2.0, 0.5, 0.5, 0.125)


def test_layout_known_answer(chunk):
    lay = O.build_layout([5, 3, 8, chunk + 1], [1, 0, 1, 1], [True, False, True, False], chunk)
    assert lay.segs["offset"].tolist() == [4, 12, 16, 24] and lay.segs["bf"].tolist() == [0, -1, 8, -1]
    assert lay.segs["bb"].tolist() == [0, 1, 2, 3] and lay.segs["nb"].tolist() == [1, 1, 1, 2]
    assert lay.block_seg.tolist() == [0, 1, 2, 3, 3]
    end = 24 + chunk + 1
    total = (end + 3) // 4 * 4 + 4
    assert lay.total == total and lay.total16 == 16 + 8
    assert lay.untouched.tolist() == [0, 1, 2, 3, 9, 10, 11, 15] + list(range(end, total))
    assert lay.untouched16.tolist() == [5, 6, 7] + list(range(16, 24))
    assert lay.elem[:9].tolist() == [4, 5, 6, 7, 8, 12, 13, 14, 16] and lay.seg[:9].tolist() == [0] * 5 + [1] * 3 + [2]
    assert lay.copies() == [(4, 0, 5), (16, 8, 8)]


def test_layouts_cover_what_the_issue_names(lay_a, lay_b, chunk):
    s = lay_a.segs
    assert lay_a.n_segs == 300 and 350000 < lay_a.total < 450000
    for n in (chunk, chunk + 1, chunk - 1, 3 * chunk + 5, 9 * chunk + 2, 17 * chunk - 3, 1, 2, 3, 4, 5, 6, 7):
        assert n in s["size"]
    assert s["size"][O.NINE] == 9 * chunk + 2 and O.NINE >= 256 and s["nb"][O.NINE] == 10
    assert s["wd"][O.NAN_AT] == 0 and O.NAN_AT >= 256
    assert (s["offset"] % 4 == 0).all() and s["offset"][0] == 4 and (s["bf"][s["bf"] >= 0] % 8 == 0).all()
    assert ((s["wd"] == 1) & (s["bf"] < 0)).any() and ((s["wd"] == 0) & (s["bf"] >= 0)).sum() == 1
    assert (s["bf"] != s["offset"]).all()                      # the engine's layout: the two arenas do not line up
    b = lay_b.segs
    assert (b["offset"] % 4 != 0).sum() >= 4 and b["offset"][1] % 4 != 0 and b["nb"][1] == 3
    assert b["offset"][O.B_MIXED] % 4 == 0 and b["bf"][O.B_MIXED] % 4 != 0 and b["nb"][O.B_MIXED] == 2


def test_reference_known_answers(chunk):
    lay, inp = _tiny(chunk)
    t = O.stage1(lay, inp.g, inp.w, inp.wdc, inp.unscale)
    assert t.value.tolist() == [3.0, 4.0, 0.75, 1.0] and t.terms.tolist() == [3.0, 4.0, 0.75, 1.0]
    c = O.clip_factors(lay, t.value, inp.w, inp.clip, inp.alpha)
    assert c.norm.tolist() == pytest.approx([5.0, 1.25], rel=1e-15)
    assert c.f.tolist() == pytest.approx([0.4, 1.0], rel=1e-15)
    # the global norm is over the CLIPPED norms (2, 1.25), not (5, 1.25)
    assert c.gn == pytest.approx(math.sqrt(5.5625), rel=1e-15) and c.F == pytest.approx(2.0 / math.sqrt(5.5625), rel=1e-15)
    assert c.metrics[0] == pytest.approx(2.0, rel=1e-15) and c.metrics[3] == pytest.approx(0.125, rel=1e-15)   # alpha/2 * 2
    assert c.metrics[4:6] == [1.0, 0.0] and c.flags == (1.0, 0.0)
    e = O.eps(chunk)
    g1 = O.clipped(lay, t.value, c, e).value
    assert g1.tolist() == pytest.approx([x * 2.0 / math.sqrt(5.5625) for x in (1.2, 1.6, 0.75, 1.0)], rel=1e-15)
    cor = O.correction(lay, t.value, c, e).value
    assert (t.value + cor).tolist() == pytest.approx(g1.tolist(), rel=1e-15)
    # clip off, and nothing fires
    off = O.clip_factors(lay, t.value, inp.w, 0.0, inp.alpha)
    assert off.f.tolist() == [1.0, 1.0] and off.F == 1.0 and off.gn == pytest.approx(math.sqrt(26.5625), rel=1e-15)
    assert off.metrics[4:6] == [0.0, 0.0] and off.flags == (0.0, 0.0)
    none = O.clip_factors(lay, t.value, inp.w, 8.0, inp.alpha)
    assert none.factor.tolist() == [1.0, 1.0] and none.flags == (0.0, 0.0)
    assert O.correction(lay, t.value, none, e).bound(None).tolist() == [0.0] * 4


def test_sgd_known_answers(chunk):
    lay = O.build_layout([1], [1], [True], chunk)
    a = lambda x: torch.tensor([0, 0, 0, 0, x, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32)
    w1, v1, e1 = O.sgd(lay, a(1.0), a(2.0), a(0.5), a(2.0), 0.25, 0.5, 0.75, 0)
    assert (v1.value.item(), w1.value.item(), e1.value.item()) == (-0.25, 0.75, 1.6875)
    assert (v1.terms.item(), w1.terms.item(), v1.n, w1.n, e1.n) == (0.75, 1.75, 3, 4, 7)
    w1, v1, e1 = O.sgd(lay, a(1.0), a(2.0), a(0.5), None, 0.25, 0.5, 0.0, 1)
    assert (v1.value.item(), w1.value.item(), w1.n, e1) == (-0.25, 0.375, 7, None)    # 1 + 0.5 * (-0.25) - 0.5
    w1, v1, _ = O.sgd(lay, a(1.0), a(2.0), a(0.5), None, 0.25, 0.0, 0.0, 0)
    assert (v1.value.item(), w1.value.item()) == (-0.5, 0.5)
    # the scalars enter as float32 values: 0.1 is not 0.1
    assert O.f32(0.1) != 0.1 and O.f32(0.1) == float(F32(0.1))
    _, _, e1 = O.sgd(lay, a(0.0), a(0.0), a(0.0), a(1.0), 0.0, 0.0, 0.9998, 0)
    assert e1.value.item() == 1.0 - float(F32(1.0) - F32(0.9998))


def test_eps_chain(chunk):
    e, u = O.eps(chunk), 2.0 ** -24
    k = chunk // 256 + 1
    assert e.sq == k * 2.0 ** -23 + O.EPS_D and e.norm == e.sq / 2 + u + O.EPS_D and e.f == e.norm + u
    assert e.gn == e.norm + e.f + 2 * u + O.EPS_D and e.ft == e.f + e.gn + 2 * u
    assert e.m0 < 1e-3 / 50      # the input margin is far outside every bound of the chain


# ---- input margins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(O.REGIMES))
@pytest.mark.parametrize("seed", [0, 1])
def test_input_margins(lay_a, regime, seed):
    """float32 and float64 cannot disagree on which factor fires: every norm is farther than 1e-3 clip from clip"""
    inp = O.make_inputs(lay_a, regime, seed)
    assert O.margins(lay_a, inp) > 1e-3
    t = O.stage1(lay_a, inp.g, inp.w, inp.wdc, inp.unscale).value
    c = O.clip_factors(lay_a, t, inp.w, inp.clip, inp.alpha)
    per, glob = int((c.f != 1.0).sum()), c.F != 1.0
    want = {"off": (0, False), "none": (0, False), "only257": (1, True), "global": (0, True)}.get(regime)
    if want:
        assert (per, glob) == want
    else:
        assert 50 < per < 250 and glob
    if regime == "only257":
        assert c.f[O.ALONE] != 1.0


def test_input_margins_of_the_two_ranks(lay_a):
    for inp, fires in zip(O.two_ranks(lay_a), (True, False)):
        assert O.margins(lay_a, inp) > 1e-3
        t = O.stage1(lay_a, inp.g, inp.w, inp.wdc, inp.unscale).value
        assert (O.clip_factors(lay_a, t, inp.w, inp.clip, inp.alpha).flags[0] == 1.0) == fires


# ---- float32 emulation of the kernels, right and with single faults -----------------------------------------------------
def _block_sum(x, chunk):
    """one block: 256 threads add the squares of their 16-byte groups in fp32, then double"""
    p = np.zeros((chunk,), dtype=F32)
    p[:x.size] = x
    p = p.reshape(-1, 256, 4)
    acc = np.zeros((256,), dtype=F32)
    for it in range(p.shape[0]):
        for l in range(4):
            acc = acc + p[it, :, l] * p[it, :, l]
    return float(acc.astype(np.float64).sum())


def emu_clip(lay, inp, fault=None):
    """(stage-1 arena, clipped arena, correction arena, metrics[6], flags) as float32 arithmetic produces them"""
    g, w, ch = inp.g.numpy().copy(), inp.w.numpy(), lay.chunk
    part, part_w = np.zeros((lay.n_blocks,)), np.zeros((lay.n_blocks,))
    wdc = F32(inp.alpha) if fault == "wdc_alpha" else F32(inp.wdc)
    for s in lay.segs:
        o, n = int(s["offset"]), int(s["size"])
        t = g[o:o + n] * F32(inp.unscale)
        if s["wd"]:
            t = t + wdc * w[o:o + n]
        g[o:o + n] = t
        for b in range(int(s["nb"])):
            part[s["bb"] + b] = _block_sum(t[b * ch:(b + 1) * ch], ch)
            if s["wd"]:
                part_w[s["bb"] + b] = _block_sum(w[o + b * ch:o + min(n, (b + 1) * ch)], ch)
    t_arena = g.copy()
    if fault == "drop_block":
        part[int(lay.segs["bb"][O.NINE]) + 4] = 0.0
    clip = F32(inp.clip)
    factor = np.ones((lay.n_segs,), dtype=F32)
    tot = totw = 0.0
    fired = False
    for i, s in enumerate(lay.segs):
        if fault == "stop_at_256" and i >= 256:
            continue
        norm = F32(math.sqrt(part[s["bb"]:s["bb"] + s["nb"]].sum()))
        f = clip / max(norm, clip) if clip > 0 else F32(1.0)
        factor[i] = f
        fired |= bool(f != 1.0)
        cn = norm if fault == "global_of_unclipped" else norm * f
        tot += float(cn) * float(cn)
        totw += part_w[s["bb"]:s["bb"] + s["nb"]].sum()
    gn = F32(math.sqrt(tot))
    Fg = clip / max(gn, clip) if clip > 0 else F32(1.0)
    finite = bool(np.isfinite(gn))
    metrics = [float(gn * Fg), float(gn), float(Fg), float(F32(0.5 * float(F32(inp.alpha)) * totw)),
               float(fired or Fg != 1.0), float(not finite)]
    flags = (float(metrics[4] != 0.0 or not finite), metrics[5])
    n_mul = 256 if fault == "stop_at_256" else lay.n_segs
    factor[:n_mul] = factor[:n_mul] * Fg
    cor = np.full_like(g, O.SENTINEL)
    for i, s in enumerate(lay.segs):
        o, n = int(s["offset"]), int(s["size"])
        c = factor[i] if fault == "correction_f" else factor[i] - F32(1.0)
        cor[o:o + n] = c * t_arena[o:o + n]
        if factor[i] != 1.0:
            g[o:o + n] = g[o:o + n] * factor[i]
    return torch.from_numpy(t_arena), torch.from_numpy(g), torch.from_numpy(cor), torch.tensor(metrics), torch.tensor(flags)


@pytest.fixture(scope="module")
def clip_runs(lay_a):
    """the right emulation of every regime, once"""
    return {r: (O.make_inputs(lay_a, r), ) + emu_clip(lay_a, O.make_inputs(lay_a, r)) for r in O.REGIMES}


def _clip_ratios(lay, inp, t, g, cor, metrics, flags):
    out = dict(O.verify_stage1(lay, inp, t))
    out.update(O.verify_clip(lay, inp, t, g, metrics, flags))
    out.update(O.verify_correction(lay, inp, t, cor))
    return out


@pytest.mark.parametrize("regime", list(O.REGIMES))
def test_rule_accepts_the_float32_emulation(lay_a, clip_runs, regime):
    inp, t, g, cor, metrics, flags = clip_runs[regime]
    ratios = _clip_ratios(lay_a, inp, t, g, cor, metrics, flags)
    print(regime, ratios)
    assert O.worst(ratios) <= 1.0, ratios
    if regime in ("off", "none"):
        assert torch.equal(g, t) and not cor[lay_a.elem].any()


# fault -> (regime that shows it, a check that must reject it)
CLIP_FAULTS = {"global_of_unclipped": ("both", "metrics[1]"), "wdc_alpha": ("none", "stage1"),
               "stop_at_256": ("only257", "G"), "correction_f": ("both", "correction"),
               "drop_block": ("off", "metrics[1]")}


@pytest.mark.parametrize("fault", list(CLIP_FAULTS))
def test_rule_rejects_clip_fault(lay_a, fault):
    regime, where = CLIP_FAULTS[fault]
    inp = O.make_inputs(lay_a, regime)
    ratios = _clip_ratios(lay_a, inp, *emu_clip(lay_a, inp, fault))
    assert ratios[where] > 1.0, (fault, ratios)


def test_rule_rejects_identity_faults(lay_a):
    """two synthetic ranks: the sum of the unclipped gradients plus the corrections; f * g for (f - 1) * g breaks it"""
    inps = O.two_ranks(lay_a)
    for fault, ok in ((None, True), ("correction_f", False)):
        ts, total = [], None
        for inp in inps:
            t, _, cor, _, _ = emu_clip(lay_a, inp, fault)
            ts.append(t)
            total = (t, cor) if total is None else (total[0] + t, total[1] + cor)
        r = O.verify_identity(lay_a, inps, ts, total[0] + total[1])
        assert (O.worst(r) <= 1.0) == ok, (fault, r)


def _sgd_case(lay, seed=0):
    inp = O.make_inputs(lay, "none", seed)
    v, dlt = O.sgd_state(lay, seed)
    e = inp.w.clone()
    e[lay.elem] += dlt[lay.elem]
    pbf = torch.full((lay.total16,), O.SENTINEL16, dtype=torch.bfloat16)
    return inp.w, inp.g, v, e, pbf


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("nesterov,m", [(0, 0.9), (1, 0.9), (0, 0.0)])
def test_rule_accepts_the_sgd_emulation(lay_a, lay_b, which, nesterov, m):
    lay = lay_a if which == "a" else lay_b
    w, g, v, e, pbf = _sgd_case(lay)
    lr, m, d = O.f32(0.1), O.f32(m), O.f32(0.9998)
    for step in range(2):
        w1, v1, e1, p1 = O.emu_sgd(lay, w, g, v, e, pbf, lr, m, d, nesterov)
        r = O.verify_sgd(lay, (w, v, e), (w1, v1, e1), g, lr, m, d, nesterov, pbf, p1)
        assert O.worst(r) <= 1.0, (step, r)
        w, v, e, pbf = w1, v1, e1, p1


SGD_FAULTS = {"nesterov_old_v": (1, "w"), "ema_swapped": (0, "ema"), "copy_truncates": (0, "16-bit copy")}


@pytest.mark.parametrize("fault", list(SGD_FAULTS))
def test_rule_rejects_sgd_fault(lay_a, fault):
    nesterov, where = SGD_FAULTS[fault]
    w, g, v, e, pbf = _sgd_case(lay_a)
    lr, m, d = O.f32(0.1), O.f32(0.9), O.f32(0.9998)
    w1, v1, e1, p1 = O.emu_sgd(lay_a, w, g, v, e, pbf, lr, m, d, nesterov, fault)
    r = O.verify_sgd(lay_a, (w, v, e), (w1, v1, e1), g, lr, m, d, nesterov, pbf, p1)
    assert r[where] > 1.0, (fault, r)


def test_rule_rejects_a_write_into_padding(lay_a):
    """a tail loop one element too long: the slot behind a tensor no longer holds what it held"""
    inp = O.make_inputs(lay_a, "none")
    t, g, cor, metrics, flags = emu_clip(lay_a, inp)
    o, n = lay_a.rng(62)                     # 3 elements: one padding float behind it
    assert n - o == 3
    g = g.clone()
    g[n] = 0.0
    assert O.verify_clip(lay_a, inp, t, g, metrics, flags)["G untouched"] > 1.0
