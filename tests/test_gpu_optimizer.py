"""The five entry points of csrc/rn_optim.hip against the float64 reference of optim_ref.py, on the paths the training
engines run: block ranges with a local copy (the overlapped all-reduce), the in-place correction, more than 256 tensors,
every clip regime, the flags in G[0:2], the skip flag in G[0], two SGD steps on the engine's layout and on offsets it
never produces.  The acceptance rule is derived in optim_ref.py; every test prints |got - ref| / bound per quantity before
it asserts that none exceeds 1.  Slots that are no tensor element hold a sentinel before every launch and must keep it."""
import pytest
import torch

import optim_ref as O

pytestmark = pytest.mark.gpu

_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
LR, DECAY = O.f32(0.1), O.f32(0.9998)


def _lib(build="bf16"):
    from retinanet import _C
    return _C.lib(build == "f16")


@pytest.fixture(scope="module")
def layouts():
    ch = O.chunk()
    return {"a": O.layout_a(ch), "b": O.layout_b(ch)}


class Arena:
    """segment table, block table, a fresh workspace and metrics on the device"""

    def __init__(self, lay, dev, lib):
        self.lay, self.dev, self.lib = lay, dev, lib
        self.segs = torch.from_numpy(lay.segs.view("uint8").copy()).to(dev)
        self.bs = torch.from_numpy(lay.block_seg.copy()).to(dev)
        self.ws = torch.zeros((lib.rn_optim_workspace_bytes(lay.n_blocks, lay.n_segs),), dtype=torch.uint8, device=dev)
        self.metrics = torch.full((8,), O.SENTINEL, dtype=torch.float32, device=dev)

    def clip(self, G, P, inp):
        from retinanet import _C
        _C.check(self.lib.rn_optim_clip(_C.ptr(G), _C.ptr(P), _C.ptr(self.segs), self.lay.n_segs, _C.ptr(self.bs),
                                        self.lay.n_blocks, inp.wdc, inp.alpha, inp.unscale, inp.clip, _C.ptr(self.metrics),
                                        _C.ptr(self.ws), self.ws.numel(), _C.current_stream()), "rn_optim_clip")

    def prepare(self, G, P, inp, local=None, begin=0, count=None):
        from retinanet import _C
        count = self.lay.n_blocks - begin if count is None else count
        _C.check(self.lib.rn_optim_clip_prepare(_C.ptr(G), _C.ptr(P), _C.ptr(self.segs), _C.ptr(self.bs), self.lay.n_blocks,
                                                begin, count, inp.wdc, inp.unscale, _C.ptr(local), _C.ptr(self.ws),
                                                self.ws.numel(), _C.current_stream()), "rn_optim_clip_prepare")

    def factors(self, inp, flags_ptr=None):
        from retinanet import _C
        _C.check(self.lib.rn_optim_clip_factors(_C.ptr(self.segs), self.lay.n_segs, self.lay.n_blocks, inp.clip, inp.alpha,
                                                _C.ptr(self.metrics), flags_ptr, _C.ptr(self.ws), self.ws.numel(),
                                                _C.current_stream()), "rn_optim_clip_factors")

    def apply(self, G, correction=None):
        from retinanet import _C
        _C.check(self.lib.rn_optim_clip_apply(_C.ptr(G), _C.ptr(correction), _C.ptr(self.segs), _C.ptr(self.bs),
                                              self.lay.n_blocks, _C.ptr(self.ws), self.ws.numel(), _C.current_stream()),
                 "rn_optim_clip_apply")

    def sgd(self, P, G, V, E, Pbf, m, nesterov, skip_ptr=None, d=DECAY):
        from retinanet import _C
        _C.check(self.lib.rn_optim_sgd_step(_C.ptr(P), _C.ptr(G), _C.ptr(V), _C.ptr(E), _C.ptr(Pbf), _C.ptr(self.segs),
                                            _C.ptr(self.bs), self.lay.n_blocks, LR, m, d if E is not None else 0.0, nesterov,
                                            skip_ptr, _C.current_stream()), "rn_optim_sgd_step")


def _stage1(lay, cuda, inp):
    """the kernel's own stage-1 arena: G after rn_optim_clip_prepare over all blocks"""
    a = Arena(lay, cuda, _lib())
    t = inp.g.to(cuda)
    a.prepare(t, inp.w.to(cuda), inp)
    torch.cuda.synchronize()
    return t.cpu()


def _report(name, ratios):
    print(name, {k: round(v, 4) for k, v in ratios.items()})
    assert O.worst(ratios) <= 1.0, (name, ratios)


# ---- 1. clip regimes through the one-call entry point --------------------------------------------------------------------
@pytest.mark.parametrize("which,regime", [("a", r) for r in O.REGIMES] + [("b", "off")])
def test_clip_regimes(cuda, layouts, which, regime):
    """layout A in every regime; layout B (offsets 1, 2, 3 mod 4: the scalar loop of the stage-1 kernel) with the clip off,
    where no norm can sit near a threshold"""
    lay = layouts[which]
    inp = O.make_inputs(lay, regime)
    t_dev = _stage1(lay, cuda, inp)
    _report(f"{which}/{regime} stage 1", O.verify_stage1(lay, inp, t_dev))
    a = Arena(lay, cuda, _lib())
    G, P = inp.g.to(cuda), inp.w.to(cuda)
    a.clip(G, P, inp)
    torch.cuda.synchronize()
    _report(f"{which}/{regime} clip", O.verify_clip(lay, inp, t_dev, G, a.metrics))
    assert a.metrics[6:].tolist() == [O.SENTINEL] * 2 and torch.equal(P.cpu(), inp.w)
    G = G.cpu()
    if regime in ("off", "none"):
        assert torch.equal(G, t_dev)                                  # nothing fires: the stage-1 value, bit for bit
        assert inp.unscale == 1.0
        plain = lay.elem[lay.wd == 0]
        assert torch.equal(G[plain], inp.g[plain])                    # not decayed, not unscaled, not clipped: the input
    if regime == "only257":
        o, e = lay.rng(0)
        q, r = lay.rng(O.ALONE)
        # tensor 0 got the global factor alone, tensor 257 its own on top of it
        f0 = (G[o:e].double().norm() / t_dev[o:e].double().norm()).item()
        f257 = (G[q:r].double().norm() / t_dev[q:r].double().norm()).item()
        assert f257 < 0.8 * f0 < 0.8


# ---- 2. the bucketed path equals the one call -----------------------------------------------------------------------------
@pytest.mark.parametrize("which,regime", [("a", "both"), ("a", "none"), ("b", "off")])
def test_bucketed_prepare_equals_one_call(cuda, layouts, which, regime):
    """rn_optim_clip_prepare over block ranges, last range first, cut at tensor boundaries (plan_buckets) and once inside a
    multi-block tensor, one empty range, a local copy; then _factors with a flags buffer and _apply."""
    lay = layouts[which]
    inp = O.make_inputs(lay, regime)
    one = Arena(lay, cuda, _lib())
    G1, P = inp.g.to(cuda), inp.w.to(cuda)
    one.clip(G1, P, inp)
    bb, nb = lay.segs["bb"], lay.segs["nb"]
    big = int(nb.argmax())
    at = [40, 150, 257, 280] if which == "a" else [1, 4, 6]
    cuts = sorted({0, lay.n_blocks, int(bb[big]) + int(nb[big]) // 2} | {int(bb[i]) for i in at})
    assert nb[big] > 1 and len(cuts) >= 5
    bk = Arena(lay, cuda, _lib())
    G2 = inp.g.to(cuda)
    local = torch.full_like(G2, O.SENTINEL)
    flags = torch.full((4,), O.SENTINEL, dtype=torch.float32, device=cuda)
    for b0, b1 in reversed(list(zip(cuts[:-1], cuts[1:]))):
        bk.prepare(G2, P, inp, local, b0, b1 - b0)
        bk.prepare(G2, P, inp, local, b0, 0)           # block_count == 0: nothing happens
    bk.factors(inp, flags.data_ptr())
    before = G2.clone()
    bk.apply(G2)
    torch.cuda.synchronize()
    assert torch.equal(G2, G1) and torch.equal(bk.metrics, one.metrics)
    m = one.metrics.tolist()
    assert flags.tolist() == [max(m[4], m[5]), m[5], O.SENTINEL, O.SENTINEL]
    assert m[4:6] == ([1.0, 0.0] if regime == "both" else [0.0, 0.0])
    dev = lay.elem.to(cuda)
    assert torch.equal(local[dev], before[dev])                       # the local copy IS the stage-1 gradient
    assert (local.cpu()[lay.untouched] == O.SENTINEL).all()
    _report(f"{which}/{regime} stage 1 (bucketed)", O.verify_stage1(lay, inp, before))
    _report(f"{which}/{regime} clip (bucketed)", O.verify_clip(lay, inp, before, G2, bk.metrics, flags[:2]))


# ---- 3. the correction identity, two synthetic ranks ------------------------------------------------------------------------
def test_correction_identity_two_ranks(cuda, layouts):
    """sum of the unclipped gradients + sum of the in-place corrections == sum of the clipped gradients"""
    lay = layouts["a"]
    inps = O.two_ranks(lay)
    P = inps[0].w.to(cuda)
    ts, cors = [], []
    for r, inp in enumerate(inps):
        a = Arena(lay, cuda, _lib())
        G = inp.g.to(cuda)
        L = torch.full_like(G, O.SENTINEL)
        a.prepare(G, P, inp, L)
        a.factors(inp)
        out = torch.full_like(G, O.SENTINEL)
        src = L.clone()
        a.apply(src, out)                              # out of place
        a.apply(L, L)                                  # in place: grads == correction, as finish() calls it
        torch.cuda.synchronize()
        assert torch.equal(src, G)                     # the out-of-place call leaves its input alone
        assert torch.equal(L, out)                     # same values, and both keep the sentinel outside the tensors
        assert (L.cpu()[lay.untouched] == O.SENTINEL).all()
        _report(f"rank {r} correction", O.verify_correction(lay, inp, G, L))
        ts.append(G)
        cors.append(L)
    assert cors[0][lay.elem.to(cuda)].abs().max().item() > 0
    assert (cors[1][lay.elem.to(cuda)] == 0).all()     # nothing fired on rank 1: exactly zero everywhere
    total = (ts[0] + ts[1]) + (cors[0] + cors[1])
    _report("identity", O.verify_identity(lay, inps, ts, total))


# ---- 4. flags and metrics[4:6] -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nothing", "fired", "inf", "nan"])
def test_flags_in_the_gradient_arena(cuda, layouts, case):
    """_factors writes its flags into G[0:2], the engine's aliasing.  inf and NaN are ordinary data: inf makes its tensor's
    factor 0 (fired, not finite); NaN leaves every factor at 1 (fmaxf drops it) and is caught by the test of the global
    norm alone, so flags[0] must fire from metrics[5]."""
    lay = layouts["a"]
    inp = O.make_inputs(lay, "both" if case == "fired" else "none")
    g = inp.g.clone()
    if case == "inf":
        g[lay.rng(5)[0] + 1] = float("inf")
    if case == "nan":
        assert lay.segs["wd"][O.NAN_AT] == 0 and O.NAN_AT >= 256
        g[lay.rng(O.NAN_AT)[0] + 2] = float("nan")
    a = Arena(lay, cuda, _lib())
    G = g.to(cuda)
    a.prepare(G, inp.w.to(cuda), inp)
    a.factors(inp, G.data_ptr())
    a.apply(G)
    torch.cuda.synchronize()
    flags, m = G[:4].tolist(), a.metrics.tolist()
    print(case, flags, m[:6])
    want = {"nothing": [0.0, 0.0], "fired": [1.0, 0.0], "inf": [1.0, 1.0], "nan": [1.0, 1.0]}[case]
    assert flags == want + [O.SENTINEL] * 2
    assert m[5] == want[1] and flags[0] == max(m[4], m[5])
    if case != "nan":
        assert m[4] == want[0]
    assert (G.cpu()[lay.untouched[4:]] == O.SENTINEL).all()
    if case == "nan":                                    # every other tensor is what it was: no factor moved
        o, e = lay.rng(O.NAN_AT)
        keep = torch.ones((lay.total,), dtype=torch.bool)
        keep[o:e] = False
        keep[:4] = False
        t = _stage1(lay, cuda, O.make_inputs(lay, "none"))
        assert torch.equal(G.cpu()[keep], t[keep])


# ---- 5. SGD, two steps, both layouts, both builds ----------------------------------------------------------------------------
def _sgd_inputs(lay, cuda, h16):
    inp = O.make_inputs(lay, "none")
    v, dlt = O.sgd_state(lay)
    e = inp.w.clone()
    e[lay.elem] += dlt[lay.elem]
    pbf = torch.full((lay.total16,), O.SENTINEL16, dtype=h16)
    return inp.w.to(cuda), inp.g.to(cuda), v.to(cuda), e.to(cuda), pbf.to(cuda)


@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_sgd_two_steps(cuda, layouts, which, build):
    lay = layouts[which]
    for nesterov, m, use_ema in ((0, 0.9, True), (1, 0.9, False), (0, 0.0, False), (1, 0.0, True), (1, 0.9, True)):
        m = O.f32(m)
        a = Arena(lay, cuda, _lib(build))
        P, G, V, E, Pbf = _sgd_inputs(lay, cuda, _DT[build])
        if not use_ema:
            E = None
        for step in range(2):                      # the second step starts from a live v
            before = (P.clone(), V.clone(), None if E is None else E.clone())
            pbf0 = Pbf.clone()
            a.sgd(P, G, V, E, Pbf, m, nesterov)
            torch.cuda.synchronize()
            _report(f"{which}/{build} nesterov={nesterov} m={m:.1f} ema={use_ema} step {step}",
                    O.verify_sgd(lay, before, (P, V, E), G, LR, m, DECAY, nesterov, pbf0, Pbf))
        assert not torch.equal(P, before[0])


# ---- 5b. SGD bit for bit: both entry points against the float32 evaluation of the header's op order ----------------------------
SGD_CASES = ((0, 0.9, True), (1, 0.9, False), (0, 0.0, False), (1, 0.0, True), (1, 0.9, True))   # (nesterov, momentum, ema)


def _sgd_by(entry, a, P, G, V, E, Pbf, m, nesterov):
    """one SGD launch through `entry`: rn_optim_sgd_step, or rn_optim_step with the RN_OPT_SGD rule (unused slots NULL)"""
    import ctypes
    from retinanet import _C
    if entry == "rn_optim_sgd_step":
        return a.sgd(P, G, V, E, Pbf, m, nesterov)
    rule = _C.OptimRule(rule=_C.RN_OPT_SGD, flags=_C.RN_OPT_NESTEROV if nesterov else 0, lr=LR, momentum=m,
                        ema_decay=DECAY if E is not None else 0.0)
    _C.check(a.lib.rn_optim_step(_C.ptr(P), _C.ptr(G), _C.ptr(V), None, None, _C.ptr(E), _C.ptr(Pbf), _C.ptr(a.segs),
                                 _C.ptr(a.bs), a.lay.n_blocks, ctypes.byref(rule), None, _C.current_stream()), "rn_optim_step")


def _sgd_bits(entry, lay, cuda, build, nesterov, m, use_ema):
    """Two steps through `entry` from _sgd_inputs; after each step every arena must equal O.emu_sgd's bit for bit, the
    16-bit copy included, and every slot that is no tensor element must still hold its sentinel.  Returns the CPU arenas
    (w, v, ema or None, 16-bit copy) after each step."""
    m = O.f32(m)
    a = Arena(lay, cuda, _lib(build))
    P, G, V, E, Pbf = _sgd_inputs(lay, cuda, _DT[build])
    g0 = G.cpu()
    want = (P.cpu(), V.cpu(), E.cpu(), Pbf.cpu())
    if not use_ema:
        E = None
    steps = []
    for step in range(2):
        _sgd_by(entry, a, P, G, V, E, Pbf, m, nesterov)
        torch.cuda.synchronize()
        want = O.emu_sgd(lay, want[0], g0, want[1], want[2], want[3], LR, m, DECAY, nesterov)
        got = (P.cpu(), V.cpu(), None if E is None else E.cpu(), Pbf.cpu())
        for name, x, y in zip(("w", "v", "ema", "16-bit copy"), got, want):
            if x is not None:
                assert torch.equal(x, y), (entry, build, nesterov, m, use_ema, step, name, int((x != y).sum()))
                free = lay.untouched16 if name == "16-bit copy" else lay.untouched
                assert bool((x[free] == (O.SENTINEL16 if name == "16-bit copy" else O.SENTINEL)).all()), (entry, step, name)
        assert torch.equal(G.cpu(), g0)
        steps.append(got)
    return steps


@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_sgd_bit_for_bit_through_both_entry_points(cuda, layouts, which, build):
    """rn_optim_sgd_step and rn_optim_step with the RN_OPT_SGD rule give the bits of the float32 NumPy evaluation of the
    header's op order (optim_ref.emu_sgd), and each other's: w, v, ema and the 16-bit copy after each of two steps, on the
    engine-like layout (16-byte body, short tails, a 9-block tensor, more than 256 tensors) and on offsets 1, 2, 3 mod 4
    with the aligned-fp32 / unaligned-16-bit tensor.  Equality, no tolerance: this is what "the SGD step did not change"
    means."""
    lay = layouts[which]
    for nesterov, m, use_ema in SGD_CASES:
        one = _sgd_bits("rn_optim_sgd_step", lay, cuda, build, nesterov, m, use_ema)
        two = _sgd_bits("rn_optim_step", lay, cuda, build, nesterov, m, use_ema)
        for step, (s1, s2) in enumerate(zip(one, two)):
            for name, x, y in zip(("w", "v", "ema", "16-bit copy"), s1, s2):
                assert (x is None and y is None) or torch.equal(x, y), (nesterov, m, use_ema, step, name)
        assert not torch.equal(one[1][0], one[0][0])


# ---- 6. the skip flag in G[0] -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_sgd_skip_flag_in_G0(cuda, layouts, which, build):
    lay = layouts[which]
    a = Arena(lay, cuda, _lib(build))
    m = O.f32(0.9)
    P, G, V, E, Pbf = _sgd_inputs(lay, cuda, _DT[build])
    start = [t.clone() for t in (P, V, E, Pbf)]
    G[0] = 1.0                                                 # some rank's flag fired: the optimistic launch is a no-op
    a.sgd(P, G, V, E, Pbf, m, 1, G.data_ptr())
    torch.cuda.synchronize()
    for got, was in zip((P, V, E, Pbf), start):
        assert torch.equal(got, was)
    G[0] = 0.0
    a.sgd(P, G, V, E, Pbf, m, 1, G.data_ptr())
    free = [t.clone() for t in start]
    a.sgd(free[0], G, free[1], free[2], free[3], m, 1, None)
    torch.cuda.synchronize()
    for got, want in zip((P, V, E, Pbf), free):
        assert torch.equal(got, want)
    assert not torch.equal(P, start[0]) and not torch.equal(Pbf, start[3])
