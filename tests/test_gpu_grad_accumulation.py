"""GPU: gradient accumulation (training.gradient_accumulation_steps).  The accumulate stage of csrc/rn_optim.hip against
accum_ref.py on the toy arenas of optim_ref.py in both builds — the bound, the header's op order bit for bit, the flag
slots, the slots nobody may write, the refusals — and the training engine on ResNet-50 at 128 x 128 with micro-batch 2:
bit-equality with the plain step where halving is exact, the rule with a clip that fires, the data-parallel path on one
rank, a dropped mixed_float16 step, checkpoint / resume, and the Executor with the key as the only change to its config."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import accum_ref as A
import optim_ref as O
from conftest import PKG
from test_gpu_optimizer import Arena, _lib, _report

pytestmark = pytest.mark.gpu

BUILDS = ["bf16", "f16"]
NAN = float("nan")


@pytest.fixture(scope="module")
def layouts():
    ch = O.chunk()
    return {"a": O.layout_a(ch), "b": O.layout_b(ch)}


# ---- the two entry points on an Arena ---------------------------------------------------------------------------------------
def _apply_accumulate(a, G, acc, first, metrics=None, ws=None, ws_bytes=None):
    from retinanet import _C
    ws = a.ws if ws is None else ws
    return a.lib.rn_optim_clip_apply_accumulate(
        _C.ptr(G), _C.ptr(acc), first, _C.ptr(a.metrics if metrics is None else metrics), _C.ptr(a.segs), _C.ptr(a.bs),
        a.lay.n_blocks, _C.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _C.current_stream())


def _clip_accumulate(a, G, P, acc, first, inp, ws_bytes=None):
    from retinanet import _C
    return a.lib.rn_optim_clip_accumulate(
        _C.ptr(G), _C.ptr(P), _C.ptr(acc), first, _C.ptr(a.segs), a.lay.n_segs, _C.ptr(a.bs), a.lay.n_blocks, inp.wdc,
        inp.alpha, inp.unscale, inp.clip, _C.ptr(a.metrics), _C.ptr(a.ws), a.ws.numel() if ws_bytes is None else ws_bytes,
        _C.current_stream())


def _factors_of(a, cuda):
    """the kernel's own fp32 factor of every tensor element, through the entry point: first != 0 on an arena of ones"""
    from retinanet import _C
    ones = torch.ones((a.lay.total,), dtype=torch.float32, device=cuda)
    out = torch.full((a.lay.total,), O.SENTINEL, dtype=torch.float32, device=cuda)
    _C.check(_apply_accumulate(a, ones, out, 1), "rn_optim_clip_apply_accumulate")
    return out


# ---- 1. kernel against the rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("which", ["a", "b"])
def test_accumulate_three_micro_steps(cuda, layouts, which, build):
    """nothing fires / per-tensor and global fire / nothing fires, into an accumulator that starts full of NaN: the
    accumulator against the rule and bit for bit against the header's op order, grads == t after each call, the flags, and
    the sentinel in A[2:4], the padding and the end slack"""
    from retinanet import _C
    lay, lib = layouts[which], _lib(build)
    inps = A.micro_inputs(lay)
    P = inps[0].w.to(cuda)
    acc = A.fresh_accumulator(lay).to(cuda)
    want_flags = [(0.0, 0.0), (1.0, 0.0), (1.0, 0.0)]
    for i, inp in enumerate(inps):
        alone = Arena(lay, cuda, lib)                   # t: stage 1 on its own
        t = inp.g.to(cuda)
        alone.prepare(t, P, inp)
        a = Arena(lay, cuda, lib)
        G, prev = inp.g.to(cuda), acc.clone()
        a.prepare(G, P, inp)
        a.factors(inp)
        _C.check(_apply_accumulate(a, G, acc, 1 if i == 0 else 0), "rn_optim_clip_apply_accumulate")
        factors = _factors_of(a, cuda)
        torch.cuda.synchronize()
        assert torch.equal(G, t), i                     # the stage does not write the gradient arena
        assert torch.equal(P.cpu(), inp.w)
        _report(f"{which}/{build} micro-step {i}", A.verify(lay, inp, G, prev, acc, i == 0, factors, a.metrics))
        got = acc.cpu()
        assert bool(torch.isfinite(got[lay.elem]).all()), i
        assert bool((got[lay.untouched[2:]] == O.SENTINEL).all()), i
        assert tuple(got[0:2].tolist()) == want_flags[i] and a.metrics[4:6].tolist() == [float(i == 1), 0.0], i
        if i == 0:                                      # first, every factor 1: a copy of t
            assert torch.equal(got[lay.elem], t.cpu()[lay.elem])


# ---- 2. skip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [True, False])
def test_not_finite_micro_step_drops_the_update(cuda, layouts, bad):
    """a NaN in micro-step 2 of 3: A[1] == 1 after micro-step 3, and rn_optim_step with A + 1 as its skip flag changes no
    array; the control without the NaN leaves A[1] == 0 and the same call moves the weights"""
    from retinanet import _C
    lay = layouts["a"]
    inps = A.micro_inputs(lay)
    if bad:
        g = inps[1].g.clone()
        g[lay.rng(O.NAN_AT)[0] + 2] = NAN
        inps[1] = inps[1]._replace(g=g)
    a = Arena(lay, cuda, _lib())
    P = inps[0].w.to(cuda)
    acc = A.fresh_accumulator(lay).to(cuda)
    flags = []
    for i, inp in enumerate(inps):
        _C.check(_clip_accumulate(a, inp.g.to(cuda), P, acc, 1 if i == 0 else 0, inp), "rn_optim_clip_accumulate")
        flags.append(tuple(acc[0:2].tolist()))
    assert flags == ([(0.0, 0.0), (1.0, 1.0), (1.0, 1.0)] if bad else [(0.0, 0.0), (1.0, 0.0), (1.0, 0.0)])
    v, d = O.sgd_state(lay)
    V, E = v.to(cuda), (inps[0].w + d).to(cuda)
    Pbf = torch.full((lay.total16,), O.SENTINEL16, dtype=torch.bfloat16, device=cuda)
    before = [x.clone() for x in (P, V, E, Pbf, acc)]
    a.sgd(P, acc, V, E, Pbf, O.f32(0.9), 0, skip_ptr=acc.data_ptr() + 4)
    torch.cuda.synchronize()
    same = [A.same_bits(x.float() if x.dtype == torch.bfloat16 else x, y.float() if y.dtype == torch.bfloat16 else y) == 0.0
            for x, y in zip((P, V, E, Pbf, acc), before)]
    assert same == ([True] * 5 if bad else [False, False, False, False, True])


# ---- 3. the one-call form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
def test_one_call_equals_the_three_stages(cuda, layouts, which):
    """rn_optim_clip_accumulate == prepare + factors + apply_accumulate, bit for bit: accumulator, gradient arena, metrics"""
    from retinanet import _C
    lay = layouts[which]
    inps = A.micro_inputs(lay)
    P = inps[0].w.to(cuda)
    one, three = Arena(lay, cuda, _lib()), Arena(lay, cuda, _lib())
    acc1, acc3 = A.fresh_accumulator(lay).to(cuda), A.fresh_accumulator(lay).to(cuda)
    for i, inp in enumerate(inps):
        G1, G3 = inp.g.to(cuda), inp.g.to(cuda)
        _C.check(_clip_accumulate(one, G1, P, acc1, 1 if i == 0 else 0, inp), "rn_optim_clip_accumulate")
        three.prepare(G3, P, inp)
        three.factors(inp)
        _C.check(_apply_accumulate(three, G3, acc3, 1 if i == 0 else 0), "rn_optim_clip_apply_accumulate")
        torch.cuda.synchronize()
        assert A.same_bits(acc1, acc3) == 0.0 and torch.equal(G1, G3) and torch.equal(one.metrics, three.metrics), i
    assert bool(torch.isfinite(acc1[lay.elem.to(cuda)]).all())


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_refusals(cuda, layouts, build):
    """RN_EINVAL before any launch — each pointer NULL in turn, accum == grads, a workspace one byte short — and the
    accumulator, the gradient arena and the metrics keep what they held"""
    from retinanet import _C
    lay, lib = layouts["b"], _lib(build)
    inp = A.micro_inputs(lay)[1]
    a = Arena(lay, cuda, lib)
    G, P = inp.g.to(cuda), inp.w.to(cuda)
    acc = A.fresh_accumulator(lay).to(cuda)
    a.prepare(G, P, inp)
    a.factors(inp)
    torch.cuda.synchronize()
    held = [x.clone() for x in (G, acc, a.metrics)]
    g, p, ac, m, sg, bs, ws, st = (_C.ptr(G), _C.ptr(P), _C.ptr(acc), _C.ptr(a.metrics), _C.ptr(a.segs), _C.ptr(a.bs),
                                   _C.ptr(a.ws), _C.current_stream())
    nb, ns, nbytes = lay.n_blocks, lay.n_segs, a.ws.numel()
    assert nbytes == lib.rn_optim_workspace_bytes(nb, ns)
    apply_cases = {"NULL grads": (None, ac, 0, m, sg, bs, nb, ws, nbytes), "NULL accum": (g, None, 0, m, sg, bs, nb, ws, nbytes),
                   "NULL metrics": (g, ac, 0, None, sg, bs, nb, ws, nbytes), "NULL segs": (g, ac, 0, m, None, bs, nb, ws, nbytes),
                   "NULL block_seg": (g, ac, 0, m, sg, None, nb, ws, nbytes), "NULL workspace": (g, ac, 0, m, sg, bs, nb, None, nbytes),
                   "accum == grads": (g, g, 1, m, sg, bs, nb, ws, nbytes),
                   "short workspace": (g, ac, 1, m, sg, bs, nb, ws, lib.rn_optim_workspace_bytes(nb, 1) - 1)}
    for what, args in apply_cases.items():
        assert lib.rn_optim_clip_apply_accumulate(*args, st) == _C.RN_EINVAL, what
        assert b"rn_optim_clip_apply_accumulate" in lib.rn_last_error(), what
    k = (inp.wdc, inp.alpha, inp.unscale, inp.clip)
    clip_cases = {"NULL grads": (None, p, ac, 0, sg, ns, bs, nb, *k, m, ws, nbytes), "NULL params": (g, None, ac, 0, sg, ns, bs, nb, *k, m, ws, nbytes),
                  "NULL accum": (g, p, None, 0, sg, ns, bs, nb, *k, m, ws, nbytes), "NULL segs": (g, p, ac, 0, None, ns, bs, nb, *k, m, ws, nbytes),
                  "NULL block_seg": (g, p, ac, 0, sg, ns, None, nb, *k, m, ws, nbytes), "NULL metrics": (g, p, ac, 0, sg, ns, bs, nb, *k, None, ws, nbytes),
                  "NULL workspace": (g, p, ac, 0, sg, ns, bs, nb, *k, m, None, nbytes), "accum == grads": (g, p, g, 1, sg, ns, bs, nb, *k, m, ws, nbytes),
                  "short workspace": (g, p, ac, 1, sg, ns, bs, nb, *k, m, ws, nbytes - 1)}
    for what, args in clip_cases.items():
        assert lib.rn_optim_clip_accumulate(*args, st) == _C.RN_EINVAL, what
        assert b"rn_optim_clip_accumulate" in lib.rn_last_error(), what
    torch.cuda.synchronize()
    for x, y in zip((G, acc, a.metrics), held):
        assert A.same_bits(x, y) == 0.0
    _C.check(_apply_accumulate(a, G, acc, 1), "the call the refusals are variations of")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(acc[lay.elem.to(cuda)]).all())


# ---- engines ----------------------------------------------------------------------------------------------------------------
SIZE, MICRO = 128, 2


def _engine(cuda, steps, seed=5, precision="mixed_bfloat16", clipnorm=None):
    """test_gpu_loss_normalizer.py::_engine's shape — ResNet-50 at 128 x 128, micro-batch 2, the default freeze list — with
    accumulation_steps"""
    from test_gpu_frozen_bn import _randomize
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=SIZE, precision=precision)
    p.architecture.batch_norm.use_sync = False
    if clipnorm is not None:
        p.training.optimizer.clipnorm = clipnorm
    builder = ModelBuilder(p, "train", device=cuda, seed=seed)
    model = builder()
    _randomize(model, seed, cuda)
    rx = [builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables]
    eng = TrainEngine(model, MICRO, frozen_regexes=rx, world_size=1, accumulation_steps=steps)
    model.optimizer.lr = lambda step: 0.01
    return p, model, eng


def _batches(p, cuda, seeds):
    from test_gpu_frozen_bn import _batch
    return [_batch(p, cuda, SIZE, MICRO, s) for s in seeds]


def _bits(t):
    return int(t.detach().reshape(1).cpu().view(torch.int32).item())


# ---- 5. N = 2 on the same batch twice is the plain step, bit for bit ---------------------------------------------------------
def test_two_equal_micro_steps_are_the_plain_step(cuda):
    """clipnorm = 1e9: no factor fires (asserted), so halving the loss gradient and the decay coefficient is exact through
    the backward pass, the norms and the sum t / 2 + t / 2: weights, momentum, moving average and the 16-bit copy of the
    N = 2 engine equal the N = 1 engine's bit for bit, and so do gradient-norm and weighted-loss.  (The BatchNorm moving
    statistics took two updates: they are not compared.)"""
    p, model_a, a = _engine(cuda, 1, clipnorm=1e9)
    _, model_b, b = _engine(cuda, 2, clipnorm=1e9)
    assert a.A is None and b.A is not None and torch.equal(a.P, b.P) and torch.equal(a.Pbf, b.Pbf)
    (images, targets), = _batches(p, cuda, (5,))
    w0 = a.P.clone()
    out_a = a.train_step(images, targets)
    assert float(a.metrics[4]) == 0.0 and float(a.metrics[5]) == 0.0
    micro = []
    for i in range(2):
        micro.append(b.accumulate_micro_step(images, targets, i))
        assert float(b.metrics[4]) == 0.0 and float(b.metrics[5]) == 0.0, i
        assert b.step_count == 0 and torch.equal(b.P, w0)
    b.apply_accumulated()
    from retinanet.model.train_engine import mean_loss_dict
    out_b = mean_loss_dict(micro)
    torch.cuda.synchronize()
    assert a.step_count == b.step_count == 1 and model_b.optimizer.iterations == 1
    assert not torch.equal(a.P, w0)
    for name in ("P", "V", "E", "Pbf"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b.A[0:2].tolist() == [0.0, 0.0]
    for k in ("gradient-norm", "weighted-loss", "total-loss", "l2-regularization", "num-anchors-matched"):
        assert _bits(out_a[k]) == _bits(out_b[k]), (k, out_a[k], out_b[k])


# ---- 6. N = 3, different batches, a clip that fires --------------------------------------------------------------------------
def _all_elements(lay, cuda):
    """(arena index, tensor) of EVERY tensor element, on the device (lay.elem may be a sample)"""
    sz = torch.from_numpy(lay.segs["size"].astype(np.int64)).to(cuda)
    start = torch.from_numpy(lay.segs["offset"].astype(np.int64)).to(cuda)
    seg = torch.repeat_interleave(torch.arange(len(lay.segs), device=cuda), sz)
    first = torch.cumsum(sz, 0) - sz
    return start[seg] + (torch.arange(seg.numel(), device=cuda) - first[seg]), seg


def _tensor_norms(eng, index, arena):
    """float64 norm of every tensor of an arena, summed on the device over ALL its elements"""
    elem, seg = index
    x = arena[elem].double()
    return torch.zeros((eng.n_segs,), dtype=torch.float64, device=arena.device).index_add_(0, seg, x * x).sqrt().cpu()


def _margin(norms, gn, clip):
    return min(float((norms - clip).abs().min()), abs(gn - clip)) / clip


def test_three_micro_steps_with_a_clip_that_fires(cuda):
    """A first run with the clip out of reach, on an engine of its own, gives every micro-step's tensor norms (they do not
    depend on the clip); clipnorm is then put below the largest global norm where optim_ref.margins' condition holds, and
    a fresh engine with the same seed is driven by hand: after each micro-step G is t_i and A follows accum_ref's rule
    given them; after apply_accumulated P, V, E follow optim_ref.verify_sgd given A, the loss dict is the mean of the
    three, and one optimizer step was counted."""
    import optim_rules_ref as R
    from retinanet.model.train_engine import mean_loss_dict
    p, _, first = _engine(cuda, 3, seed=7, clipnorm=1e9)
    batches = _batches(p, cuda, (7, 8, 9))
    lay = R.engine_layout(first)                        # a sample of the elements; the norms below take all of them
    index = _all_elements(lay, cuda)
    norms = []
    for i, (images, targets) in enumerate(batches):     # the first run
        first.accumulate_micro_step(images, targets, i)
        assert float(first.metrics[4]) == 0.0
        norms.append(_tensor_norms(first, index, first.G))
    del first
    p, model, eng = _engine(cuda, 3, seed=7, clipnorm=1e9)
    opt = model.optimizer
    gns = [float((n ** 2).sum().sqrt()) for n in norms]
    # candidates: below the largest global norm, so that at least that micro-step clips; the first one every norm of every
    # micro-step keeps 2e-3 c away from (twice optim_ref.margins' condition)
    cands = [max(gns) * k for k in (0.8, 0.7, 0.6, 0.5, 0.9, 0.4, 0.3)]
    clip = O.f32(next(c for c in cands if all(_margin(n, A.clip_from_norms(n, O.f32(c)).gn, O.f32(c)) > 2e-3 for n in norms)))
    opt.clipnorm = clip
    before = {k: getattr(eng, k).clone() for k in ("P", "V", "E", "Pbf")}
    micro, fired, clips = [], [], []
    for i, (images, targets) in enumerate(batches):
        prev = eng.A.clone()
        micro.append(eng.accumulate_micro_step(images, targets, i))
        torch.cuda.synchronize()
        nrm = _tensor_norms(eng, index, eng.G)
        assert torch.allclose(nrm, norms[i], rtol=1e-12, atol=0.0), i     # the same t_i as in the dry run
        c = A.clip_from_norms(nrm, clip)
        assert _margin(nrm, c.gn, clip) > 1e-3, (i, _margin(nrm, c.gn, clip))
        fired.append(c.flags[0])
        clips.append(c)
        assert float(eng.metrics[4]) == c.flags[0] and float(eng.metrics[5]) == 0.0, i
        assert O.rel(eng.metrics[1], c.gn, O.eps(lay.chunk).gn) <= 1.0 and O.rel(eng.metrics[0], c.metrics[0], O.eps(lay.chunk).m0) <= 1.0
        _report(f"engine micro-step {i}", A.verify(lay, None, eng.G, prev, eng.A, i == 0, c=c))
        assert eng.step_count == 0 and torch.equal(eng.P, before["P"])
    assert max(fired) == 1.0, (clip, gns)               # at least one micro-step clipped
    acc = eng.A.clone()
    eng.apply_accumulated()
    torch.cuda.synchronize()
    assert eng.step_count == 1 and opt.iterations == 1 and torch.equal(eng.A, acc)
    lr, m, d = O.f32(opt.lr(0)), O.f32(opt.momentum), O.f32(opt.ema_decay(0))
    _report("engine update from A", O.verify_sgd(lay, (before["P"], before["V"], before["E"]), (eng.P, eng.V, eng.E), acc, lr,
                                                 m, d, 0, before["Pbf"], eng.Pbf))
    assert not torch.equal(eng.P, before["P"])
    # the loss dict of train_step_accumulated is mean_loss_dict of the micro-steps' dicts: the mean, l2 from the last
    out = mean_loss_dict(micro)
    for k in ("weighted-loss", "class-loss", "box-loss", "total-loss", "gradient-norm", "num-anchors-matched"):
        vals = [float(mi[k]) for mi in micro]
        assert float(out[k]) == pytest.approx(sum(vals) / 3, rel=1e-6), k
    assert len({float(mi["weighted-loss"]) for mi in micro}) == 3
    assert _bits(out["l2-regularization"]) == _bits(micro[-1]["l2-regularization"])
    for mi, c in zip(micro, clips):                     # metrics[0] * R * N
        assert float(mi["gradient-norm"]) == pytest.approx(3 * c.metrics[0], rel=1e-5)
    # and train_step_accumulated is those calls: a second step through it counts one more optimizer step
    out2 = eng.train_step_accumulated(batches)
    assert eng.step_count == 2 and set(out2) == set(out) and np.isfinite(float(out2["total-loss"]))
    with pytest.raises(ValueError):
        eng.train_step_accumulated(batches[:2])
    with pytest.raises(RuntimeError):
        eng.accumulate_micro_step(*batches[1], 1)       # out of order: micro-step 0 comes first
    with pytest.raises(RuntimeError):
        eng.apply_accumulated()


# ---- 7. the data-parallel path on one rank -----------------------------------------------------------------------------------
def _worker_forced_dp(rank, world, port, out):
    """test_gpu_data_parallel.py::_worker_forced_dp with N = 2: ONE rank on an `nccl` group, the plain accumulated step and
    the data-parallel machinery forced on"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.dirname(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda:0"))
    from test_gpu_frozen_bn import _batch
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    res = {}
    for tag, force in (("plain", False), ("dp", True)):
        p = default_params(input_size=SIZE, batch_train=4)
        p.architecture.backbone.depth = 14
        p.training.optimizer.clipnorm = 1e9
        model = ModelBuilder(p, "train", device=dev, seed=21)()
        eng = TrainEngine(model, MICRO, frozen_regexes=[], world_size=1, force_dp=force, accumulation_steps=2)
        model.optimizer.lr = lambda step: 0.01
        w0 = eng.P.clone()
        batches = [_batch(p, dev, SIZE, MICRO, s) for s in (21, 22)]
        eng.accumulate_micro_step(*batches[0], 0)
        first = eng._micro_messages
        eng.accumulate_micro_step(*batches[1], 1)
        eng.apply_accumulated()
        torch.cuda.synchronize()
        res[tag] = {"P": eng.P.cpu().numpy(), "V": eng.V.cpu().numpy(), "moved": not torch.equal(eng.P, w0),
                    "sync_bn": bool(eng.sync_bn), "dp_active": bool(eng.dp_active), "messages": eng.syncbn_messages_per_step,
                    "first": first, "overlap_on": bool(eng.overlap.on), "buckets_planned": eng.overlap.buckets is not None,
                    "buckets_launched": int(eng.overlap.done), "steps": eng.step_count}
        del model, eng
        torch.cuda.empty_cache()
    out[rank] = res
    dist.destroy_process_group()


def test_forced_data_parallel_accumulation_on_one_rank(cuda):
    """force_dp=True over a one-rank group, N = 2: SyncBN messages inside every micro-step (their total is reported), the
    all-reduce of A in plain order — the overlap planned and launched no bucket — and, a sum over one rank being the
    identity, the weights of the plain N = 2 engine bit for bit"""
    import torch.multiprocessing as mp
    from test_gpu_frozen_bn import _free_port
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_forced_dp, args=(1, _free_port(), out), nprocs=1, join=True)
    plain, dp = out[0]["plain"], out[0]["dp"]
    assert not plain["dp_active"] and plain["messages"] == 0 and plain["moved"] and plain["steps"] == 1
    assert dp["dp_active"] and dp["sync_bn"] and dp["first"] > 10 and dp["messages"] == 2 * dp["first"]
    for r in (plain, dp):
        assert not r["overlap_on"] and not r["buckets_planned"] and r["buckets_launched"] == 0
    np.testing.assert_array_equal(dp["P"], plain["P"])
    np.testing.assert_array_equal(dp["V"], plain["V"])


# ---- 8. mixed_float16: one micro-step not finite drops the optimizer step -----------------------------------------------------
def test_not_finite_micro_step_drops_the_step_under_mixed_float16(cuda):
    """an inf planted in one loss-gradient buffer of micro-step 0 of 2 (micro-step 1 is clean): the update is dropped on
    the device, the scale is halved ONCE, optimizer.iterations does not advance; the clean step before it is the control"""
    p, model, eng = _engine(cuda, 2, precision="mixed_float16")
    opt = model.optimizer
    assert opt.dynamic_loss_scale and eng.f16
    batches = _batches(p, cuda, (5, 6))
    w0 = eng.P.clone()
    eng.train_step_accumulated(batches)
    eng.finish_step()
    s0 = eng.loss_scale["scale"]
    assert eng.step_count == 1 and not eng.loss_scale["skipped"] and eng.loss_scale["good"] == 1 and not torch.equal(eng.P, w0)
    before = [x.clone() for x in (eng.P, eng.V, eng.E, eng.Pbf)]
    backward = eng.backward

    def poisoned(loss_grads):
        buf = next(iter(eng.loss_grad_buffers()["class-predictions"].values()))
        buf.view(-1)[0] = float("inf")
        return backward(loss_grads)

    eng.backward = poisoned
    eng.accumulate_micro_step(*batches[0], 0)
    eng.backward = backward
    assert eng.A[0:2].tolist() == [1.0, 1.0]
    eng.accumulate_micro_step(*batches[1], 1)
    assert float(eng.metrics[5]) == 0.0 and eng.A[0:2].tolist() == [1.0, 1.0]     # the clean micro-step keeps the flag
    assert eng._micro_scale == s0
    eng.apply_accumulated()
    assert eng.step_count == 2 and eng._ls_pending        # optimistic until the flag is looked at
    for x, y in zip((eng.P, eng.V, eng.E, eng.Pbf), before):
        assert torch.equal(x, y)
    eng.finish_step()
    assert eng.loss_scale["skipped"] and eng.loss_scale["scale"] == s0 / 2 and eng.loss_scale["good"] == 0
    assert eng.step_count == 1 and opt.iterations == 1
    eng.train_step_accumulated(batches)                   # the next step runs at the halved scale and is applied
    eng.finish_step()
    assert eng._micro_scale == s0 / 2 and eng.step_count == 2 and not eng.loss_scale["skipped"]
    assert not torch.equal(eng.P, before[0]) and bool(torch.isfinite(eng.P).all())


# ---- 9. checkpoint ----------------------------------------------------------------------------------------------------------
def test_checkpoint_between_accumulated_steps_resumes_bit_exact(cuda, tmp_path):
    """save after optimizer step 1 (N = 2), restore into a fresh engine, step 2: the uninterrupted run's bits.  The file
    has no accumulator; a save inside a step is refused."""
    from retinanet import tf_checkpoint
    p, model, eng = _engine(cuda, 2, seed=7)
    b = _batches(p, cuda, (7, 8, 9, 10))
    eng.train_step_accumulated(b[:2])
    prefix = str(tmp_path / "weights_step_1")
    eng.save_checkpoint(prefix)
    arrays, slots = tf_checkpoint.load_weights(prefix)
    assert int(arrays["SGD/iter"]) == 1
    assert {s for (_, s) in slots} == {"momentum", "average"}
    eng.accumulate_micro_step(*b[2], 0)
    with pytest.raises(RuntimeError, match="inside an optimizer step"):
        eng.save_checkpoint(str(tmp_path / "never"))
    want = eng.accumulate_micro_step(*b[3], 1)
    eng.apply_accumulated()
    torch.cuda.synchronize()
    _, model2, eng2 = _engine(cuda, 2, seed=7)
    eng2.restore_checkpoint(prefix)
    assert eng2.step_count == 1 and eng2._micro_next == 0
    eng2.accumulate_micro_step(*b[2], 0)
    got = eng2.accumulate_micro_step(*b[3], 1)
    eng2.apply_accumulated()
    torch.cuda.synchronize()
    assert eng2.step_count == 2
    for k in ("weighted-loss", "gradient-norm"):
        assert _bits(got[k]) == _bits(want[k]), k
    for name in ("P", "V", "E", "Pbf", "A"):
        assert torch.equal(getattr(eng2, name), getattr(eng, name)), name


# ---- 10. the Executor: the configuration file is all a user changes ------------------------------------------------------------
def test_executor_accumulates_and_resumes(cuda, tmp_path):
    """test_gpu_executor_optim.py's pattern with `gradient_accumulation_steps: 2` as the only change: batch_size.train = 4
    becomes micro-batches of 2, three optimizer steps consume six of them, the counters count optimizer steps, and a
    second Executor resumes from `final_weights_step_3`"""
    from test_gpu_executor import _dataset, _params
    from retinanet import Executor, tf_checkpoint
    from retinanet.dataloader import InputPipeline
    from retinanet.distribute import get_strategy
    from retinanet.model import ModelBuilder
    p = _params(tmp_path, _dataset(tmp_path))
    p.experiment.run_mode = "train"
    p.training.gradient_accumulation_steps = 2
    pulled = []

    def executor(params):
        pipe = InputPipeline("train", params, False, 1, device=cuda)

        def counted(ctx):
            for images, targets in pipe(ctx):
                pulled.append(int(images.shape[0]))
                yield images, targets
        return Executor(params=params, strategy=get_strategy(params.training.strategy), run_mode="train",
                        model_builder=ModelBuilder(params, "train", device=cuda), train_input_fn=counted)

    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        ex = executor(p)
        eng = ex._engine
        assert ex.accumulation_steps == 2 and eng.accumulation_steps == 2 and eng.B == 2 and eng.A is not None
        w0 = eng.P.clone()
        ex.run()
        assert pulled == [2] * 6
        assert int(ex.optimizer.iterations) == 3 and eng.step_count == 3
        assert not torch.equal(w0, eng.P) and bool(torch.isfinite(eng.P).all())
        mdir = os.path.join(p.experiment.model_dir, p.experiment.name)
        prefix = tf_checkpoint.latest_checkpoint(mdir)
        assert prefix.endswith("final_weights_step_3")
        arrays, _ = tf_checkpoint.load_weights(prefix)
        assert int(arrays["SGD/iter"]) == 3
        p2 = copy.deepcopy(p)
        p2.training.train_steps = 4
        ex2 = executor(p2)
        assert int(ex2.optimizer.iterations) == 3 and ex2._engine.step_count == 3
        for a, b in ((ex2._engine.P, eng.P), (ex2._engine.V, eng.V), (ex2._engine.E, eng.E)):
            assert torch.equal(a, b)
        ex2.run()
        assert int(ex2.optimizer.iterations) == 4 and bool(torch.isfinite(ex2._engine.P).all())
        assert pulled == [2] * 8
    finally:
        os.chdir(cwd)
