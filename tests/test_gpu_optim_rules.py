"""rn_optim_step (SGD, Adam, RMSprop, Adagrad) against the float64 reference of optim_rules_ref.py: every mode for three
consecutive steps on the engine's offsets and on offsets it never produces, both builds, the skip flag, the refusals, and
the same rule on a TrainEngine's own arenas after real training steps, through a checkpoint, over ten Adam steps and
through the overlapped data-parallel step on one rank of an RCCL group.  The
acceptance rule is derived in optim_rules_ref.py; every test prints |got - ref| / allowance per quantity before it asserts
that none exceeds 1.  Slots that are no tensor element hold a sentinel before every launch and must keep it."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as O
import optim_rules_ref as R

pytestmark = pytest.mark.gpu

_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
_KEYS = ("w", "s0", "s1", "s2", "ema", "pbf")


def _lib(build="bf16"):
    from retinanet import _C
    return _C.lib(build == "f16")


@pytest.fixture(scope="module")
def layouts():
    ch = O.chunk()
    return {"aligned": R.rule_layout(ch, False), "skewed": R.rule_layout(ch, True)}


class Tables:
    def __init__(self, lay, dev):
        self.lay = lay
        self.segs = torch.from_numpy(lay.segs.view("uint8").copy()).to(dev)
        self.bs = torch.from_numpy(lay.block_seg.copy()).to(dev)


def _launch(lib, tab, r, st, g, ema_on=True, null_unused=False, skip_ptr=None, n_blocks=None):
    """rn_optim_step on the state dict `st` (device tensors, updated in place); returns the status"""
    from retinanet import _C
    u1, u2 = r.uses
    rule = _C.OptimRule(rule=r.rule, flags=r.flags, lr=r.lr, beta1=r.beta1, beta2=r.beta2, rho=r.rho, momentum=r.momentum,
                        epsilon=r.epsilon, ema_decay=r.ema_decay)
    s1 = None if (null_unused and not u1) else st["s1"]
    s2 = None if (null_unused and not u2) else st["s2"]
    return lib.rn_optim_step(_C.ptr(st["w"]), _C.ptr(g), _C.ptr(st["s0"]), _C.ptr(s1), _C.ptr(s2),
                             _C.ptr(st["ema"]) if ema_on else None, _C.ptr(st["pbf"]), _C.ptr(tab.segs), _C.ptr(tab.bs),
                             tab.lay.n_blocks if n_blocks is None else n_blocks, ctypes.byref(rule), skip_ptr,
                             _C.current_stream())


def _report(name, ratios):
    print(name, {k: round(v, 4) for k, v in ratios.items()})
    assert O.worst(ratios) <= 1.0, (name, ratios)


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


# ---- 1. every mode, three steps, both layouts, both builds, the moving average on and off -------------------------------------
@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("ema_on", [True, False], ids=["ema", "no-ema"])
@pytest.mark.parametrize("which", ["aligned", "skewed"])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_three_steps(cuda, layouts, mode, which, ema_on, build):
    """t = 1, 2, 3 with fresh gradients, from the slots' initial values.  With the moving average off the slots the rule
    does not use are NULL (allowed); with it on they are real arrays that must come back bit for bit."""
    from retinanet import _C
    lay = layouts[which]
    tab, lib = Tables(lay, cuda), _lib(build)
    st = {k: v.to(cuda) for k, v in R.start_state(lay, mode, _DT[build]).items()}
    for t in (1, 2, 3):
        r, g = R.mode_rule(mode, t, ema_on), R.gradients(lay, t).to(cuda)
        before, g0 = _clone(st), g.clone()
        _C.check(_launch(lib, tab, r, st, g, ema_on, null_unused=not ema_on), "rn_optim_step")
        torch.cuda.synchronize()
        assert torch.equal(g, g0)
        _report(f"{mode}/{which}/{build} ema={ema_on} t={t}", R.verify(lay, r, before, st, g, ema_on))
        assert not torch.equal(st["w"], before["w"]) and torch.isfinite(st["w"][lay.elem.to(cuda)]).all()
    if "amsgrad" in mode:
        assert not torch.equal(st["s2"], st["s1"])         # vhat kept a maximum that v has left


# ---- 2. the skip flag ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_skip_flag_leaves_every_arena_alone(cuda, layouts, mode, build):
    from retinanet import _C
    lay = layouts["aligned"]
    tab, lib = Tables(lay, cuda), _lib(build)
    st = {k: v.to(cuda) for k, v in R.start_state(lay, mode, _DT[build]).items()}
    r, g = R.mode_rule(mode, 1), R.gradients(lay, 1).to(cuda)
    start = _clone(st)
    g[0] = 1.0                                             # G[0], where the engine keeps the flag
    _C.check(_launch(lib, tab, r, st, g, skip_ptr=g.data_ptr()), "rn_optim_step")
    torch.cuda.synchronize()
    for k in _KEYS:
        assert torch.equal(st[k], start[k]), k
    g[0] = 0.0
    _C.check(_launch(lib, tab, r, st, g, skip_ptr=g.data_ptr()), "rn_optim_step")
    free = _clone(start)
    _C.check(_launch(lib, tab, r, free, g), "rn_optim_step")
    torch.cuda.synchronize()
    for k in _KEYS:
        assert torch.equal(st[k], free[k]), k
    assert not torch.equal(st["w"], start["w"]) and not torch.equal(st["pbf"], start["pbf"])


# ---- 3. refusals: RN_EINVAL, nothing launched --------------------------------------------------------------------------------
BAD = {"rule 0": (dict(rule=0), ()), "rule 5": (dict(rule=5), ()), "rule -1": (dict(rule=-1), ()),
       "adam + centered": (dict(rule=R.ADAM, flags=R.CENTERED), ()), "adam + momentum": (dict(rule=R.ADAM, flags=R.MOMENTUM), ()),
       "rmsprop + amsgrad": (dict(rule=R.RMSPROP, flags=R.AMSGRAD), ()), "adagrad + amsgrad": (dict(rule=R.ADAGRAD, flags=R.AMSGRAD), ()),
       "adagrad + centered": (dict(rule=R.ADAGRAD, flags=R.CENTERED), ()), "flag 8": (dict(rule=R.ADAM, flags=8), ()),
       "no slot0": (dict(rule=R.ADAGRAD), ("s0",)), "adam without v": (dict(rule=R.ADAM), ("s1",)),
       "amsgrad without vhat": (dict(rule=R.ADAM, flags=R.AMSGRAD), ("s2",)),
       "momentum without its slot": (dict(rule=R.RMSPROP, flags=R.MOMENTUM), ("s1",)),
       "centered without mg": (dict(rule=R.RMSPROP, flags=R.CENTERED), ("s2",)), "no blocks": (dict(rule=R.ADAM), ("blocks",)),
       "flag 16": (dict(rule=R.ADAM, flags=16), ()), "sgd + amsgrad": (dict(rule=R.SGD, flags=R.AMSGRAD), ()),
       "sgd + centered": (dict(rule=R.SGD, flags=R.CENTERED), ()), "sgd + momentum flag": (dict(rule=R.SGD, flags=R.MOMENTUM), ()),
       "rmsprop + nesterov": (dict(rule=R.RMSPROP, flags=R.NESTEROV), ()), "sgd without slot0": (dict(rule=R.SGD), ("s0",))}


@pytest.mark.parametrize("case", list(BAD))
def test_refusals_launch_nothing(cuda, layouts, case):
    from retinanet import _C
    lay = layouts["aligned"]
    tab, lib = Tables(lay, cuda), _lib()
    st = {k: v.to(cuda) for k, v in R.start_state(lay, "adam", torch.bfloat16).items()}
    start = _clone(st)
    g = R.gradients(lay, 1).to(cuda)
    fields, missing = BAD[case]
    r = R.mode_rule("adam", 1)._replace(**fields)
    call = dict(st)
    for k in missing:
        if k != "blocks":
            call[k] = None
    rule = _C.OptimRule(rule=r.rule, flags=r.flags, lr=r.lr, beta1=r.beta1, beta2=r.beta2, rho=r.rho, momentum=r.momentum,
                        epsilon=r.epsilon, ema_decay=r.ema_decay)
    status = lib.rn_optim_step(_C.ptr(call["w"]), _C.ptr(g), _C.ptr(call["s0"]), _C.ptr(call["s1"]), _C.ptr(call["s2"]),
                               _C.ptr(call["ema"]), _C.ptr(call["pbf"]), _C.ptr(tab.segs), _C.ptr(tab.bs),
                               0 if "blocks" in missing else lay.n_blocks, ctypes.byref(rule), None, _C.current_stream())
    torch.cuda.synchronize()
    assert status == _C.RN_EINVAL, case
    assert b"rn_optim_step" in lib.rn_last_error()
    for k in _KEYS:
        assert torch.equal(st[k], start[k]), (case, k)


# ---- 4. the engine -------------------------------------------------------------------------------------------------------------
ENGINE_OPTS = {"adam": dict(name="adam"), "adam+amsgrad": dict(name="adam", amsgrad=True),
               "rmsprop": dict(name="rmsprop"), "rmsprop+centered+momentum": dict(name="rmsprop", centered=True, momentum=0.9),
               "adagrad": dict(name="adagrad")}
_RATE = {"adam": 1e-3, "rmsprop": 1e-3, "adagrad": 1e-2}


@pytest.fixture(scope="module")
def engines(cuda):
    """two engines of the same model (the second restores what the first saved), built once for this module"""
    from test_gpu_train_step import _setup
    out = []
    for _ in range(2):
        p, model, eng, targets, images = _setup(cuda, 128, 2, True, seed=7, depth=26)
        init = {k: v.clone() for k, v in model.variables.items()}       # every test starts from these
        out.append((p, model, eng, targets, images.to(cuda), init))
    return out


def _configure(rig, which, rate=None):
    """model.optimizer <- the configuration `which`; the engine starts over from the model's first variables"""
    p, model, eng, init = rig[0], rig[1], rig[2], rig[5]
    from retinanet.optimizers import build_optimizer
    d = {k: v for k, v in dict(p.training.optimizer).items() if k not in ("name", "momentum", "nesterov")}
    d.update(ENGINE_OPTS[which])
    rate = _RATE[d["name"]] if rate is None else rate
    d["lr_params"] = dict(d["lr_params"], warmup_learning_rate=rate / 2, initial_learning_rate=rate, warmup_steps=4)
    model.optimizer = build_optimizer(d, p.training.train_steps, p.floatx.precision)
    _start_over(rig)
    return model.optimizer


def _start_over(rig):
    model, eng, init = rig[1], rig[2], rig[5]
    with torch.no_grad():
        for k, v in model.variables.items():
            v.copy_(init[k])
    eng.load_from_model()
    for bn, d in eng.bn_state.items():
        d["mm"].copy_(model.variables[bn + "/moving_mean"])
        d["mv"].copy_(model.variables[bn + "/moving_variance"])
    eng.step_count = 0


def _state(eng):
    return {"w": eng.P, "s0": eng.V, "s1": eng.S1, "s2": eng.S2, "ema": eng.E, "pbf": eng.Pbf}


def _snapshot(eng):
    return {k: (None if v is None else v.clone()) for k, v in _state(eng).items()}


@pytest.mark.parametrize("which", list(ENGINE_OPTS))
def test_engine_train_steps_follow_the_rule(cuda, engines, which):
    """Two train_steps: after each, the arenas satisfy the rule given the gradient the step kernel read (G after the
    clip).  A wrong t, swapped slots, a missing initial accumulator or a slot arena too many would all show."""
    p, model, eng, targets, images, _ = engines[0]
    opt = _configure(engines[0], which)
    lay = R.engine_layout(eng)
    names = [s[0] if s else None for s in opt.slots()] + [None, None]
    assert [a is not None for a in (eng.V, eng.S1, eng.S2)] == [n is not None for n in names[:3]]
    init = opt.slots()[0][1]
    assert bool((eng.V[lay.elem.to(cuda)] == init).all()) and (which != "adagrad" or init == pytest.approx(0.1))
    for step in range(2):
        before = _snapshot(eng)
        eng.train_step(images, targets)
        torch.cuda.synchronize()
        assert eng.step_count == step + 1
        r = R.engine_rule(opt, step)
        assert r.uses == (eng.S1 is not None, eng.S2 is not None)
        _report(f"engine {which} step {step}", R.verify(lay, r, before, _state(eng), eng.G, True))
        assert not torch.equal(eng.P, before["w"])


def test_engine_sgd_keeps_one_slot_arena(cuda, engines):
    """back to SGD on the same engine: V alone, zero again, and the step is the SGD rule's"""
    from retinanet.optimizers import build_optimizer
    p, model, eng, targets, images, _ = engines[0]
    _configure(engines[0], "adam+amsgrad")
    eng.train_step(images, targets)
    model.optimizer = build_optimizer(p.training.optimizer, p.training.train_steps, p.floatx.precision)
    _start_over(engines[0])
    assert eng.S1 is None and eng.S2 is None and not eng.V.any()
    lay = R.engine_layout(eng)
    before = _snapshot(eng)
    eng.train_step(images, targets)
    torch.cuda.synchronize()
    opt = model.optimizer
    lr, m, d = O.f32(opt.lr(0)), O.f32(opt.momentum), O.f32(opt.ema_decay(0))
    _report("engine sgd", O.verify_sgd(lay, (before["w"], before["s0"], before["ema"]), (eng.P, eng.V, eng.E), eng.G, lr, m, d,
                                       0, before["pbf"], eng.Pbf))


@pytest.mark.parametrize("which", ["adam+amsgrad", "rmsprop+centered+momentum", "adagrad"])
def test_resume_from_checkpoint_is_bit_exact(cuda, engines, tmp_path, which):
    """two steps, a checkpoint, two more; a second engine restores and must land on the same bits: weights, every slot,
    the moving average, the BatchNorm statistics and the next two losses"""
    from retinanet import tf_checkpoint as ck
    (p, model, eng, targets, images, _), (p2, model2, eng2, targets2, images2, _) = engines
    opt = _configure(engines[0], which)
    for _ in range(2):
        eng.train_step(images, targets)
    prefix = str(tmp_path / "weights_step_2")
    eng.save_checkpoint(prefix)
    arrays, slots = ck.load_weights(prefix)
    cls = opt.class_name
    assert int(arrays[cls + "/iter"]) == 2 and "SGD/iter" not in arrays
    k0 = eng.train_names[0]
    assert {s for (k, s) in slots if k == k0} == {s[0] for s in opt.slots() if s} | {"average"}
    want = [eng.train_step(images, targets)["weighted-loss"].item() for _ in range(2)]
    torch.cuda.synchronize()
    want_state = _snapshot(eng)
    want_mm = {bn: (d["mm"].clone(), d["mv"].clone()) for bn, d in eng.bn_state.items()}

    _configure(engines[1], which)
    with torch.no_grad():
        for v in model2.variables.values():
            v.add_(0.01)
    eng2.load_from_model()
    eng2.restore_checkpoint(prefix)
    assert eng2.step_count == 2 and model2.optimizer.iterations == 2
    got = [eng2.train_step(images2, targets2)["weighted-loss"].item() for _ in range(2)]
    torch.cuda.synchronize()
    assert got == want
    for k, v in _state(eng2).items():
        assert (v is None) == (want_state[k] is None) and (v is None or torch.equal(v, want_state[k])), k
    for bn, (mm, mv) in want_mm.items():
        assert torch.equal(eng2.bn_state[bn]["mm"], mm) and torch.equal(eng2.bn_state[bn]["mv"], mv)


def test_resume_under_another_optimizer_keeps_weights_and_starts_fresh_slots(cuda, engines, tmp_path, caplog):
    (p, model, eng, targets, images, _), (p2, model2, eng2, _, _, _) = engines
    _configure(engines[0], "rmsprop+centered+momentum")
    for _ in range(2):
        eng.train_step(images, targets)
    prefix = str(tmp_path / "weights_step_2")
    eng.save_checkpoint(prefix)
    torch.cuda.synchronize()
    opt2 = _configure(engines[1], "adagrad")
    with caplog.at_level("WARNING"):
        eng2.restore_checkpoint(prefix)
    assert "RMSprop" in caplog.text and "Adagrad" in caplog.text and "fresh" in caplog.text
    assert torch.equal(eng2.P, eng.P) and torch.equal(eng2.E, eng.E) and eng2.step_count == 2
    lay = R.engine_layout(eng2)
    assert bool((eng2.V[lay.elem.to(cuda)] == opt2.slots()[0][1]).all()) and eng2.S1 is None and eng2.S2 is None


# lr of the ten-step run: chosen on the CPU in float64 ("Adam, RMSprop, Adagrad": both loss sequences)
TEN_STEP_RATE = 1e-3


def test_ten_adam_steps_on_one_batch(cuda, engines):
    p, model, eng, targets, images, _ = engines[0]
    _configure(engines[0], "adam", rate=TEN_STEP_RATE)
    model.optimizer.learning_rate = lambda step: TEN_STEP_RATE
    losses = [eng.train_step(images, targets)["weighted-loss"].item() for _ in range(10)]
    print("ten adam steps", losses)
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


# ---- 5. the overlapped data-parallel step --------------------------------------------------------------------------------------
def _worker_dp_adam(rank, world, port, out):
    """ONE rank on a real `nccl` process group: Adam + amsgrad through the plain step, through the forced data-parallel
    machinery (buckets all-reduced during the backward pass, the optimistic launch with G[0] as its predicate) and
    through it with a clip that fires (the optimistic launch must do nothing, the second one steps once)"""
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda:0"))
    from test_gpu_data_parallel import _build
    from retinanet.optimizers import build_optimizer
    res, plain = {}, None
    # two steps where the result is compared with the plain order's bits; one step against the rule where the clip fires
    for tag, force, clip, steps in (("plain", False, 1e9, 2), ("dp", True, 1e9, 2), ("dp_clip", True, 0.5, 1)):
        model, eng, images, targets = _build(1, 0, clipnorm=clip, force_dp=force)
        p = model.params
        d = {k: v for k, v in dict(p.training.optimizer).items() if k not in ("name", "momentum", "nesterov")}
        d.update(name="adam", amsgrad=True, clipnorm=clip)
        model.optimizer = opt = build_optimizer(d, p.training.train_steps, p.floatx.precision)
        opt.learning_rate = lambda step: 1e-3
        r = {}
        for step in range(steps):
            eng._bind_optimizer()
            before = _snapshot(eng)
            eng.train_step(images, targets)
            torch.cuda.synchronize()
        if tag == "dp_clip":
            r["worst"] = O.worst(R.verify(R.engine_layout(eng), R.engine_rule(opt, 0), before, _state(eng), eng.G, True))
        r.update(overlapped=bool(eng.overlap.on), unsafe=bool(eng.overlap.unsafe), clip_fired=bool(eng.overlap.clip_fired),
                 steps=eng.step_count, slots=[a is not None for a in (eng.V, eng.S1, eng.S2)])
        if tag == "plain":
            plain = _snapshot(eng)
        elif tag == "dp":
            r["equal"] = all(torch.equal(v, plain[k]) for k, v in _state(eng).items())
        res[tag] = r
        del model, eng
        torch.cuda.empty_cache()
    out[rank] = res
    dist.destroy_process_group()


def test_overlapped_data_parallel_step_takes_the_new_kernel(cuda):
    import torch.multiprocessing as mp
    from test_gpu_data_parallel import _free_port
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_dp_adam, args=(1, _free_port(), out), nprocs=1, join=True)
    r = out[0]
    print(r)
    assert not r["plain"]["overlapped"]
    for tag, steps in (("plain", 2), ("dp", 2), ("dp_clip", 1)):
        assert r[tag]["steps"] == steps and r[tag]["slots"] == [True, True, True], (tag, r[tag])
    assert r["dp_clip"]["worst"] <= 1.0, r["dp_clip"]
    for tag in ("dp", "dp_clip"):          # (the queue probe may keep the plain order, and says so)
        assert r[tag]["overlapped"] or r[tag]["unsafe"], tag
    assert r["dp"]["equal"] and not r["dp"]["clip_fired"]
    assert r["dp_clip"]["clip_fired"] or not r["dp_clip"]["overlapped"]
