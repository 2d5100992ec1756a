"""Adam / RMSprop / Adagrad without a GPU: the optimizer builder (names, Keras defaults, refusals), the float64 reference of
optim_rules_ref.py against torch.optim where the two formulas coincide, and the acceptance rule against a float32
emulation of the header's op order — the right one is accepted in every mode, each single fault is rejected by name.

What the cross-check with torch.optim does NOT cover: Adam with epsilon > 0 (torch adds epsilon to sqrt(v) / sqrt(1 -
beta2^t), Keras to sqrt(v): the two agree only at epsilon = 0) and RMSprop with momentum > 0 (the fused op puts epsilon
inside the root, torch outside).  Those two placements are stated from Keras 2.8 and pinned by the emulation alone."""
import copy

import numpy as np
import pytest
import torch

import optim_ref as O
import optim_rules_ref as R

F32 = np.float32
F64 = torch.float64


# ---- the builder --------------------------------------------------------------------------------------------------------
def _opt_params(**kw):
    from retinanet.cfg import default_params
    d = copy.deepcopy(dict(default_params().training.optimizer))
    d.pop("momentum"), d.pop("nesterov")
    d.update(kw)
    return d


def _build(**kw):
    from retinanet.optimizers import build_optimizer
    return build_optimizer(_opt_params(**kw), 1000, "mixed_bfloat16")


def test_builder_names_and_keras_defaults():
    a = _build(name="Adam")
    assert (a.name, a.class_name, a.beta_1, a.beta_2, a.epsilon, a.amsgrad) == ("adam", "Adam", 0.9, 0.999, 1e-7, False)
    r = _build(name="RMSPROP")
    assert (r.name, r.class_name, r.rho, r.momentum, r.epsilon, r.centered) == ("rmsprop", "RMSprop", 0.9, 0.0, 1e-7, False)
    g = _build(name="adagrad")
    assert (g.name, g.class_name, g.initial_accumulator_value, g.epsilon) == ("adagrad", "Adagrad", 0.1, 1e-7)
    for o in (a, r, g):       # what surrounds the rule is the same object as under SGD
        assert o.clipnorm == 10.0 and o.use_moving_average and o.moving_average_decay == 0.9998 and o.iterations == 0
        assert not o.dynamic_loss_scale and o.lr(0) == pytest.approx(0.008)


def test_builder_takes_the_keras_arguments():
    a = _build(name="adam", beta_1=0.8, beta_2=0.99, epsilon=1e-8, amsgrad=True)
    assert (a.beta_1, a.beta_2, a.epsilon, a.amsgrad) == (0.8, 0.99, 1e-8, True)
    r = _build(name="rmsprop", rho=0.95, momentum=0.9, epsilon=1e-6, centered=True)
    assert (r.rho, r.momentum, r.epsilon, r.centered) == (0.95, 0.9, 1e-6, True)
    g = _build(name="adagrad", initial_accumulator_value=0.5, epsilon=1e-5)
    assert (g.initial_accumulator_value, g.epsilon) == (0.5, 1e-5)


def test_builder_sgd_is_what_it_was():
    from retinanet.cfg import default_params
    from retinanet.optimizers import build_optimizer
    s = build_optimizer(default_params().training.optimizer, 1000, "mixed_float16")
    assert (s.name, s.class_name, s.momentum, s.nesterov, s.clipnorm, s.dynamic_loss_scale) == ("sgd", "SGD", 0.9, False, 10.0, True)
    assert s.slots() == [("momentum", 0.0)] and s.step_size(7) == s.lr(7)
    assert build_optimizer(dict(default_params().training.optimizer, name="SGD", nesterov=True), 1000, "x").nesterov


@pytest.mark.parametrize("name", ["adamax", "nadam", "adadelta", "ftrl", "adamw", "lamb", ""])
def test_builder_refuses_other_names(name):
    with pytest.raises(ValueError) as e:
        _build(name=name)
    for known in ("sgd", "adam", "rmsprop", "adagrad"):
        assert known in str(e.value)


@pytest.mark.parametrize("name,key", [("adam", "nesterov"), ("adam", "momentum"), ("adam", "rho"), ("rmsprop", "beta_1"),
                                      ("rmsprop", "nesterov"), ("adagrad", "momentum"), ("adagrad", "amsgrad")])
def test_builder_refuses_a_key_the_class_does_not_take(name, key):
    with pytest.raises(TypeError) as e:
        _build(name=name, **{key: 0.5})
    assert repr(key) in str(e.value)


def test_builder_slots_and_checkpoint_names():
    from retinanet.optimizers.builder import iter_key, read_iterations
    assert _build(name="adam").slots() == [("m", 0.0), ("v", 0.0), None]
    assert _build(name="adam", amsgrad=True).slots() == [("m", 0.0), ("v", 0.0), ("vhat", 0.0)]
    assert _build(name="rmsprop").slots() == [("rms", 0.0), None, None]
    assert _build(name="rmsprop", momentum=0.5, centered=True).slots() == [("rms", 0.0), ("momentum", 0.0), ("mg", 0.0)]
    assert _build(name="adagrad").slots() == [("accumulator", 0.1)]
    a = _build(name="adam")
    assert iter_key(a) == "Adam/iter" and iter_key(_build(name="rmsprop")) == "RMSprop/iter"
    assert iter_key(_build(name="adagrad")) == "Adagrad/iter" and iter_key(None) == "SGD/iter"
    assert read_iterations({"Adam/iter": np.int64(5), "SGD/iter": np.int64(9)}, a) == (5, "Adam")
    assert read_iterations({"SGD/iter": np.int64(9)}, a) == (9, "SGD")          # written under another optimizer
    assert read_iterations({}, a) == (0, None)


def test_adam_step_size_is_alpha_of_iterations_plus_one():
    a = _build(name="adam")
    lr = a.lr(0)
    assert a.step_size(0) == pytest.approx(lr * (1 - 0.999) ** 0.5 / (1 - 0.9), rel=1e-14)
    a.iterations = 2
    assert a.step_size() == pytest.approx(a.lr(2) * (1 - 0.999 ** 3) ** 0.5 / (1 - 0.9 ** 3), rel=1e-14)
    assert a.step_size(2) == pytest.approx(R.adam_alpha(a.lr(2), 0.9, 0.999, 3), rel=1e-14)
    assert _build(name="rmsprop").step_size(2) == a.lr(2) and _build(name="adagrad").step_size(2) == a.lr(2)


# ---- the float64 reference against torch.optim ------------------------------------------------------------------------------
def _cross(make_torch, rule_at, uses, s0_init=0.0, steps=3):
    gen = torch.Generator().manual_seed(77)
    n = 4096
    w = torch.randn((n,), generator=gen, dtype=F64) * 0.05
    p = torch.nn.Parameter(w.clone())
    opt = make_torch([p])
    s = [torch.full((n,), s0_init, dtype=F64), torch.zeros((n,), dtype=F64), torch.zeros((n,), dtype=F64)]
    for t in range(1, steps + 1):
        g = torch.pow(10.0, torch.rand((n,), generator=gen, dtype=F64) * 6 - 4) * torch.sign(torch.randn((n,), generator=gen, dtype=F64))
        p.grad = g.clone()
        opt.step()
        out = R.step(rule_at(t), w, g, s[0], s[1] if uses[0] else None, s[2] if uses[1] else None, f32_consts=False)
        w = out["w"].v
        for i, k in enumerate(("s0", "s1", "s2")):
            if k in out:
                s[i] = out[k].v
        torch.testing.assert_close(w, p.detach(), rtol=1e-12, atol=1e-15)
    return s, opt.state[p]


def test_reference_against_torch_adagrad():
    lr, eps = 0.05, 1e-7
    s, st = _cross(lambda ps: torch.optim.Adagrad(ps, lr=lr, initial_accumulator_value=0.1, eps=eps),
                   lambda t: R.Rule(R.ADAGRAD, 0, lr, epsilon=eps), (False, False), s0_init=0.1)
    torch.testing.assert_close(s[0], st["sum"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("centered", [False, True])
def test_reference_against_torch_rmsprop_without_momentum(centered):
    lr, eps, rho = 0.01, 1e-7, 0.9
    s, st = _cross(lambda ps: torch.optim.RMSprop(ps, lr=lr, alpha=rho, eps=eps, momentum=0, centered=centered),
                   lambda t: R.Rule(R.RMSPROP, R.CENTERED if centered else 0, lr, rho=rho, epsilon=eps), (False, centered))
    torch.testing.assert_close(s[0], st["square_avg"], rtol=1e-13, atol=0)
    if centered:
        torch.testing.assert_close(s[2], st["grad_avg"], rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("amsgrad", [False, True])
def test_reference_and_step_size_against_torch_adam_at_epsilon_zero(amsgrad):
    """alpha_t comes from the product's OptimizerConfig.step_size: a `t` for `t + 1` there fails here"""
    a = _build(name="adam", epsilon=0.0, amsgrad=amsgrad)
    a.learning_rate = lambda step: 0.002
    s, st = _cross(lambda ps: torch.optim.Adam(ps, lr=0.002, betas=(0.9, 0.999), eps=0.0, amsgrad=amsgrad),
                   lambda t: R.Rule(R.ADAM, R.AMSGRAD if amsgrad else 0, a.step_size(t - 1), 0.9, 0.999, epsilon=0.0),
                   (True, amsgrad))
    torch.testing.assert_close(s[0], st["exp_avg"], rtol=1e-13, atol=1e-300)
    torch.testing.assert_close(s[1], st["exp_avg_sq"], rtol=1e-13, atol=0)
    if amsgrad:
        torch.testing.assert_close(s[2], st["max_exp_avg_sq"], rtol=1e-13, atol=0)


def test_allowance_arithmetic_known_answers():
    one = lambda x: torch.tensor([x], dtype=F64)
    x, y = R.Val(one(3.0)), R.Val(one(4.0))
    s = x * y
    assert s.v.item() == 12.0 and s.a.item() == R.U * 12.0 + R.TINY
    q = s / R.Val(one(2.0))
    assert q.v.item() == 6.0 and q.a.item() == pytest.approx(s.a.item() / 2 * (1 + R.U) + R.U * 6.0 + R.TINY, rel=1e-12)
    r = R.Val(one(4.0), one(1e-6)).sqrt()
    assert r.v.item() == 2.0 and 2.5e-7 < r.a.item() - R.U * 2.0 < 2.5e-7 * (1 + 1e-6)
    z = R.Val(one(0.0)).sqrt()
    assert z.v.item() == 0.0 and z.a.item() == R.TINY
    m = R.Val(one(1.0), one(0.5)).maximum(R.Val(one(2.0), one(0.25)))
    assert (m.v.item(), m.a.item()) == (2.0, 0.5)
    bad = R.Val(one(1.0)) / R.Val(one(1e-3), one(2e-3))          # the divisor's allowance reaches zero
    assert bad.a.isnan().all() and O.ratio(torch.tensor([1000.5]), bad.ref()) == float("inf")


# ---- float32 emulation of the kernel, right and with single faults ----------------------------------------------------------
def emu(lay, r, st, g, ema_on=True, fault=None):
    """rn_optim_step in NumPy float32, the header's op order; returns the new state dict"""
    new = {k: v.clone() for k, v in st.items()}
    arr = {k: new[k].numpy() for k in ("w", "s0", "s1", "s2", "ema")}
    old = {k: st[k].numpy() for k in arr}
    gn = g.numpy()
    c1 = F32(1.0) - F32(r.beta1 if r.rule == R.ADAM else r.rho)
    c2, omd = F32(1.0) - F32(r.beta2), F32(1.0) - F32(r.ema_decay)
    lr, eps, mom_c = F32(r.lr), F32(r.epsilon), F32(r.momentum)
    for s in lay.segs:
        o, n = int(s["offset"]), int(s["size"])
        sl = slice(o, o + n)
        w, gg, s0, s1, s2 = old["w"][sl], gn[sl], old["s0"][sl], old["s1"][sl], old["s2"][sl]
        if r.rule == R.ADAM:
            m = s0 + (gg - s0) * c1
            v = s1 + (gg * gg - s1) * c2
            d = v
            if r.flags & R.AMSGRAD:
                d = np.maximum(s2, v)
                if fault != "vhat_not_stored":
                    arr["s2"][sl] = d
            arr["s0"][sl], arr["s1"][sl] = m, v
            den = np.sqrt(d + eps) if fault == "adam_eps_inside" else np.sqrt(d) + eps
            nw = w - (lr * m) / den
        elif r.rule == R.RMSPROP:
            ms = s0 + (gg * gg - s0) * c1
            arr["s0"][sl] = ms
            d = ms
            if r.flags & R.CENTERED:
                mg = s2 + (gg - s2) * c1
                arr["s2"][sl] = mg
                d = ms - mg * mg
            if r.flags & R.MOMENTUM:
                den = np.sqrt(d) + eps if fault == "rms_momentum_eps_outside" else np.sqrt(d + eps)
                mom = mom_c * s1 + (lr * gg) / den
                arr["s1"][sl] = mom
                nw = w - mom
            else:
                nw = w - (lr * gg) / (np.sqrt(d) + eps)
        elif r.rule == R.SGD:
            vel = mom_c * s0 - lr * gg
            arr["s0"][sl] = vel
            nw = w + (mom_c * vel - lr * gg) if r.flags & R.NESTEROV else w + vel
        else:
            acc = s0 + gg * gg
            arr["s0"][sl] = acc
            nw = w - (lr * gg) / (np.sqrt(s0 if fault == "adagrad_old_accumulator" else acc) + eps)
        nw = nw.astype(F32)
        arr["w"][sl] = nw
        if ema_on:
            e = old["ema"][sl]
            arr["ema"][sl] = e - omd * (e - (w if fault == "ema_from_old_weight" else nw))
        if s["bf"] >= 0:
            x = torch.from_numpy(nw.copy())
            if fault == "copy_truncates":
                x = (x.view(torch.int32) & -65536).view(torch.float32)
            new["pbf"][int(s["bf"]):int(s["bf"]) + n] = x.to(new["pbf"].dtype)
    return new


@pytest.fixture(scope="module")
def lays():
    ch = O.chunk()
    return {"aligned": R.rule_layout(ch, False), "skewed": R.rule_layout(ch, True)}


def test_layouts_and_gradients_cover_what_the_issue_names(lays):
    ch = O.chunk()
    for lay in lays.values():
        assert lay.segs["size"].tolist() == [1, 3, 4, 5, 255, 1025, ch - 1, ch, ch + 1, 2 * ch + 7]
        assert set(lay.segs["wd"].tolist()) == {0, 1} and (lay.segs["bf"] < 0).sum() == 2
        assert lay.untouched.numel() > 8 and lay.untouched16.numel() > 8
    a, b = lays["aligned"].segs, lays["skewed"].segs
    assert (a["offset"] % 4 == 0).all() and (a["bf"][a["bf"] >= 0] % 8 == 0).all()
    assert {int(x) % 4 for x in b["offset"]} == {0, 1, 2, 3}
    g = R.gradients(lays["aligned"], 1)[lays["aligned"].elem].double()
    nz = g[g != 0].abs()
    assert (g == 0).sum() > 100 and nz.min().item() == pytest.approx(1e-6, rel=1e-6) and nz.max().item() == 100.0
    assert nz.min() >= 0.99e-6 and (nz < 1e-5).sum() > 100 and (nz > 10).sum() > 100
    assert not torch.equal(R.gradients(lays["aligned"], 1), R.gradients(lays["aligned"], 2))


@pytest.mark.parametrize("ema_on", [True, False])
@pytest.mark.parametrize("which", ["aligned", "skewed"])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_rule_accepts_the_float32_emulation(lays, mode, which, ema_on):
    lay = lays[which]
    st = R.start_state(lay, mode, torch.bfloat16)
    for t in (1, 2, 3):
        r, g = R.mode_rule(mode, t, ema_on), R.gradients(lay, t)
        if r.flags & R.CENTERED:
            margin = R.centered_margin(lay, r, st, g)
            print(mode, t, "centered margin", margin)
            assert margin > 1e-3
        new = emu(lay, r, st, g, ema_on)
        ratios = R.verify(lay, r, st, new, g, ema_on)
        print(mode, which, t, {k: round(v, 4) for k, v in ratios.items()})
        assert O.worst(ratios) <= 1.0, (mode, t, ratios)
        assert not torch.equal(new["w"], st["w"]) and torch.isfinite(new["w"][lay.elem]).all()
        st = new


# fault -> (mode that shows it, the check that must reject it)
FAULTS = {"adam_t_for_t_plus_1": ("adam", "w"), "adam_eps_inside": ("adam", "w"),
          "rms_momentum_eps_outside": ("rmsprop+momentum", "s1"), "adagrad_old_accumulator": ("adagrad", "w"),
          "vhat_not_stored": ("adam+amsgrad", "s2"), "ema_from_old_weight": ("adam", "ema"),
          "copy_truncates": ("rmsprop", "16-bit copy")}


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_rule_rejects_fault(lays, fault, t):
    mode, where = FAULTS[fault]
    lay = lays["aligned"]
    st = R.start_state(lay, mode, torch.bfloat16)
    for k in range(1, t):                                   # a live state in front of step 2
        st = emu(lay, R.mode_rule(mode, k), st, R.gradients(lay, k))
    r, g = R.mode_rule(mode, t), R.gradients(lay, t)
    run = r
    if fault == "adam_t_for_t_plus_1":     # alpha of `iterations` = t - 1; at the first step that is 0 / 0
        run = r._replace(lr=O.f32(R.adam_alpha(R.LR, R.BETA1, R.BETA2, t - 1)) if t > 1 else float("nan"))
    ratios = R.verify(lay, r, st, emu(lay, run, st, g, fault=fault), g)
    assert ratios[where] > 1.0, (fault, ratios)
    for k, v in ratios.items():            # what is no tensor element is a copy whatever the arithmetic did
        assert v == 0.0 or not k.endswith(("untouched", "unused")), (fault, k)


def test_rule_rejects_a_write_into_padding_and_into_an_unused_slot(lays):
    lay = lays["aligned"]
    st = R.start_state(lay, "adagrad", torch.bfloat16)
    r, g = R.mode_rule("adagrad", 1), R.gradients(lay, 1)
    new = emu(lay, r, st, g)
    assert O.worst(R.verify(lay, r, st, new, g)) <= 1.0
    o, e = lay.rng(1)
    assert e - o == 3
    bad = {k: v.clone() for k, v in new.items()}
    bad["s0"][e] = 0.0                                       # the padding float behind a 3-element tensor
    assert R.verify(lay, r, st, bad, g)["s0 untouched"] > 1.0
    bad = {k: v.clone() for k, v in new.items()}
    bad["s1"][lay.elem[5]] = 1.0                             # adagrad has no second slot
    assert R.verify(lay, r, st, bad, g)["s1 unused"] > 1.0
