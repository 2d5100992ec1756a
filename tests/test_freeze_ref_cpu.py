"""CPU self-test of tests/freeze_ref.py: its closed-form gradients through frozen layers against torch.autograd on a
three-layer toy — live conv -> frozen conv + BatchNorm (inference mode) + relu -> frozen depthwise — and its teeth."""
import types

import pytest
import torch
import torch.nn.functional as F

import freeze_ref as FR

F64 = torch.float64
EPS = 1e-3


def _toy(seed=0, H=10, W=9, act="relu", factor=None):
    """x0 [2,H,W,4] -(live 3x3, bias)-> a -(frozen 3x3 / 2, BatchNorm, act)-> b -(frozen depthwise 3x3 / 2, SAME)-> c, as an
    engine stand-in with the tensors of one forward + autograd backward, and the autograd gradients {a, b, live kernel}."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=F64)
    v = {"live/kernel": rnd(3, 3, 4, 8) / 6, "live/bias": rnd(8) * 0.1, "fz/kernel": rnd(3, 3, 8, 16) / 8.5,
         "fz_bn/gamma": torch.rand(16, generator=gen, dtype=F64) + 0.5, "fz_bn/beta": rnd(16) * 0.1,
         "fz_bn/moving_mean": rnd(16) * 0.1, "fz_bn/moving_variance": torch.rand(16, generator=gen, dtype=F64) + 0.5,
         "dw/depthwise_kernel": rnd(3, 3, 16, 1) / 3}
    for t in v.values():
        t.requires_grad_(True)
    nchw, nhwc = (lambda t: t.permute(0, 3, 1, 2)), (lambda t: t.permute(0, 2, 3, 1))
    x0 = rnd(2, H, W, 4)
    a = nhwc(F.conv2d(nchw(x0), v["live/kernel"].permute(3, 2, 0, 1), v["live/bias"], padding=1))
    y = nhwc(F.conv2d(nchw(a), v["fz/kernel"].permute(3, 2, 0, 1), None, stride=2, padding=1))
    scale = v["fz_bn/gamma"] / torch.sqrt(v["fz_bn/moving_variance"] + EPS)
    u = y * scale + (v["fz_bn/beta"] - v["fz_bn/moving_mean"] * scale)
    if factor is not None:
        u = u * factor[:, None, None, None]
    b = {"relu": F.relu, "relu6": F.relu6, "none": lambda t: t, "swish": lambda t: t * torch.sigmoid(t)}[act](u)
    Hb, Wb = b.shape[1:3]
    Hc, Wc = -(-Hb // 2), -(-Wb // 2)
    th, tw = max((Hc - 1) * 2 + 3 - Hb, 0), max((Wc - 1) * 2 + 3 - Wb, 0)
    pt, pl = th // 2, tw // 2
    c = nhwc(F.conv2d(F.pad(nchw(b), (pl, tw - pl, pt, th - pt)), v["dw/depthwise_kernel"].permute(2, 3, 0, 1), None,
                      stride=2, groups=16))
    for t in (a, b):
        t.retain_grad()
    up = rnd(*c.shape)
    (c * up).sum().backward()
    g = types.SimpleNamespace(
        convs={"live": dict(k=3, cin=4, cout=8, stride=1, bias=True, kvar="live/kernel"),
               "fz": dict(k=3, cin=8, cout=16, stride=2, bias=False, kvar="fz/kernel")},
        dws={"dw": dict(k=3, C=16, stride=2, kvar="dw/depthwise_kernel")})
    ops = [dict(op="conv", out="a", inp="x0", conv="live", bn=None, act=None, residual=None, group=None, out_dtype="bf16", pad=1),
           dict(op="conv", out="b", inp="a", conv="fz", bn="fz_bn", act=act, residual=None, group=None, out_dtype="bf16", pad=1),
           dict(op="dwconv", out="c", inp="b", dw="dw", bn=None, act=None, group=None, pad_top=pt, pad_left=pl)]
    tensors = {"x0": (H, W, 4, "bf16"), "a": (H, W, 8, "bf16"), "b": (Hb, Wb, 16, "bf16"), "c": (Hc, Wc, 16, "bf16")}
    frozen = {"fz/kernel", "dw/depthwise_kernel"}
    eng = types.SimpleNamespace(
        g=g, ops=ops, tensors=tensors, h16=None, eps=EPS, bal_out={}, bal_src={}, dy_of={},
        t={"x0": x0, "a": a.detach(), "b": b.detach(), "c": c.detach()}, raw={"b": y.detach()},
        grad={"c": up, "b": b.grad, "a": a.grad}, model=types.SimpleNamespace(variables={k: t.detach() for k, t in v.items()}),
        requires={"x0": False, "a": True, "b": True, "c": True},
        dc_masks={} if factor is None else {"b": (factor, 0.8)},
        _bn_trainable=lambda op: False,
        _conv_trainable=lambda op: (g.dws[op["dw"]]["kvar"] if op["op"] == "dwconv" else g.convs[op["conv"]]["kvar"]) not in frozen,
        joins=types.SimpleNamespace(writers={"b": ["dw_dgrad:c"], "a": ["dgrad:b"]}))
    return eng, {"a": a.grad, "b": b.grad, "live/kernel": v["live/kernel"].grad}


def _close(got, want, tol=1e-11):
    return (got - want).abs().max().item() <= tol * max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("act", ["relu", "relu6", "none", "swish"])
@pytest.mark.parametrize("shape", [(10, 9), (9, 12), (8, 8)])
def test_frozen_layers_match_autograd(act, shape):
    eng, true = _toy(seed=3, H=shape[0], W=shape[1], act=act)
    conv, dw = eng.ops[1], eng.ops[2]
    assert FR.is_frozen(eng, conv) and FR.is_frozen(eng, dw) and not FR.is_frozen(eng, eng.ops[0])
    assert FR.frozen_input_keys(eng) == ["a", "b"]
    assert _close(FR.frozen_input_gradient(eng, dw), true["b"])
    assert _close(FR.frozen_input_gradient(eng, conv), true["a"])
    for key in ("a", "b"):
        assert _close(FR.expected(eng, key), true[key])
    # what reaches the live conv below the two frozen layers is its whole upstream: its weight gradient follows
    w = eng.model.variables["live/kernel"].clone().requires_grad_(True)
    out = F.conv2d(eng.t["x0"].permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), eng.model.variables["live/bias"], padding=1)
    dw_live = torch.autograd.grad(out, w, FR.expected(eng, "a").permute(0, 3, 1, 2))[0]
    assert _close(dw_live, true["live/kernel"])


def test_drop_connect_factor_and_teeth():
    factor = torch.tensor([0.0, 1.25], dtype=F64)
    eng, true = _toy(seed=4, act="none", factor=factor)
    conv = eng.ops[1]
    got = FR.frozen_input_gradient(eng, conv)
    assert _close(got, true["a"]) and bool((got[0] == 0).all()) and bool((got[1] != 0).any())
    # teeth: without the BatchNorm scale, without the gate, or with the kernel untransposed the gradient is another one
    eng, true = _toy(seed=5, act="relu")
    conv = eng.ops[1]
    dz, y = eng.grad["b"], eng.raw["b"]
    var = eng.model.variables
    scale, shift = FR.fold(var["fz_bn/gamma"], var["fz_bn/beta"], var["fz_bn/moving_mean"], var["fz_bn/moving_variance"], EPS)
    pre = FR.pre_activation(y, scale, shift)
    w = var["fz/kernel"].permute(3, 2, 0, 1)
    dx = lambda dy, w=w: FR.conv_input_gradient(dy, w, 2, 1, (10, 9))
    assert _close(dx(FR.output_gradient(dz, pre, "relu", scale)), true["a"])
    assert not _close(dx(FR.output_gradient(dz, pre, "relu", None)), true["a"], 1e-3)
    assert not _close(dx(FR.output_gradient(dz, pre, "none", scale)), true["a"], 1e-3)
    assert not _close(dx(FR.output_gradient(dz, pre, "relu", scale), w.flip(2, 3)), true["a"], 1e-3)


def test_storage_rounding_points():
    """with a storage type the value in front of the activation and dy are 16-bit tensors, the data gradient is not"""
    eng, _ = _toy(seed=6)
    eng.h16 = torch.bfloat16
    conv = eng.ops[1]
    dy = FR.frozen_output_gradient(eng, conv)
    assert torch.equal(dy, dy.to(torch.bfloat16).to(F64))
    dx = FR.frozen_input_gradient(eng, conv)
    assert not torch.equal(dx, dx.to(torch.bfloat16).to(F64))
    assert torch.equal(FR.writer_parts(eng, "a")[0], dx.to(torch.bfloat16).to(F64))       # handed over as a storage tensor
    dwp = FR.writer_parts(eng, "b")[0]
    assert torch.equal(dwp, FR.frozen_input_gradient(eng, eng.ops[2]))                     # depthwise: fp32 epilogue
