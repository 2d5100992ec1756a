"""Float64 restatement of the gradient a FROZEN conv / depthwise layer hands down (training.freeze_variables: `backbone`,
`fpn`, `head` above trainable layers), written out in closed form — no autograd in this file's arithmetic.

A frozen layer has no weight, bias, gamma or beta gradient; what is left of its backward pass is

    dy = r(scale * (factor_n * (dz * act'(pre))))      the gradient at the conv output (rn_bn_frozen_bwd; rn_act_bwd or dz
                                                       itself where the layer has no BatchNorm)
    dx = conv_transpose(dy, r(w))                      the data gradient (the forward kernel on dy with flipped weights)

with scale = gamma / sqrt(moving_variance + eps), pre = r(r(r(y scale + shift) factor_n) + residual) the value in front of
the activation, rebuilt from the conv output y the forward pass stored, and r() the rounding to the storage type where the
engine holds a 16-bit tensor (tests/join_ref.py states the same points for the live layers).

`expected(eng, key)` is join_ref.expected with the contributions of frozen layers replaced by these formulas: the other
writers of a buffer (live layers, top-down, BalanceFeatures) keep join_ref's autograd restatement, the sum over the writers
and the rounding between them are join_ref's.  tests/test_freeze_ref_cpu.py checks the formulas against torch.autograd."""
import torch
import torch.nn.functional as F

import join_ref as J

F64 = torch.float64


def storage(x, dt):
    """x rounded to the storage type dt (None: not at all)"""
    return x if dt is None else x.to(dt).to(x.dtype)


def fold(gamma, beta, mean, var, eps):
    """(scale, shift) of a BatchNorm in inference mode"""
    scale = gamma / torch.sqrt(var + eps)
    return scale, beta - mean * scale


def act_derivative(pre, act):
    if act in (None, "none"):
        return torch.ones_like(pre)
    if act == "relu":
        return (pre > 0).to(pre.dtype)
    if act == "relu6":
        return ((pre > 0) & (pre < 6)).to(pre.dtype)
    if act == "swish":
        s = torch.sigmoid(pre)
        return s * (1 + pre * (1 - s))
    raise KeyError(act)


def pre_activation(y, scale=None, shift=None, factor=None, residual=None, dt=None):
    """NHWC value in front of the activation from the stored conv output y: BatchNorm (inference mode), the per-image
    drop_connect factor, the residual add, each a storage tensor"""
    u = y
    if scale is not None:
        u = storage(y * scale + shift, dt)
    if factor is not None:
        u = storage(u * factor[:, None, None, None], dt)
    if residual is not None:
        u = storage(u + residual, dt)
    return u


def output_gradient(dz, pre, act, scale=None, factor=None, dt=None):
    """dy at the conv output of a frozen layer from dz at the layer output"""
    g = dz * act_derivative(pre, act)
    if factor is not None:
        g = g * factor[:, None, None, None]
    if scale is not None:
        g = g * scale
    return storage(g, dt)


def conv_input_gradient(dy, w_oihw, stride, pad, in_hw):
    """NHWC gradient at the input ([N, H, W, Cin], in_hw = (H, W)) of a conv with kernel w [Cout][Cin][k][k]"""
    k = w_oihw.shape[2]
    g = dy.permute(0, 3, 1, 2)
    opad = [in_hw[i] - ((g.shape[2 + i] - 1) * stride - 2 * pad + k) for i in (0, 1)]
    dx = F.conv_transpose2d(g, w_oihw, None, stride=stride, padding=pad, output_padding=opad)
    return dx.permute(0, 2, 3, 1)


def depthwise_input_gradient(dy, w_c1kk, stride, pad_top, pad_left, in_hw):
    """the same for a depthwise conv with kernel [C][1][k][k] and TensorFlow SAME pads (the odd element bottom / right)"""
    H, W = in_hw
    g = dy.permute(0, 3, 1, 2)
    full = F.conv_transpose2d(g, w_c1kk, None, stride=stride, groups=w_c1kk.shape[0])     # the padded input's gradient
    full = F.pad(full, (0, max(pad_left + W - full.shape[3], 0), 0, max(pad_top + H - full.shape[2], 0)))
    return full[:, :, pad_top:pad_top + H, pad_left:pad_left + W].permute(0, 2, 3, 1)


# ---- on an engine ------------------------------------------------------------------------------------------------------------
def is_frozen(eng, op):
    return op["op"] in ("conv", "dwconv") and not eng._conv_trainable(op)


def frozen_output_gradient(eng, op, dt=F64):
    """dy at the conv output of frozen op `op` from the engine's boundary tensors"""
    h = eng.h16
    dz = J._upstream(eng, op, dt)
    if op.get("out_dtype") == "f32":          # prediction conv: the loss gradient is its dy
        return dz
    scale = shift = factor = residual = None
    if op.get("bn"):
        var = lambda n: J._var(eng, op["bn"] + n, dt)
        scale, shift = fold(var("/gamma"), var("/beta"), var("/moving_mean"), var("/moving_variance"), eng.eps)
        y = J._val(eng, op["out"], dt, eng.raw)
        if op["out"] in eng.dc_masks:
            factor = J._f(eng.dc_masks[op["out"]][0], dt)
        if op.get("residual"):
            residual = J._val(eng, op["residual"], dt)
        pre = pre_activation(y, scale, shift, factor, residual, h)
    else:                                     # no BatchNorm: rn_act_bwd gates on the stored output (relu / relu6 / none)
        if op.get("act") == "swish":
            raise KeyError("swish without a BatchNorm has no backward")
        pre = J._val(eng, op["out"], dt)
    return output_gradient(dz, pre, op.get("act"), scale, factor, h)


def frozen_input_gradient(eng, op, dt=F64):
    """what the data-gradient launch of frozen op `op` computes for its input, unrounded"""
    h = eng.h16
    dy = frozen_output_gradient(eng, op, dt)
    H, W = eng.tensors[op["inp"]][:2]
    if op["op"] == "dwconv":
        d = eng.g.dws[op["dw"]]
        w = storage(J._var(eng, d["kvar"], dt).permute(2, 3, 0, 1), h)        # [k,k,C,1] -> [C,1,k,k]
        return depthwise_input_gradient(dy, w, d["stride"], op["pad_top"], op["pad_left"], (H, W))
    c = eng.g.convs[op["conv"]]
    w = storage(J._var(eng, c.get("kvar", op["conv"] + "/kernel"), dt).permute(3, 2, 0, 1), h)   # HWIO -> OIHW
    return conv_input_gradient(dy, w, c["stride"], op["pad"], (H, W))


def label_ops(eng, key, label):
    """the conv / depthwise ops whose data-gradient step labelled `label` writes buffer `key` (the matching of
    join_ref.label_parts, tests/join_ref.py:304-314), [] for the other kinds of label"""
    kind, _, arg = label.partition(":")
    convs = [o for o in eng.ops if o["op"] in ("conv", "dwconv")]
    if kind == "dgrad":
        return [o for o in convs if o["op"] == "conv" and (o.get("group") or o["out"]) == arg
                and eng.requires.get(o["inp"]) and J.input_key(eng, o) == key]
    if kind == "dw_dgrad":
        outs = arg.split("+")
        return [o for o in convs if o["op"] == "dwconv" and o["out"] in outs and J.input_key(eng, o) == key]
    return []


def writer_parts(eng, key, dt=F64, cache=None):
    """join_ref.writer_parts with the frozen layers' contributions in closed form.  An implicit-GEMM data gradient is
    handed over as a storage tensor (join_ref.py:307-310), a depthwise one in fp32."""
    cache = {} if cache is None else cache
    labels = eng.joins.writers[key]
    by_label = {}
    for label in dict.fromkeys(labels):
        ops = label_ops(eng, key, label)
        if ops and all(is_frozen(eng, o) for o in ops):
            if len(ops) != labels.count(label):
                raise KeyError(f"{label!r} stands {labels.count(label)} time(s) among the writers of {key} and matches {len(ops)}")
            parts = [frozen_input_gradient(eng, o, dt) for o in ops]
            if label.startswith("dgrad:"):
                parts = [storage(p, eng.h16) for p in parts]
        else:
            parts = list(J.label_parts(eng, key, label, dt, cache, labels.count(label)))
        by_label[label] = parts
    return [by_label[label].pop(0) for label in labels]


def expected(eng, key, dt=F64, cache=None):
    """float64 tensor eng.grad[key] must hold after forward + backward (join_ref.expected's sum over the writers)"""
    parts = writer_parts(eng, key, dt, cache)
    total = parts[0]
    for p in parts[1:]:
        total = storage(total.detach(), eng.h16) + p
    return J._holds(eng, key, total, dt).detach()


def frozen_input_keys(eng):
    """the gradient buffers at the input of every frozen conv / depthwise op that has one, in graph order"""
    keys = []
    for op in eng.ops:
        if is_frozen(eng, op) and eng.requires.get(op["inp"]):
            k = J.input_key(eng, op)
            if k not in keys:
                keys.append(k)
    return keys
