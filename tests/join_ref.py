"""Teacher-forced float64 restatement of what every activation-gradient buffer of a TrainEngine must hold after
forward + backward.

expected(eng, key) is the sum, over the labels of eng.joins.writers[key], of that labelled backward step's contribution to
`key`.  Every contribution is the autograd gradient (float64) of a LOCAL function of one op, evaluated at the engine's own
boundary tensors: the step's upstream gradient (eng.grad[op out], the loss-gradient buffer at the prediction convs), the
forward tensors the engine stored (eng.t, eng.raw, eng.bal_out, the drop_connect factors) and the weights rounded to the
storage type.  No backward formula is written out here.  The VALUES are rounded where oracle/model_ref.py rounds them.  A
GRADIENT is rounded where the engine stores one as a 16-bit tensor and nowhere else, as in
test_bottleneck_tail_forward_backward_tight: dy at every conv output (`_r`, which rounds both directions), davg inside
BalanceFeatures, the result of an implicit-GEMM data-gradient launch (its epilogue rounds the conv output before it adds
what the buffer holds), and a gradient buffer after each of its writers — a later writer adds to the rounded sum so far,
in the writers' order.  The other rounding points (`_rf`) round the value only: rn_bn_bwd_apply / rn_bn_frozen_bwd keep the gated
gradient, the drop_connect factor and the skip gradient in fp32 registers between dz and dy.  The local function of a conv
launch is

    act(r(r(drop_connect(r(BN(r(conv(x, r(w))))))) + res))

with the value of the conv output replaced by the engine's stored raw output (eng.raw), so the BatchNorm statistics are
those of the tensor the engine normalised — the computation of test_bottleneck_tail_forward_backward_tight.

What a buffer holds is read from the planner: the plain top-down kernels carry the finer level's gradient internally, so
grad[outs[l]] holds only what its labelled writers (the out-convs) put there and grad[ins[l]] is derived from it and from
the stored grad[ins[l-1]] (restated instead where a later step, the max-pool above the backbone's top level, has added to
that buffer since); the weighted (fused) top-down kernels overwrite grad[outs[l]] with the gated gradient g_l, which
`_holds` restates; the pass-through top level is one buffer for dout and din, updated in place.

The label-to-restatement mapping is total: an unknown label raises KeyError, a label that matches another number of ops
than its count in `writers` raises too.

The comparison (`figures`, `accept`) is the one of the tight slice test: cosine > 0.9999, elements beyond 2 bf16 ulp < 2e-2,
beyond 4 ulp < 5e-3; for tensors of fewer than 1000 elements the two fractions become whole counts, never below 2.
"""
import torch
import torch.nn.functional as F

from model_ref import _r
from ulp_ref import _ulp_outliers

F64 = torch.float64
LIMITS = dict(cos=0.9999, o2=2e-2, o4=5e-3)   # test_bottleneck_tail_forward_backward_tight's numbers


# ---- the comparison ------------------------------------------------------------------------------------------------------
def figures(got, want64, mantissa_bits=7):
    """(cosine, fraction beyond 2 ulp, fraction beyond 4 ulp) of a gradient buffer against its float64 restatement;
    mantissa_bits: of the ulp (ulp_ref._ulp_outliers)"""
    a, b = got.detach().to("cpu").double().reshape(-1), want64.detach().to("cpu").double().reshape(-1)
    cos = (a @ b / (a.norm() * b.norm() + 1e-300)).item()
    return cos, _ulp_outliers(a, b, 2.0, mantissa_bits), _ulp_outliers(a, b, 4.0, mantissa_bits)


def accept(fig, n, limits=LIMITS):
    """fig = figures(...) of a tensor of n elements.  n < 1000: each fraction limit becomes a count, at least 2."""
    cos, o2, o4 = fig
    if not (cos > limits["cos"]):     # (also rejects NaN)
        return False
    if n >= 1000:
        return o2 < limits["o2"] and o4 < limits["o4"]
    return round(o2 * n) <= max(2, int(limits["o2"] * n)) and round(o4 * n) <= max(2, int(limits["o4"] * n))


# ---- rounding ------------------------------------------------------------------------------------------------------------
def _rf(x, on):
    """Round the VALUE to the storage type and let the gradient pass unrounded: a point where the forward pass holds a
    16-bit value but the backward pass materialises no gradient tensor (the BatchNorm output, drop_connect, the residual
    sum and the activation all live inside rn_bn_bwd_apply / rn_bn_frozen_bwd, which keep g in fp32 registers).  `_r`
    (oracle/model_ref.py) rounds the gradient too: used where the engine STORES one — dy at every conv output, davg of
    BalanceFeatures, and every gradient buffer after every writer (`expected`)."""
    if not on:
        return x
    dt = torch.bfloat16 if on is True else on
    return x + (x.detach().to(dt).to(x.dtype) - x.detach())


# ---- engine accessors ------------------------------------------------------------------------------------------------------
def _f(t, dt):
    return t.detach().to("cpu").to(dt)


def _val(eng, name, dt, table=None):
    """stored tensor `name` (eng.t, or `table`) without its pad channels"""
    t = (eng.t if table is None else table)[name]
    return _f(t[..., :eng.tensors[name][2]], dt)


def _var(eng, name, dt):
    return _f(eng.model.variables[name], dt)


def input_key(eng, op):
    return "bal:" + op["inp"] if op["inp"] in eng.bal_src else op["inp"]


def _input(eng, op, dt):
    """what the op's forward read: BalanceFeatures' copy of a balanced pyramid level, else the tensor itself"""
    return _val(eng, op["inp"], dt, eng.bal_out if op["inp"] in eng.bal_src else None)


def _upstream(eng, op, dt):
    """gradient at the op's output: the loss-gradient buffer at a prediction conv, else the op output's gradient buffer"""
    if op.get("out_dtype") == "f32":
        return _f(eng.dy_of[op["out"]][..., :eng.tensors[op["out"]][2]], dt)
    return _f(eng.grad[op["out"]], dt)


def _act(x, kind):
    if kind == "relu":
        return F.relu(x)
    if kind == "relu6":
        return F.relu6(x)
    if kind == "swish":
        return x * torch.sigmoid(x)
    if kind in (None, "none"):
        return x
    raise KeyError(kind)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _up(x, f):
    return x.repeat_interleave(f, 1).repeat_interleave(f, 2)


def _pool(x, f):
    return _nhwc(F.max_pool2d(_nchw(x), f))


# ---- local functions ---------------------------------------------------------------------------------------------------
def conv_output(eng, op, x):
    """conv / depthwise op on NHWC x with the weights as the engine multiplies them (+ the f32 bias): the layer's
    unrounded output"""
    h, dt = eng.h16, x.dtype
    if op["op"] == "dwconv":
        d = eng.g.dws[op["dw"]]
        k, s = d["k"], d["stride"]
        w = _r(_var(eng, d["kvar"], dt).permute(2, 3, 0, 1), h)       # [k,k,C,1] -> [C,1,k,k]
        H, W = x.shape[1], x.shape[2]
        Ho, Wo = eng.tensors[op["out"]][:2]
        pt, pl = op["pad_top"], op["pad_left"]                         # TF SAME: the odd element goes bottom / right
        pb, pr = max((Ho - 1) * s + k - H - pt, 0), max((Wo - 1) * s + k - W - pl, 0)
        return _nhwc(F.conv2d(F.pad(_nchw(x), (pl, pr, pt, pb)), w, None, stride=s, groups=d["C"]))
    c = eng.g.convs[op["conv"]]
    w = _r(_var(eng, c.get("kvar", op["conv"] + "/kernel"), dt).permute(3, 2, 0, 1), h)   # HWIO -> OIHW
    b = _var(eng, op["conv"] + "/bias", dt) if c["bias"] else None
    if op["op"] == "stem":      # first-layer conv: the image's own pads (7x7 / 2: 3 and 3; EfficientNet's 3x3 / 2: TF SAME)
        k, s, pt, pl = op.get("k", 7), c["stride"], op.get("pad_top", 3), op.get("pad_left", 3)
        Ho, Wo = eng.tensors[op["out"]][:2]
        pb, pr = max((Ho - 1) * s + k - x.shape[1] - pt, 0), max((Wo - 1) * s + k - x.shape[2] - pl, 0)
        return _nhwc(F.conv2d(F.pad(_nchw(x), (pl, pr, pt, pb)), w, b, stride=s))
    return _nhwc(F.conv2d(_nchw(x), w, b, stride=c["stride"], padding=op["pad"]))


def layer(eng, op, x, res=None, raw=None):
    """(raw conv output, layer output) of a conv / depthwise op: conv -> BatchNorm (batch statistics, or the folded moving
    ones where it is frozen under a trainable conv) -> drop_connect -> + res -> act, rounded where model_ref.py rounds.
    raw: the engine's stored conv output; its VALUE replaces the computed one, the derivative stays the conv's."""
    h, dt = eng.h16, x.dtype
    y = conv_output(eng, op, x)
    if op.get("out_dtype") == "f32":      # prediction conv: f32 layer, nothing rounded, nothing behind it
        return y, y
    if raw is not None:
        y = y + (raw - y).detach()
    y = _r(y, h)
    u = y
    if op.get("bn"):
        gamma, beta = _var(eng, op["bn"] + "/gamma", dt), _var(eng, op["bn"] + "/beta", dt)
        if eng._bn_trainable(op):
            mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
            u = (y - mean) / torch.sqrt(var + eng.eps) * gamma + beta
        else:                             # inference mode (forward.fold_bn)
            scale = gamma / torch.sqrt(_var(eng, op["bn"] + "/moving_variance", dt) + eng.eps)
            u = y * scale + (beta - _var(eng, op["bn"] + "/moving_mean", dt) * scale)
        u = _rf(u, h)
    if op["out"] in eng.dc_masks:
        u = _rf(u * _f(eng.dc_masks[op["out"]][0], dt)[:, None, None, None], h)
    if res is not None:
        u = _rf(u + res, h)
    return y, _rf(_act(u, op.get("act")), h)


def squeeze_excite(eng, op, x):
    """efficientnet.py SE.call as model_ref.py restates it: every op's output a storage tensor"""
    h, dt, name = eng.h16, x.dtype, op["se"]
    w1, b1 = _r(_var(eng, name + "/conv2d/kernel", dt)[0, 0], h), _var(eng, name + "/conv2d/bias", dt)
    w2, b2 = _r(_var(eng, name + "/conv2d_1/kernel", dt)[0, 0], h), _var(eng, name + "/conv2d_1/bias", dt)
    s = _rf(x.mean((1, 2)), h)
    s = _rf(_act(_rf(s @ w1 + b1, h), "swish"), h)
    s = _rf(s @ w2 + b2, h)
    return _rf(_rf(torch.sigmoid(s), h)[:, None, None, :] * x, h)


def maxpool(eng, op, x):
    k, s, pt, pl = op["k"], op["stride"], op["pad_top"], op["pad_left"]
    Ho, Wo = eng.tensors[op["out"]][:2]
    pb, pr = max((Ho - 1) * s + k - x.shape[1] - pt, 0), max((Wo - 1) * s + k - x.shape[2] - pl, 0)
    return _nhwc(F.max_pool2d(F.pad(_nchw(x), (pl, pr, pt, pb), value=float("-inf")), k, s))


def fusion_coef(eng, op, j, dt):
    """(a_l, a_u, s) of fusion j of a weighted top-down op (tests/fusion_ref.py: one rounding per TF op)"""
    h = eng.h16
    w_l, w_u = (_var(eng, n, dt).reshape(-1) for n in op["fusion_vars"][j])
    a_l, a_u = _r(F.relu(w_l), h), _r(F.relu(w_u), h)
    return a_l, a_u, _r(_r(a_l + a_u, h) + _r(torch.tensor(1e-4, dtype=dt), h), h)


def topdown_sum(eng, op, j, inp, upper):
    """level j < L-1 in front of its activation: in[j] + up2(out[j+1]), or the weighted sum of the fusion modes"""
    if not op.get("fusion"):
        return inp + _up(upper, 2)
    h = eng.h16
    a_l, a_u, s = fusion_coef(eng, op, j, inp.dtype)
    return _rf(_rf(_rf(inp * a_l, h) / s, h) + _rf(_rf(_up(upper, 2) * a_u, h) / s, h), h)


def topdown_level(eng, op, j, inp, upper):
    return _rf(_act(topdown_sum(eng, op, j, inp, upper), op["act"]), eng.h16)


def balance(eng, op, ins):
    """balance_features.py:19-60 as model_ref.py restates it, NHWC"""
    h, mid, n = eng.h16, op["mid"], len(ins)
    avg = None
    for i, x in enumerate(ins):
        x = _up(x, 2 ** (i - mid)) if i > mid else _pool(x, 2 ** (mid - i)) if i < mid else x
        avg = x if avg is None else avg + x
    avg = _r(avg / float(n), h)
    return [_rf(x + (_pool(avg, 2 ** (i - mid)) if i > mid else _up(avg, 2 ** (mid - i)) if i < mid else avg), h)
            for i, x in enumerate(ins)]


# ---- contributions ------------------------------------------------------------------------------------------------------
def _grad(out, wrt, upstream):
    return torch.autograd.grad(out, wrt, upstream, allow_unused=False)[0]


def _layer_grads(eng, op, dt, cache):
    """{'inp': d/d input, 'res': d/d residual} of the op's local function at the engine's upstream gradient"""
    ck = ("layer", op["out"], dt)
    if ck not in cache:
        x = _input(eng, op, dt).requires_grad_(True)
        res = _val(eng, op["residual"], dt).requires_grad_(True) if op.get("residual") else None
        raw = _val(eng, op["out"], dt, eng.raw) if op["out"] in eng.raw else None
        _, out = layer(eng, op, x, res, raw)
        gs = torch.autograd.grad(out, [x] + ([res] if res is not None else []), _upstream(eng, op, dt))
        cache[ck] = {"inp": gs[0], "res": gs[1] if res is not None else None}
    return cache[ck]


def _launch_first(eng, op):
    grp = op.get("group")
    if grp is None:
        return op["out"]
    return next(o["out"] for o in eng.ops if o["op"] == op["op"] and o.get("group") == grp)


def _topdown_carried(eng, op, j, dt):
    """what level j < L-1 sends to the gradient of out[j+1]: the derivative of its sum at the gradient the engine stored
    for that sum — the plain kernels' din[j] (grad[ins[j]]), the weighted kernels' g_j (which overwrote grad[outs[j]])"""
    upper = _val(eng, op["outs"][j + 1], dt).requires_grad_(True)
    z = topdown_sum(eng, op, j, _val(eng, op["ins"][j], dt), upper)
    key = op["ins"][j]
    if op.get("fusion"):
        gz = _f(eng.grad[op["outs"][j]], dt)
    elif eng.joins.writers[key] == ["topdown"]:
        gz = _f(eng.grad[key], dt)
    else:   # a later step (the max-pool that reads this level) has added to the buffer since: restate what the step stored
        gz = _r(_topdown(eng, op, key, dt).detach(), eng.h16)
    return _grad(z, upper, gz)


def _topdown(eng, op, key, dt):
    L, l = len(op["ins"]), op["ins"].index(key)
    if l == L - 1:          # passes through: the step adds what the level below carries, in place
        return _topdown_carried(eng, op, L - 2, dt)
    inp = _val(eng, key, dt).requires_grad_(True)
    upper = _val(eng, op["outs"][l + 1], dt)
    if op.get("fusion"):    # din[l] from the STORED gated gradient g_l
        return _grad(topdown_sum(eng, op, l, inp, upper), inp, _f(eng.grad[op["outs"][l]], dt))
    total = _f(eng.grad[op["outs"][l]], dt)
    if l > 0:
        total = total + _topdown_carried(eng, op, l - 1, dt)
    return _grad(topdown_level(eng, op, l, inp, upper), inp, total)


def _balance_grads(eng, op, dt, cache):
    ck = ("balance", tuple(op["tensors"]), dt)
    if ck not in cache:
        ins = [_val(eng, n, dt).requires_grad_(True) for n in op["tensors"]]
        outs = balance(eng, op, ins)
        gs = torch.autograd.grad(outs, ins, [_f(eng.grad["bal:" + n], dt) for n in op["tensors"]])
        cache[ck] = dict(zip(op["tensors"], gs))
    return cache[ck]


def label_parts(eng, key, label, dtype=F64, cache=None, count=None):
    """What each backward step labelled `label` adds to the gradient buffer `key`, one tensor per step; count: how often
    the label stands in writers[key] (launches over distinct inputs of one group share a label), checked against the ops
    it matches."""
    cache = {} if cache is None else cache
    kind, _, arg = label.partition(":")
    convs = [o for o in eng.ops if o["op"] in ("conv", "dwconv", "stem")]
    if kind == "dgrad":
        ops = [o for o in convs if o["op"] == "conv" and (o.get("group") or o["out"]) == arg
               and eng.requires.get(o["inp"]) and input_key(eng, o) == key]
        # the implicit-GEMM launch hands its result over as a storage tensor before anything is added to it: the epilogue
        # rounds the conv output in front of a residual (include/rnet_hip.h, rn_conv_problem: "if residual given: t = rb(t)"),
        # the 1x1 / 2 and sub-pixel forms go through a 16-bit buffer that rn_scatter_add2x / rn_depth_to_space2x add
        parts = [_r(_layer_grads(eng, o, dtype, cache)["inp"].detach(), eng.h16) for o in ops]
    elif kind == "dw_dgrad":
        outs = arg.split("+")
        ops = [o for o in convs if o["op"] == "dwconv" and o["out"] in outs and input_key(eng, o) == key]
        parts = [_layer_grads(eng, o, dtype, cache)["inp"] for o in ops]
    elif kind == "bn":
        ops = [o for o in convs if o.get("residual") == key and _launch_first(eng, o) == arg]
        parts = [_layer_grads(eng, o, dtype, cache)["res"] for o in ops]
    elif kind == "maxpool":
        ops = [o for o in eng.ops if o["op"] == "maxpool" and o["out"] == arg and o["inp"] == key]
        parts = []
        for o in ops:
            x = _val(eng, key, dtype).requires_grad_(True)
            parts.append(_grad(maxpool(eng, o, x), x, _f(eng.grad[o["out"]], dtype)))
    elif kind == "se":
        ops = [o for o in eng.ops if o["op"] == "se" and o["out"] == arg and o["inp"] == key]
        parts = []
        for o in ops:
            x = _val(eng, key, dtype).requires_grad_(True)
            parts.append(_grad(squeeze_excite(eng, o, x), x, _f(eng.grad[o["out"]], dtype)))
    elif label == "topdown":
        ops = [o for o in eng.ops if o["op"] == "topdown" and key in o["ins"]]
        parts = [_topdown(eng, o, key, dtype) for o in ops]
    elif label == "balance":
        ops = [o for o in eng.ops if o["op"] == "balance" and key in o["tensors"]]
        parts = [_balance_grads(eng, o, dtype, cache)[key] for o in ops]
    else:
        raise KeyError(f"no restatement for the backward step labelled {label!r} (writer of {key})")
    if not ops or (count is not None and len(ops) != count):
        raise KeyError(f"{label!r} stands {count} time(s) among the writers of {key} and matches {len(ops)} op(s)")
    return parts


def contribution(eng, key, label, dtype=F64, cache=None, count=None):
    """the sum of label_parts"""
    parts = label_parts(eng, key, label, dtype, cache, count)
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


def writer_parts(eng, key, dtype=F64, cache=None):
    """one contribution per entry of writers[key], in the writers' order (steps that share a label: in graph order)"""
    cache = {} if cache is None else cache
    labels = eng.joins.writers[key]
    by_label = {label: list(label_parts(eng, key, label, dtype, cache, labels.count(label))) for label in dict.fromkeys(labels)}
    return [by_label[label].pop(0) for label in labels]


def _holds(eng, key, total, dt):
    """What the buffer holds once the backward pass is over, given the sum of its writers' contributions.  One kind of
    buffer is written again by a step that is not among its writers: outs[l], l < L-1, of a WEIGHTED top-down op, which
    rn_fpn_fused_bwd_level overwrites with the gated gradient g_l = (dout + carried) act'(z_l)."""
    for op in eng.ops:
        if op["op"] == "topdown" and op.get("fusion") and key in op["outs"][:-1]:
            l = op["outs"].index(key)
            if l > 0:      # (the kernel reads dout as its writers stored it)
                total = _r(total.detach(), eng.h16) + _topdown_carried(eng, op, l - 1, dt)
            z = topdown_sum(eng, op, l, _val(eng, op["ins"][l], dt), _val(eng, op["outs"][l + 1], dt))
            z = z.detach().requires_grad_(True)
            return _grad(_rf(_act(z, op["act"]), eng.h16), z, total)
    return total


def expected(eng, key, dtype=F64, cache=None):
    """float64 tensor that eng.grad[key] must hold after forward + backward.  cache: a dict shared between the keys of one
    engine state (an op's local gradients serve its input and its residual)."""
    parts = writer_parts(eng, key, dtype, cache)
    total = parts[0]
    for p in parts[1:]:     # a later writer reads what the buffer holds: the sum so far, rounded to the storage type
        total = _r(total.detach(), eng.h16) + p
    return _holds(eng, key, total, dtype).detach()


def join_kind(eng, key):
    """the step kinds that write `key`, for the report: e.g. 'bn+dgrad+dgrad'"""
    return "+".join(sorted(label.partition(":")[0] for label in eng.joins.writers[key]))
