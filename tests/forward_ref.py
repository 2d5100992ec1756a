"""Teacher-forced float64 restatement of what every stored tensor of an engine must hold after a forward pass, and a
step-by-step driver over InferenceEngine.steps.  No GPU code.

expected_forward(eng, key) is the value of the ONE op (or one fused launch) that writes the tensor, computed by join_ref's
local functions (conv_output, layer, squeeze_excite, maxpool, topdown_level, balance: the rounding points of
oracle/model_ref.py) from the inputs the engine stored — so no rounding noise travels from layer to layer and the bound is
a few ulp of the storage type.  Keys: a tensor name (eng.t), `raw:<name>` (eng.raw: the conv output in front of a
BatchNorm step), `bal:<name>` (eng.bal_out: BalanceFeatures' copy in training).  expected_moving restates the moving
statistics of a live BatchNorm from the raw tensor the engine normalised.

Both engines: a TrainEngine as it is (the attributes join_ref reads); an InferenceEngine through inference_view(), where
squeeze-excite and BalanceFeatures work in place — a tensor then has two writers, and the input of the second is gone once
the pass is over.  run_stepwise() runs the launch list one step at a time with every buffer the step does not declare as
read (InferenceEngine.step_io) filled with NaN: the pre-step values of the declared reads are the teacher-forced input of
every step, the in-place ones included, and a step that reads or writes outside its declaration shows.

Bounds (none fitted to what a GPU returns):
  16-bit tensors   join_ref.figures / accept / LIMITS on the ulp of the storage type (mantissa bits 7 | 10)
  f32 predictions  test_gpu_conv._close for f32 outputs: rtol 2e-4, atol 2e-4 x the tensor's largest magnitude
  moving stats     test_bn_train_forward_backward: rtol 1e-5, atol 1e-5
"""
import types

import torch

import join_ref as J
from model_ref import _r

F64 = torch.float64
F32_RTOL = F32_ATOL = 2e-4      # test_gpu_conv._close(out_f32=True)
STAT_RTOL = STAT_ATOL = 1e-5    # test_bn_train_forward_backward


class StepFault(AssertionError):
    """run_stepwise: a step did not keep to its step_io entry"""


# ---- the engines as join_ref reads them ------------------------------------------------------------------------------------
def inference_view(eng, variables):
    """What join_ref reads, over an InferenceEngine (or a stand-in with g, t, h16, eps, step_io): every BatchNorm in
    inference form, no drop_connect, squeeze-excite and BalanceFeatures in place."""
    ops = []
    for op in eng.g.ops:
        o = dict(op)
        if o["op"] == "se":
            o["inp"] = o["out"] = o["tensor"]
        ops.append(o)
    stem = next((o for o in ops if o["op"] == "stem"), None)
    fused_pools = set(eng.step_io["conv:stem"][1]) - {stem["out"]} if stem else set()
    return types.SimpleNamespace(
        g=eng.g, ops=ops, tensors=eng.g.tensors, t=eng.t, raw={}, bal_out={}, bal_src={}, dc_masks={}, bn_state={},
        model=types.SimpleNamespace(variables=variables), h16=eng.h16, eps=eng.eps, _bn_trainable=lambda op: False,
        fused_pools=fused_pools, bneck=getattr(eng, "bneck", {}), _bneck_skip=getattr(eng, "_bneck_skip", set()))


def _unrounded(eng):
    """the same engine with no storage type: the dtype=float32 prediction layers round nothing"""
    return types.SimpleNamespace(g=eng.g, tensors=eng.tensors, model=eng.model, eps=eng.eps, h16=None)


def writers(eng):
    """{key: [writer, ...]} in launch order for every stored tensor the forward pass writes.  A writer is (kind, ...):
    layer op | raw op | bneck blk | stem_pool stem pool | se op | maxpool op | topdown op level | balance op index.
    Two writers: the tensor is gated / balanced in place (the serving engine; a frozen squeeze-excite in training)."""
    out = {}
    fused_pools = getattr(eng, "fused_pools", set())
    skip = getattr(eng, "_bneck_skip", set())
    blocks = {first: fb.blk for first, fb in getattr(eng, "bneck", {}).items()}
    stem = next((o for o in eng.ops if o["op"] == "stem"), None)
    for op in eng.ops:
        kind = op["op"]
        if kind == "stem" and fused_pools:
            pool = next(o for o in eng.ops if o["op"] == "maxpool" and o["out"] in fused_pools)
            out.setdefault(pool["out"], []).append(("stem_pool", op, pool))
        elif kind == "conv" and op["out"] in skip:
            if op["out"] in blocks:
                out.setdefault(blocks[op["out"]]["name"], []).append(("bneck", blocks[op["out"]]))
        elif kind in ("conv", "dwconv", "stem"):
            if op["out"] in eng.raw:
                out.setdefault("raw:" + op["out"], []).append(("raw", op))
            out.setdefault(op["out"], []).append(("layer", op))
        elif kind == "se":
            out.setdefault(op["out"], []).append(("se", op))
        elif kind == "maxpool":
            if op["out"] not in fused_pools:
                out.setdefault(op["out"], []).append(("maxpool", op))
        elif kind == "topdown":
            for j in range(len(op["ins"]) - 1):     # (the top level passes through: one buffer, not written)
                out.setdefault(op["outs"][j], []).append(("topdown", op, j))
        elif kind == "balance":
            for i, n in enumerate(op["tensors"]):
                out.setdefault("bal:" + n if n in eng.bal_out else n, []).append(("balance", op, i))
        else:
            raise KeyError(f"no forward restatement for op kind {kind!r}")
    assert stem is None or fused_pools or stem["out"] in out
    return out


def stored(eng, key):
    """the engine's buffer behind `key`, without its pad channels"""
    kind, _, name = key.rpartition(":") if key.startswith(("raw:", "bal:")) else ("", "", key)
    table = {"raw": eng.raw, "bal": eng.bal_out, "": eng.t}[kind]
    return table[name][..., :eng.tensors[name][2]]


def never_written(eng):
    """buffers of eng.t that no launch of the forward pass writes, from the writers: the input image apart"""
    return set(eng.t) - {"images"} - set(writers(eng)) - {o["outs"][-1] for o in eng.ops if o["op"] == "topdown"}


# ---- the restatement -----------------------------------------------------------------------------------------------------
def _read(eng, name, dt, inputs, bal=False):
    if inputs is not None and name in inputs:
        t = inputs[name]
    else:
        t = (eng.bal_out if bal else eng.t)[name]
    return J._f(t[..., :eng.tensors[name][2]], dt)


def _layer_value(eng, op, dt, x, res=None, raw=None):
    if op.get("out_dtype") == "f32":
        return J.conv_output(_unrounded(eng), op, x)
    return J.layer(eng, op, x, res, raw)[1]


def _op_input(eng, op, dt, inputs):
    if op["op"] == "stem":      # the image as rn_pack_image_nhwc4 stores it: rounded to the storage type
        return _r(_read(eng, op["inp"], dt, inputs), eng.h16)
    return _read(eng, op["inp"], dt, inputs, bal=op["inp"] in eng.bal_src)


def writer_value(eng, writer, dtype=F64, inputs=None):
    """float64 value one writer (see `writers`) stores, from the stored inputs of its op (`inputs`: {name: tensor} that
    replace the engine's buffers — the pre-step values of run_stepwise)"""
    kind, op = writer[0], writer[1]
    rd = lambda n: _read(eng, n, dtype, inputs)
    if kind == "raw":
        return _r(J.conv_output(eng, op, _op_input(eng, op, dtype, inputs)), eng.h16).detach()
    if kind == "layer":
        res = rd(op["residual"]) if op.get("residual") else None
        raw = J._val(eng, op["out"], dtype, eng.raw) if op["out"] in eng.raw else None
        return _layer_value(eng, op, dtype, _op_input(eng, op, dtype, inputs), res, raw).detach()
    if kind == "bneck":         # retinanet/model/bottleneck.py: shortcut, 1x1, 3x3, 1x1 + shortcut, every layer's output rounded
        blk, x = op, rd(op["x"])
        sc = _layer_value(eng, blk["sc"], dtype, x) if blk["sc"] else x
        y = _layer_value(eng, blk["b"], dtype, _layer_value(eng, blk["a"], dtype, x))
        return _layer_value(eng, blk["out"], dtype, y, sc).detach()
    if kind == "stem_pool":
        return J.maxpool(eng, writer[2], _layer_value(eng, op, dtype, _op_input(eng, op, dtype, inputs))).detach()
    if kind == "se":
        return J.squeeze_excite(eng, op, rd(op["inp"])).detach()
    if kind == "maxpool":
        return J.maxpool(eng, op, rd(op["inp"])).detach()
    if kind == "topdown":
        j = writer[2]
        return J.topdown_level(eng, op, j, rd(op["ins"][j]), rd(op["outs"][j + 1])).detach()
    if kind == "balance":
        return J.balance(eng, op, [rd(n) for n in op["tensors"]])[writer[2]].detach()
    raise KeyError(kind)


def expected_forward(eng, name, dtype=F64, inputs=None, writer=None):
    """float64 value the stored tensor `name` (a key of `writers`) must hold after a forward pass: that of its last
    writer, or of `writer`"""
    return writer_value(eng, writers(eng)[name][-1] if writer is None else writer, dtype, inputs)


def live_bn_ops(eng):
    return [o for o in eng.ops if o["op"] in ("conv", "dwconv", "stem") and o.get("bn") in eng.bn_state]


def expected_moving(eng, op, before, dtype=F64):
    """(moving mean, moving variance) of the live BatchNorm of `op` after one forward pass: `before` = {"mm", "mv"} blended
    with the mean and the Bessel-corrected variance of the raw tensor the engine normalised, by the engine's momentum"""
    y = J._val(eng, op["out"], dtype, eng.raw)
    n = y.numel() // y.shape[-1]
    m = float(eng.momentum_bn)
    mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False) * n / (n - 1)
    return J._f(before["mm"], dtype) * m + mean * (1 - m), J._f(before["mv"], dtype) * m + var * (1 - m)


# ---- the comparison ------------------------------------------------------------------------------------------------------
def mantissa_bits(h16):
    return 10 if h16 == torch.float16 else 7


def judge(key, got, want, h16):
    """-> (key, kind, elements, figures, accepted).  A 16-bit tensor: kind 'h16', figures = join_ref.figures on the ulp of
    the storage type, join_ref.accept; an f32 prediction map: kind 'f32', figures = (largest |error| / allowed,)."""
    got, want = got.detach().to("cpu"), want.detach().to("cpu").double()
    assert tuple(got.shape) == tuple(want.shape), (key, tuple(got.shape), tuple(want.shape))
    finite = bool(torch.isfinite(got).all())
    if got.dtype == torch.float32:
        allowed = F32_ATOL * want.abs().max() + F32_RTOL * want.abs()
        worst = ((got.double() - want).abs() / allowed).max().item()
        return key, "f32", want.numel(), (worst,), finite and worst <= 1.0
    fig = J.figures(got, want, mantissa_bits(h16))
    return key, "h16", want.numel(), fig, finite and J.accept(fig, want.numel())


def judge_stat(key, got, want):
    """moving statistic: -> (key, 'stat', elements, (largest |error| / allowed, largest |error|), accepted)"""
    got, want = got.detach().to("cpu").double(), want.detach().to("cpu").double()
    err = (got - want).abs()
    worst = (err / (STAT_ATOL + STAT_RTOL * want.abs())).max().item()
    return key, "stat", want.numel(), (worst, err.max().item()), bool(torch.isfinite(got).all()) and worst <= 1.0


def final_keys(eng):
    """the keys whose value can be rebuilt once the pass is over: one writer (an in-place second writer has overwritten
    its own input; run_stepwise judges those)"""
    return [k for k, w in writers(eng).items() if len(w) == 1]


def check_state(eng, before=None, got=None, dtype=F64):
    """Judge every stored tensor of final_keys(eng) and, with `before` (the bn_state of before the pass), every live
    BatchNorm's moving statistics.  got(key) -> the tensor to judge, default the engine's buffer.  -> rows of judge."""
    rows = []
    for key in final_keys(eng):
        rows.append(judge(key, stored(eng, key) if got is None else got(key), expected_forward(eng, key, dtype), eng.h16))
    if before is not None:
        for op in live_bn_ops(eng):
            bn = op["bn"]
            mm, mv = expected_moving(eng, op, before[bn], dtype)
            rows.append(judge_stat("mm:" + bn, eng.bn_state[bn]["mm"], mm))
            rows.append(judge_stat("mv:" + bn, eng.bn_state[bn]["mv"], mv))
    return rows


def failures(rows):
    return [(r[0], r[1], r[2], tuple(float(f"{v:.4g}") for v in r[3])) for r in rows if not r[4]]


def report_line(name, rows):
    """tensors compared, the worst cosine and outlier fractions with their tensors, the worst f32 and moving-statistic error"""
    h = [r for r in rows if r[1] == "h16"]
    parts = [f"forward steps, {name}: {sum(r[1] != 'stat' for r in rows)} tensors compared"]
    if h:
        c, o2, o4 = min(h, key=lambda r: r[3][0]), max(h, key=lambda r: r[3][1]), max(h, key=lambda r: r[3][2])
        parts.append(f"worst cosine {c[3][0]:.9f} ({c[0]}), beyond 2 ulp {o2[3][1]:.3g} ({o2[0]}), "
                     f"beyond 4 ulp {o4[3][2]:.3g} ({o4[0]})")
    f = [r for r in rows if r[1] == "f32"]
    if f:
        w = max(f, key=lambda r: r[3][0])
        parts.append(f"worst f32 error {w[3][0]:.3g} of its bound ({w[0]})")
    s = [r for r in rows if r[1] == "stat"]
    if s:
        w = max(s, key=lambda r: r[3][1])
        parts.append(f"{len(s)} moving statistics, worst error {w[3][1]:.3g} ({w[0]})")
    return "; ".join(parts)


# ---- the step driver ------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


def run_stepwise(eng, check, stream=None):
    """Run eng.steps one at a time on one stream (`stream`: what the step callables take).  For each step every eng.t
    buffer is saved, every buffer that step_io[name] does not list as read is filled with NaN (the step's own outputs
    too, unless they are inputs), the step runs, and

      * a buffer outside the declared writes that changed                               -> StepFault (undeclared write)
      * a declared write that is not also a read and did not change                     -> StepFault
      * a non-finite element in a declared write (an undeclared read, a part left out,
        an in-place step whose entry omits its own tensor)                              -> StepFault
      * check(name, reads_before, buffers_after): the caller's comparison of the written tensors with their restatement
        on the pre-step values of the declared reads ({name: tensor} both; names outside eng.t, `:stem_in`, left out).

    Then the saved buffers are restored and the declared writes kept, so the next step sees the real chain: when the
    loop ends eng.t holds what a plain pass leaves."""
    t = eng.t
    for fn, name in eng.steps:
        reads, writes = eng.step_io[name]
        saved = {k: v.clone() for k, v in t.items()}
        for k, v in t.items():
            if k not in reads:
                v.fill_(float("nan"))
        fn(stream)
        for v in t.values():
            _sync(v)
            break
        changed = {k for k, v in t.items()
                   if not (_same_bits(v, saved[k]) if k in reads else bool(torch.isnan(v).all()))}
        if changed - set(writes):
            raise StepFault(f"{name} wrote {sorted(changed - set(writes))}, which step_io does not declare")
        for k in writes:
            if k not in t:
                continue
            if k not in reads and k not in changed:
                raise StepFault(f"{name} declares the write {k} and left it as it was")
            if not bool(torch.isfinite(t[k]).all()):
                bad = int((~torch.isfinite(t[k])).sum())
                raise StepFault(f"{name}: {bad} of {t[k].numel()} elements of {k} are not finite — an undeclared read, a "
                                "part of the write left out, or an in-place step whose entry omits its own tensor")
        check(name, {k: saved[k] for k in reads if k in t}, {k: t[k] for k in writes if k in t})
        for k, v in t.items():
            if k not in writes:
                v.copy_(saved[k])


def step_checker(view, rows, covered):
    """check callback of run_stepwise over the engine behind `view` (inference_view): every written tensor against the
    restatement of THIS step's writer on the pre-step reads; judge rows go to `rows` (key `<step> -> <tensor>`), the
    (tensor, writer index) pairs judged to `covered`.  pack_stem_input and conv:stem are one unit: from the images to
    the stem output (or the pool output of the fused launch)."""
    table = writers(view)
    held = {}

    def check(name, reads, after):
        if name == "pack_stem_input":
            held.update(reads)
            return
        inputs = dict(reads, **held) if name == "conv:stem" else reads
        for k, got in after.items():
            later = name.startswith("se:") or name == "balance_features"
            ws = table.get(k, [])
            if name == "fpn_topdown" and not any(w[0] == "topdown" for w in ws):
                continue        # the top level passes through
            idx = next(i for i, w in enumerate(ws) if (w[0] in ("se", "balance")) == later)
            want = writer_value(view, ws[idx], F64, inputs)
            rows.append(judge(f"{name} -> {k}", got[..., :view.tensors[k][2]], want, view.h16))
            covered.add((k, idx))
    return check


# ---- teeth on an engine's own numbers ---------------------------------------------------------------------------------------
class _WithVariables:
    """the engine with other variables behind model.variables"""

    def __init__(self, eng, variables):
        self._eng, self.model = eng, types.SimpleNamespace(variables=variables)

    def __getattr__(self, name):
        return getattr(self._eng, name)


def wiring_teeth(eng, per_kind=3):
    """The engine's stored outputs against restatements that carry ONE wiring error each — had the engine made that error,
    its buffer would be this far from the restatement, so every one must be REJECTED: a shared launch's segment normalised
    with another level's BatchNorm, the conv bias counted twice in a folded shift (inference-form BatchNorm only: batch
    statistics cancel a bias), the residual read from another tensor of the same shape, the activation dropped.  Up to
    `per_kind` layers each.  -> [(error, key, rejected)]"""
    out, table, count = [], writers(eng), {}
    v = eng.model.variables

    def tooth(kind, what, op, wrong_op, e=eng):
        if count.get(kind, 0) >= per_kind:
            return
        count[kind] = count.get(kind, 0) + 1
        row = judge(op["out"], stored(eng, op["out"]), writer_value(e, ("layer", wrong_op)), eng.h16)
        out.append((what, op["out"], not row[4]))

    groups = set()
    for op in eng.ops:
        if op["op"] not in ("conv", "dwconv") or not op.get("bn") or [w[0] for w in table.get(op["out"], [])] != ["layer"]:
            continue
        grp = op.get("group")
        peers = [o for o in eng.ops if grp and o["op"] == op["op"] and o.get("group") == grp and o.get("bn") not in (None, op["bn"])]
        if peers and grp not in groups:
            groups.add(grp)
            tooth("bn", f"{op['out']} normalised with {peers[0]['bn']}", op, dict(op, bn=peers[0]["bn"]))
        if op["op"] == "conv" and eng.g.convs[op["conv"]]["bias"] and not eng._bn_trainable(op):
            mm = op["bn"] + "/moving_mean"
            twice = _WithVariables(eng, {**v, mm: v[mm] - v[op["conv"] + "/bias"].to(v[mm].device, v[mm].dtype)})
            tooth("bias", f"{op['out']}: conv bias twice in the folded shift", op, op, twice)
        if op.get("residual"):
            same = [n for n in eng.t if n not in (op["residual"], op["out"]) and eng.tensors[n] == eng.tensors[op["residual"]]
                    and bool(torch.isfinite(eng.t[n]).all())]
            if same:
                tooth("residual", f"{op['out']}: residual from {same[0]}", op, dict(op, residual=same[0]))
        if op.get("act") not in (None, "none"):
            tooth("act", f"{op['out']}: activation dropped", op, dict(op, act=None))
    return out
