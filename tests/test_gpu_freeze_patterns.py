"""GPU: training.freeze_variables with the `backbone`, `fpn` and `head` keys (and their combinations with the others) on
ResNet and on EfficientNet-B0 with its separable FPN and heads — frozen layers below, between and above trainable ones
(DESIGN.md section 7f).  Shapes, weights and batches are those of test_gpu_frozen_bn.py: 128 x 128, B = 2, use_sync off."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import freeze_ref as FR
import join_ref as J
from join_counts import check_joins
from test_gpu_frozen_bn import _batch, _randomize, _ulp_outliers

pytestmark = pytest.mark.gpu

SIZE, B = 128, 2
MODELS = ["resnet14", "resnet26", "efficientnet-b0"]
KEY_LISTS = [["backbone"], ["fpn"], ["head"], ["fpn", "head"], ["backbone", "fpn"], ["backbone", "fpn", "head"], ["head", "bn"]]
UNCHECKED_CAP = 2      # test_gpu_gradient_joins.py:34 — and, as there, none is used


def _params(model, keys):
    from retinanet.cfg import default_params, efficientnet_params
    if model.startswith("efficientnet"):
        p = efficientnet_params(model, input_size=SIZE)      # separable FPN and heads, relu, mixed_float16
        assert p.architecture.activation.type == "relu" and p.floatx.precision == "mixed_float16"
    else:
        p = default_params(input_size=SIZE)
        p.architecture.backbone.depth = int(model[len("resnet"):])
    p.training.freeze_variables = list(keys)
    p.architecture.batch_norm.use_sync = False
    return p


def _build(cuda, model, keys, seed=5, regexes=None, weight_decay=True, **engine_kw):
    """-> SimpleNamespace(p, builder, model, eng, images, targets, frozen): `frozen` is the set the patterns name, computed
    here from the variable names alone"""
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = _params(model, keys)
    p.training.use_weight_decay = weight_decay
    builder = ModelBuilder(p, "train", device=cuda, seed=seed)
    net = builder()
    _randomize(net, seed, cuda)
    rx = [builder.FREEZE_VARS_REGEX[k] for k in keys] if regexes is None else regexes
    eng = TrainEngine(net, B, frozen_regexes=rx, **{"world_size": 1, **engine_kw})
    net.optimizer.lr = lambda step: 0.01
    images, targets = _batch(p, cuda, SIZE, B, seed)
    frozen = {k for k in net.variables if any(r.search(k) for r in rx)}
    return SimpleNamespace(p=p, builder=builder, model=net, eng=eng, images=images, targets=targets, frozen=frozen)


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _ENGINES.clear()
    torch.cuda.empty_cache()


def _shared(cuda, model, keys):
    """one engine per (model, key list) for the tests that only read its plan or step it once"""
    key = (model, tuple(keys))
    if key not in _ENGINES:
        _ENGINES[key] = _build(cuda, model, keys)
    return _ENGINES[key]


def _kernel_names(eng):
    return [k for k in eng.train_names if eng.var_kind.get(k, ("other",))[0] != "other"]


def _frozen_layer_ops(eng):
    return [o for o in eng.ops if o["op"] in ("conv", "dwconv", "stem") and not eng._conv_trainable(o)]


def _pack_buffers(eng):
    return [t[5] for t in eng.frozen_dgrad_packs] + [t[3] for t in eng.frozen_dw_flip_packs]


# ---- 1: builds and steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", KEY_LISTS, ids=["+".join(k) for k in KEY_LISTS])
@pytest.mark.parametrize("model", MODELS)
def test_builds_and_steps(cuda, model, keys):
    """Before this feature the EfficientNet cases and every case with a frozen layer above a trainable one raised
    NotImplementedError.  One train_step with weight decay on: nothing frozen moves, everything else does."""
    s = _shared(cuda, model, keys)
    eng, net, frozen = s.eng, s.model, s.frozen
    specs = net.graph.var_specs
    assert eng.frozen == frozen
    assert eng.train_names == [k for k in net.variables if specs[k].get("trainable", True) and k not in frozen]
    assert set(eng.p_off) == set(eng.train_names)          # no slice of the parameter / gradient / slot / EMA arenas
    before = {k: v.clone() for k, v in net.variables.items()}
    live_stats = {bn: (d["mm"].clone(), d["mv"].clone()) for bn, d in eng.bn_state.items()}
    assert all(bn + "/gamma" not in frozen for bn in live_stats)
    frozen_bn = [b for b in net.graph.bns if b + "/gamma" in frozen]
    assert set(frozen_bn) | set(live_stats) == set(net.graph.bns) and not set(frozen_bn) & set(live_stats)
    packs = [t.clone() for t in _pack_buffers(eng)]
    out = eng.train_step(s.images, s.targets)
    torch.cuda.synchronize()
    eng.finish_step()
    assert np.isfinite(float(out["weighted-loss"].item())) and np.isfinite(float(out["gradient-norm"].item()))
    assert bool(torch.isfinite(eng.P).all())
    eng.store_to_model()
    moved = [k for k in frozen if not torch.equal(net.variables[k], before[k])]
    assert not moved, moved[:8]
    still = [k for k in _kernel_names(eng) if torch.equal(net.variables[k], before[k])]
    assert not still, still[:8]
    same = [bn for bn, (mm, mv) in live_stats.items() if torch.equal(eng.bn_state[bn]["mm"], mm)
            or torch.equal(eng.bn_state[bn]["mv"], mv)]
    assert not same, same[:8]
    # the data-gradient weight packs of frozen layers are constants
    assert all(torch.equal(a, b) for a, b in zip(packs, _pack_buffers(eng)))
    assert eng.syncbn_messages_per_step == 0


# ---- 2: nothing is computed for a frozen variable ------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", KEY_LISTS, ids=["+".join(k) for k in KEY_LISTS])
@pytest.mark.parametrize("model", MODELS)
def test_nothing_is_planned_for_a_frozen_variable(cuda, model, keys):
    s = _shared(cuda, model, keys)
    eng, frozen = s.eng, s.frozen
    # the planner's step records: no step completes a frozen gradient, every side-stream step (weight / bias gradients)
    # completes trainable ones, no weight-gradient launch belongs to a frozen layer
    for step in eng.bwd_steps:
        assert not set(step.writes) & frozen, sorted(set(step.writes) & frozen)[:4]
        assert not step.side or (step.writes and set(step.writes) <= set(eng.train_names))
    wgrad_layers = {n[len("wgrad:"):] for n, _ in eng.wgrad_launches}
    assert all(eng.g.convs[c].get("kvar", c + "/kernel") not in frozen for c in wgrad_layers)
    assert all(eng.g.dws[n[len("dw_wgrad:"):]]["kvar"] not in frozen for n, _ in eng.dw_wgrad_launches)
    assert {k for st in eng.bwd_steps for k in st.writes} == set(eng.train_names)
    # a frozen layer whose launch hands no gradient down keeps nothing for a backward pass
    inference, through, dropped = [], [], []
    for op in _frozen_layer_ops(eng):
        if eng._passes_gradient(op):
            through.append(op)
        elif op.get("survival") is not None:
            dropped.append(op)       # drop_connect between BatchNorm and residual add: raw output + rn_bn_apply, forward only
        else:
            inference.append(op)
    for op in inference:
        assert op["out"] not in eng.raw and op["out"] not in eng.grad and op["out"] not in eng.bn_groups, op["out"]
    for op in dropped:
        grp = eng.bn_groups[op["out"]]
        assert op["out"] in eng.raw and op["out"] not in eng.grad and grp.frozen and grp.dys == [None]
        assert not grp.problem.seg[0].dy and not grp.problem.seg[0].act_mask and grp.problem.seg[0].sample_scale
    for op in (o for o in eng.ops if o["op"] == "se" and not eng._se_trainable(o)):
        assert op["out"] == op["inp"] == op["tensor"] and op["out"] not in eng.se_state
        assert op["tensor"] + ":se" not in eng.t and op["out"] not in eng.grad
    assert set(eng.se_state) == {o["out"] for o in eng.ops if o["op"] == "se" and eng._se_trainable(o)}
    for op in through:
        assert op["out"] in eng.grad and (not op.get("bn") or op["out"] in eng.raw)
    # the three forms occur where the key lists put them
    above = bool(set(keys) & {"fpn", "head"}) and not {"backbone", "fpn"} <= set(keys)
    assert bool(through) == above, (len(through), keys)
    if "backbone" in keys:
        assert inference and bool(dropped) == model.startswith("efficientnet")
    # frozen data-gradient packs are constants: packed on load, never in the per-step repack list
    lo, hi = eng.P.data_ptr(), eng.P.data_ptr() + 4 * eng.P.numel()
    per_step = [t[5] for t in eng.dgrad_packs] + [t[3] for t in eng.dw_flip_packs]
    assert all(lo <= t[0] < hi for t in eng.dgrad_packs + eng.dw_flip_packs)
    assert not {t.data_ptr() for t in per_step} & {t.data_ptr() for t in _pack_buffers(eng)}
    assert bool(_pack_buffers(eng)) == bool(through)
    assert all(t[0] in frozen for t in eng.frozen_dgrad_packs + eng.frozen_dw_flip_packs)
    if model.startswith("efficientnet") and through:
        assert eng.frozen_dw_flip_packs and eng.frozen_dgrad_packs
    if not model.startswith("efficientnet") and "backbone" in keys:
        # stage-1 fused bottleneck eligibility is unchanged: every block the library accepts at this shape is taken
        from retinanet.model.bottleneck import fused_blocks
        assert len(eng.bneck) == len(fused_blocks(eng.lib, eng.g, B, lambda blk: True))


# ---- 3: l2-regularization ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,keys", [("resnet14", ["fpn"]), ("resnet14", ["backbone", "fpn", "head"]),
                                        ("efficientnet-b0", ["backbone"]), ("efficientnet-b0", ["head"])],
                         ids=["resnet14-fpn", "resnet14-all", "efficientnet-b0-backbone", "efficientnet-b0-head"])
def test_l2_regularization_counts_trainable_kernels_only(cuda, model, keys):
    """alpha / 2 * sum ||w||^2 over the trainable decayed kernels (executor.py:296-327), in float64 from the engine's own
    weights as the step reads them.  Tolerance: rel 1e-5, the one of the existing assertions on this term
    (test_gpu_train_kernels.py:959, test_gpu_fusion.py:622; test_gpu_train_step.py itself asserts none)."""
    s = _build(cuda, model, keys)
    eng = s.eng
    alpha = float(s.p.training.weight_decay_alpha)
    kernels = _kernel_names(eng)
    assert kernels and not set(kernels) & s.frozen
    want = sum(alpha * 0.5 * float((eng._pview(k).double() ** 2).sum()) for k in kernels)
    everything = want + sum(alpha * 0.5 * float((s.model.variables[k].double() ** 2).sum()) for k in s.frozen
                            if k.endswith("kernel"))
    out = eng.train_step(s.images, s.targets)
    torch.cuda.synchronize()
    got = float(out["l2-regularization"].item())
    print(f"l2-regularization {model} {keys}: {got:.8f}, float64 over trainable kernels {want:.8f}, with the frozen ones {everything:.8f}")
    assert got == pytest.approx(want, rel=1e-5)
    assert abs(everything - want) > 100 * 1e-5 * want, "the frozen kernels' share is too small for this check to see"
    assert float(out["total-loss"].item()) == pytest.approx(float(out["weighted-loss"].item()) + got, rel=1e-6)


# ---- 4: gradients through frozen layers, tight -----------------------------------------------------------------------------------
def _forward_backward(cuda, eng, images, seed=99):
    """test_gpu_gradient_joins.run_engine's pass: fixed drop_connect factors, random loss gradients, every gradient buffer
    poisoned with 1024 in front of the backward pass.  A mixed_float16 engine gets its loss gradients times 2048, as a real
    step hands them over times the loss scale (LossScaleOptimizer): a frozen separable layer with the reference's
    initialisation and an inference-mode BatchNorm shrinks a gradient ~20-fold where a live BatchNorm divides by the batch
    deviation, so four of them take N(0, 1) loss gradients to ~5e-7 — float16 subnormals with two or three bits."""
    scale = 2048.0 if eng.f16 else 1.0
    for j, (out, (m, sp)) in enumerate(sorted(eng.dc_masks.items(), key=lambda kv: int(kv[0][1:].split("_")[0]))):
        m.copy_(torch.tensor([0.0 if (j % 4 == b) else 1.0 / sp for b in range(B)]))
    with torch.cuda.device(cuda):
        preds = eng.forward(images.to(cuda), draw=False)
        g = torch.Generator().manual_seed(seed)
        up = {k: {lv: (torch.randn(preds[k][lv].shape, generator=g) * scale).to(cuda) for lv in preds[k]} for k in preds}
        for buf in eng.grad.values():
            buf.fill_(1024.0)
        eng.backward(up)
        torch.cuda.synchronize()


def _rerun_in_range(cuda, eng, key):
    """Run the depthwise data-gradient launches that write eng.grad[key] again (the engine's own rn_dw_problem records,
    eng.dw_launches, in planning order: the first stores, the later ones accumulate) after multiplying the gradient at each
    writer's output by 2^k in place — exact in float16 — with k such that the buffer's rms lands near 1/4.  The buffer is
    poisoned first.  Returns k."""
    import ctypes
    from retinanet import _C
    labels = eng.joins.writers[key]
    launches = [(n, p, ups) for n, kind, p, ups in eng.dw_launches if kind == "dgrad" and n in labels]
    assert [n for n, _, _ in launches] == labels, (key, labels)
    ops = [o for label in dict.fromkeys(labels) for o in FR.label_ops(eng, key, label)]
    assert len(ops) == len(labels) and len({o["out"] for o in ops}) == len(ops)
    k = int(torch.floor(torch.log2(0.25 / eng.grad[key].double().pow(2).mean().sqrt())).item())
    for o in ops:
        u = eng.grad[o["out"]]
        assert float(u.float().abs().max()) * 2.0 ** k < 2.0 ** 15, (key, o["out"], k)
        before = u.double()
        u.mul_(2.0 ** k)
        assert torch.equal(u.double(), before * 2.0 ** k)
    eng.grad[key].fill_(1024.0)
    st = _C.current_stream()
    with torch.cuda.device(cuda):
        for n, p, ups in launches:
            for a in ups:
                _C.check(eng.lib.rn_upsample_zero2x(*a, st), "rn_upsample_zero2x")
            _C.check(eng.lib.rn_depthwise_conv2d_nhwc_fwd(ctypes.byref(p), st), n)
        torch.cuda.synchronize()
    return k


@pytest.mark.parametrize("model,keys", [("resnet26", ["fpn"]), ("resnet26", ["head"]), ("efficientnet-b0", ["head"])],
                         ids=["resnet26-fpn", "resnet26-head", "efficientnet-b0-head"])
def test_gradients_through_frozen_layers_match_float64(cuda, model, keys):
    """The gradient buffer at the input of EVERY frozen conv / depthwise op that has one, against freeze_ref.expected: the
    frozen layers' contributions in closed form in float64 from the engine's boundary tensors, the sum over the writers
    of a join as tests/join_ref.py takes it.  Bounds: join_ref.LIMITS through join_ref.accept, unchanged (cosine > 0.9999,
    beyond 2 ulp < 2e-2, beyond 4 ulp < 5e-3); no key is left out.

    float16 engines, keys out of the storage type's range: the metric judges an element at no less than 2^-8 of the
    tensor's rms, where two bfloat16 ulps are rms * 2^-15; a float16 tensor resolves 2^-25 (half a subnormal quantum), so
    a buffer with rms < 2^-10 cannot be held to these bounds by ANY float16 tensor.  At 128 x 128 pyramid level 7 is one
    pixel, each frozen depthwise layer above it passes only its centre tap (|w| ~ 0.026 at the reference's
    initialisation), and from the top of a tower to fpn_out7 the gradient shrinks 3.5e8-fold — more than float16 holds
    between overflow and that resolution, whatever the loss-gradient scale (measured with N(0, 2048^2) loss gradients:
    fpn_out7 rms 1.39e-5, all subnormals, 20.3 % beyond 2 ulp; the other 74 buffers pass).  Such a key is therefore checked
    a second time with its inputs in range (_rerun_in_range): the gradients at its writers' outputs — the engine's own,
    from the pass above — times a power of two, which is exact, and the engine's planned data-gradient launches run again
    on them.  Same launches, same reference, same bounds; the first pass's figures are printed.  Only keys written by
    depthwise data gradients alone are re-run (their launches are self-contained records of the engine); any other key
    stands on its first pass."""
    s = _build(cuda, model, keys)
    eng = s.eng
    check_joins(eng)
    _forward_backward(cuda, eng, s.images)
    keys_ = FR.frozen_input_keys(eng)
    frozen_ops = [o for o in eng.ops if FR.is_frozen(eng, o) and eng.requires.get(o["inp"])]
    groups = {o.get("group") for o in frozen_ops}
    if keys == ["head"]:      # the shared five-level tower groups, both heads in one launch
        assert {"tower0", "tower1", "tower2", "tower3"} <= groups
        assert sum(o.get("group") == "tower0" for o in frozen_ops) == 10
        first = "tower0:dw" if model.startswith("efficientnet") else "tower0"     # both heads read one pyramid level: a join
        assert all(len(eng.joins.writers[J.input_key(eng, o)]) == 2 for o in frozen_ops if o.get("group") == first)
    if model.startswith("efficientnet"):      # separable pairs: depthwise + pointwise of one frozen SeparableConv2D
        assert any(o["op"] == "dwconv" for o in frozen_ops) and {"tower1:dw", "tower1"} <= groups
        assert "box-head_t1_p3:dw" in keys_ and "box-head_t0_p3" in keys_
    if keys == ["fpn"]:
        assert {"fpn_1x1", "fpn_out"} <= groups and "fpn_td3" in keys_ and "g2b1_out" in keys_
    rows, cache, wants_rms = [], {}, {}
    for key in keys_:
        want = FR.expected(eng, key, cache=cache)
        wants_rms[key] = float(want.pow(2).mean().sqrt())
        got = eng.grad[key]
        assert tuple(got.shape) == tuple(want.shape), (key, got.shape, want.shape)
        fig = J.figures(got, want)
        rows.append((key, J.join_kind(eng, key), want.numel(), fig, J.accept(fig, want.numel())))
    worst = lambda i, pick: pick(rows, key=lambda r: r[3][i])
    c, o2, o4 = worst(0, min), worst(1, max), worst(2, max)
    rms = {k: float(eng.grad[k].double().pow(2).mean().sqrt()) for k in keys_}
    print(f"frozen data gradients, {model} {keys}: rms of the buffers {min(rms.values()):.3g} ({min(rms, key=rms.get)}) .. {max(rms.values()):.3g}")
    print(f"frozen data gradients, {model} {keys}: {len(rows)} keys; worst cosine {c[3][0]:.7f} ({c[0]}), beyond 2 ulp "
          f"{o2[3][1]:.3g} ({o2[0]}), beyond 4 ulp {o4[3][2]:.3g} ({o4[0]})")
    if eng.h16 == torch.float16:
        for i, row in enumerate(rows):
            key = row[0]
            if wants_rms[key] < 2.0 ** -10 and all(lb.startswith("dw_dgrad:") for lb in eng.joins.writers[key]):
                k = _rerun_in_range(cuda, eng, key)
                want = FR.expected(eng, key)
                fig = J.figures(eng.grad[key], want)
                print(f"  {key}: rms {wants_rms[key]:.3g}, first pass {tuple(float(f'{v:.4g}') for v in row[3])}; with the writers' "
                      f"inputs times 2^{k}: {tuple(float(f'{v:.4g}') for v in fig)}")
                rows[i] = (key, row[1], want.numel(), fig, J.accept(fig, want.numel()))
    unchecked = set(keys_) - {r[0] for r in rows}
    assert len(unchecked) == 0 <= UNCHECKED_CAP
    bad = [(r[0], r[1], r[2], tuple(float(f"{v:.4g}") for v in r[3])) for r in rows if not r[4]]
    assert not bad, f"{len(bad)} of {len(rows)} buffers miss cos > 0.9999 / 2 ulp < 2e-2 / 4 ulp < 5e-3: {bad[:12]}"


# ---- 5: same trainable gradients as without the freeze ---------------------------------------------------------------------------
def _gradients(cuda, s):
    eng = s.eng
    with torch.cuda.device(cuda):
        eng._step_args = dict(wdc=0.0, alpha=0.0, unscale=1.0, clip=0.0)
        eng._prepack_dgrad_weights()
        preds = eng.forward(s.images)
        s.model.loss(s.targets, preds, compute_grads=True, grad_scale=1.0, grads_bf16=eng.loss_grad_buffers(), normalizer=None)
        eng._train_step_active = True
        try:
            eng.backward(None)
        finally:
            eng._train_step_active = False
        torch.cuda.synchronize()
    return {k: eng._pview(k, eng.G).double().cpu() for k in eng.train_names}


def test_trainable_gradients_equal_those_without_the_freeze(cuda):
    """Every BatchNorm frozen in both engines, so the forward passes compute the same function: ["bn", "fpn"] against ["bn"]
    on ResNet-14, same weights, same batch.  Every variable that trains in both gets the same gradient, within the
    project's weight-gradient bound against float64 (test_gpu_frozen_bn.py:521-525: cosine > 0.9999, 2e-3 relative) with
    the unfrozen engine's gradient as the reference.  Bit-equal tensors are reported."""
    a, b = _build(cuda, "resnet14", ["bn", "fpn"], weight_decay=False), _build(cuda, "resnet14", ["bn"], weight_decay=False)
    for k in a.model.variables:
        assert torch.equal(a.model.variables[k], b.model.variables[k]), k
    ga, gb = _gradients(cuda, a), _gradients(cuda, b)
    common = [k for k in a.eng.train_names if k in gb]
    assert set(common) == set(a.eng.train_names) and len(common) < len(gb)
    assert any(k.startswith("conv2d") for k in common) and any(k.startswith("box-head") for k in common)
    bits, bad = 0, []
    for k in common:
        x, y = ga[k].reshape(-1), gb[k].reshape(-1)
        if torch.equal(x, y):
            bits += 1
            continue
        cos = (x @ y / (x.norm() * y.norm() + 1e-300)).item()
        rel = ((x - y).norm() / (y.norm() + 1e-300)).item()
        if not (cos > 0.9999 and rel < 2e-3):
            bad.append((k, cos, rel))
    print(f"gradients with the FPN frozen against without: {len(common)} variables, {bits} bit-equal")
    assert not bad, bad[:8]
    assert all(float(gb[k].abs().sum()) > 0 for k in common if k.endswith("kernel"))


# ---- 6: drop_connect under a frozen backbone -------------------------------------------------------------------------------------
def test_drop_connect_stays_on_under_a_frozen_backbone(cuda):
    """EfficientNet-B0, ["backbone"]: the model is still called with training=True, so a frozen MBConv skip block draws its
    per-image factor every step.  Its output, in float64 from its boundary tensors: rb(factor[n] BN_inference(conv(x))) +
    skip.  Bounds: the forward checks of test_bottleneck_tail_with_frozen_batchnorm_tight (test_gpu_frozen_bn.py:490, :492 —
    beyond 2 ulp < 2e-3 for the raw conv output, < 3e-3 for the block output)."""
    s = _build(cuda, "efficientnet-b0", ["backbone"])
    eng, var = s.eng, s.model.variables
    blocks = [o for o in eng.ops if o.get("survival") is not None]
    assert len(blocks) == 9 and set(eng.dc_masks) == {o["out"] for o in blocks}
    assert all(not eng._conv_trainable(o) and not eng.requires[o["out"]] for o in blocks)
    rb = lambda t: t.to(eng.h16).double()
    f64 = lambda k: var[k].to(cuda).double()
    seen = []
    for step in range(4):
        with torch.cuda.device(cuda):
            eng.forward(s.images)            # draws
            torch.cuda.synchronize()
        for op in blocks:
            m, p = eng.dc_masks[op["out"]]
            factor = m.double()
            assert all(f in (0.0, pytest.approx(1.0 / p, rel=1e-6)) for f in factor.tolist()), (op["out"], factor.tolist(), p)
            seen += factor.tolist()
            x, skip = eng.t[op["inp"]].double(), eng.t[op["residual"]].double()
            w = rb(var[op["conv"] + "/kernel"].to(cuda))[0, 0]
            scale = f64(op["bn"] + "/gamma") / torch.sqrt(f64(op["bn"] + "/moving_variance") + eng.eps)
            shift = f64(op["bn"] + "/beta") - f64(op["bn"] + "/moving_mean") * scale
            y64 = x @ w
            assert _ulp_outliers(eng.raw[op["out"]], y64, 2.0) < 2e-3, (step, op["out"])                 # :490
            out64 = rb(rb(rb(y64) * scale + shift) * factor[:, None, None, None]) + skip
            assert _ulp_outliers(eng.t[op["out"]], out64, 2.0) < 3e-3, (step, op["out"])                 # :492
            for n in range(B):
                if factor[n] == 0:           # a dropped block hands the skip through, bit for bit
                    assert torch.equal(eng.t[op["out"]][n], eng.t[op["residual"]][n])
    assert 0.0 in seen and any(f > 1.0 for f in seen), "the factors never dropped / never kept a block in 4 steps"
    assert not all(f == 1.0 for f in seen)


# ---- 7: checkpoint / resume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,keys", [("efficientnet-b0", ["backbone"]), ("resnet14", ["fpn"])],
                         ids=["efficientnet-b0-backbone", "resnet14-fpn"])
def test_checkpoint_resume_with_frozen_layers(cuda, tmp_path, model, keys):
    """test_checkpoint_resume_with_frozen_batchnorm with whole layers frozen: save after one step, restore into a fresh
    engine whose variables — the frozen ones included — start somewhere else; the frozen layers' packed weights, folded
    BatchNorm and data-gradient packs are rebuilt from the restored variables and the next step is bit-equal.  (The
    drop_connect generator is no part of a checkpoint, here or in the reference: the test carries its state over.)"""
    s = _build(cuda, model, keys, seed=7)
    eng = s.eng
    eng.train_step(s.images, s.targets)
    prefix = str(tmp_path / "weights_step_1")
    eng.save_checkpoint(prefix)
    frozen_vars = {k: s.model.variables[k].clone() for k in s.frozen}
    packs = [t.clone() for t in _pack_buffers(eng)]
    rng = eng.dc_generator.get_state()
    want = eng.train_step(s.images, s.targets)["weighted-loss"].item()
    torch.cuda.synchronize()
    s2 = _build(cuda, model, keys, seed=7)
    eng2 = s2.eng
    with torch.no_grad():
        for v in s2.model.variables.values():
            v.add_(0.01)
    eng2.load_from_model()
    if packs:
        assert not any(torch.equal(a, b) for a, b in zip(packs, _pack_buffers(eng2)))      # load_from_model repacked
    eng2.restore_checkpoint(prefix)
    eng2.dc_generator.set_state(rng)
    for k, v in frozen_vars.items():
        assert torch.equal(s2.model.variables[k], v), k
    assert all(torch.equal(a, b) for a, b in zip(packs, _pack_buffers(eng2)))
    assert eng2.step_count == 1
    got = eng2.train_step(s2.images, s2.targets)["weighted-loss"].item()
    torch.cuda.synchronize()
    assert got == want
    assert torch.equal(eng2.P, eng.P) and torch.equal(eng2.V, eng.V) and torch.equal(eng2.E, eng.E)
    eng2.store_to_model()
    for k, v in frozen_vars.items():
        assert torch.equal(s2.model.variables[k], v), k


# ---- 8: executor path --------------------------------------------------------------------------------------------------------------
def test_executor_path_backbone_on_efficientnet(cuda):
    """The executor's own route (test_gpu_frozen_bn.py::test_executor_path_backbone_bn), fine_tuning.fine_tune off:
    Executor._maybe_freeze_layers marks the backbone's LAYERS (stem, blocks_i), the model hands their variables to
    `train_engine` as frozen names; two steps."""
    from retinanet.executor import Executor
    from retinanet.model import ModelBuilder
    p = _params("efficientnet-b0", ["backbone"])
    assert not p.fine_tuning.fine_tune
    builder = ModelBuilder(p, "train", device=cuda, seed=5)
    net = builder()
    _randomize(net, 5, cuda)
    assert Executor._maybe_freeze_layers(SimpleNamespace(params=p, model_builder=builder, _model=net))
    eng = net.train_engine(B, world_size=1)
    backbone = {k for k in net.variables if k.startswith("efficientnet-b0/")}
    assert backbone and eng.frozen == backbone and not set(eng.train_names) & backbone
    assert all(k.startswith(("fpn", "box-head", "class-head")) for k in eng.train_names)
    before = {k: net.variables[k].clone() for k in backbone}
    net.optimizer.lr = lambda step: 0.01
    images, targets = _batch(p, cuda, SIZE, B, 5)
    w0 = eng.P.clone()
    losses = [float(eng.train_step(images, targets)["weighted-loss"].item()) for _ in range(2)]
    torch.cuda.synchronize()
    eng.finish_step()
    assert all(np.isfinite(losses)), losses
    assert not torch.equal(eng.P, w0) and bool(torch.isfinite(eng.P).all())
    eng.store_to_model()
    assert all(torch.equal(net.variables[k], v) for k, v in before.items())


# ---- 9: the refusals that remain -----------------------------------------------------------------------------------------------
def test_refusals_that_remain(cuda):
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    # one level of a grouped launch frozen: no freeze pattern splits a group
    with pytest.raises(NotImplementedError, match="mixes frozen and live"):
        _build(cuda, "resnet14", [], regexes=[re.compile(r"^fpn/p3-out-")])
    from retinanet.model import ModelBuilder as MB
    with pytest.raises(NotImplementedError, match="mixes frozen and live kernels"):     # every BatchNorm frozen, one kernel of two
        _build(cuda, "resnet14", [], regexes=[MB.FREEZE_VARS_REGEX["bn"], re.compile(r"^box-head/box-head-1-conv2d/")])
    with pytest.raises(NotImplementedError, match="frozen conv under a trainable BatchNorm"):
        _build(cuda, "resnet14", [], regexes=[re.compile(r"^box-head/box-head-1-conv2d/")])
    # a frozen squeeze-excite above a live layer: no backward without its weight gradients
    with pytest.raises(NotImplementedError, match="squeeze-excite .*blocks_3/se is frozen while layers below it train"):
        _build(cuda, "efficientnet-b0", [], regexes=[re.compile(r"blocks_3/se/")])
    # half a layer: the reference freezes whole layers
    with pytest.raises(ValueError, match="freeze patterns split a layer"):
        _build(cuda, "resnet14", [], regexes=[re.compile(r"^fpn/.*/kernel$")])
    # the auxiliary head under `backbone` / `resnet_initial` (test_gpu_aux_head.py:449-455)
    import test_gpu_aux_head as AH
    builder = ModelBuilder(AH._params(True, 1.0), "train", device=cuda)
    for key in ("resnet_initial", "backbone"):
        with pytest.raises(NotImplementedError, match=AH.HEAD):
            TrainEngine(builder(), AH.B, frozen_regexes=[builder.FREEZE_VARS_REGEX[key]])


# ---- data parallel: what a frozen layer does not send ---------------------------------------------------------------------------
def test_frozen_layers_send_no_syncbn_message_and_no_gradient_bucket(cuda):
    """One rank planned as one of two (world_size = 2, use_sync on), its collectives replaced by a counter: the forward and
    backward pass send one SyncBN message each per LIVE BatchNorm launch group and none for a frozen BatchNorm; the
    gradient-bucket layout covers the trainable variables' slices of the arena and nothing else."""
    from retinanet.model import ModelBuilder
    from retinanet.model.data_parallel import plan_buckets
    from retinanet.model.train_engine import TrainEngine
    p = _params("resnet14", ["backbone"])
    p.architecture.batch_norm.use_sync = True
    builder = ModelBuilder(p, "train", device=cuda, seed=5)
    net = builder()
    _randomize(net, 5, cuda)
    rx = [builder.FREEZE_VARS_REGEX["backbone"]]
    eng = TrainEngine(net, B, frozen_regexes=rx, world_size=2)
    frozen = {k for k in net.variables if rx[0].search(k)}
    assert eng.sync_bn and eng.dp_active
    live = [g for g in eng.bn_groups.values() if not g.frozen]
    assert live and all(o["bn"].startswith(("fpn", "box-head", "class-head")) for g in live for o in g.ops)
    assert all(g.sums is None and g.bsums is None for g in eng.bn_groups.values() if g.frozen)
    assert not any(b + "/gamma" in frozen for g in live for b in (o["bn"] for o in g.ops))
    sent = []
    eng.small.all_reduce = lambda t: sent.append(t.numel())      # (one rank: the sum over the ranks is the tensor itself)
    images, targets = _batch(p, cuda, SIZE, B, 5)
    with torch.cuda.device(cuda):
        eng.small.begin_step(targets["num-positives"], carry_normalizer=False)
        preds = eng.forward(images)
        forward_messages = len(sent)
        g = torch.Generator().manual_seed(99)
        eng.backward({k: {lv: torch.randn(preds[k][lv].shape, generator=g).to(cuda) for lv in preds[k]} for k in preds})
        torch.cuda.synchronize()
    assert forward_messages == len(live) and len(sent) == 2 * len(live)
    eng.small.count = len(sent)
    eng.syncbn_messages_per_step = eng.small.end_step()
    assert eng.syncbn_messages_per_step == 2 * len(live)
    # gradient buckets
    buckets, _ = plan_buckets(eng.train_names, eng.p_off, eng._seg_blocks, eng._ready_steps(), 1 << 20)
    covered = torch.zeros((eng.P.numel(),), dtype=torch.bool)
    for bkt in buckets:
        covered[bkt["begin"]:bkt["end"]] = True
    assert not set(eng.p_off) & frozen and not set(eng._seg_blocks) & frozen
    for k in eng.train_names:
        off, n = eng.p_off[k]
        assert bool(covered[off:off + n].all()), k
    assert int(covered.sum()) <= 4 + sum((n + 3) // 4 * 4 for _, n in eng.p_off.values())
    assert buckets[-1]["end"] == eng.P.numel() == eng.n_params
