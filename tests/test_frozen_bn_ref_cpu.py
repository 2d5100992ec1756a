"""CPU: the frozen-BatchNorm reference (frozen_bn_ref.py) against central finite differences of its own float64 forward,
its fp32 / storage form against the float64 one, and the four `*-bn` freeze patterns on the variable lists of ResNet-50
and EfficientNet-B0."""
import numpy as np
import pytest
import torch

import frozen_bn_ref as F

P, C, ROWS = 24, 16, 6            # 4 images of 6 rows


def _inputs(act, residual, seed=0):
    """points at least 0.05 away from the kinks of relu / relu6 (0 and 6): a central difference of width 1e-6 never
    straddles one"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-3.0, 3.0, (P, C))
    scale = rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C)
    shift = rng.uniform(-1.0, 1.0, C)
    res = rng.uniform(-2.0, 2.0, (P, C)) if residual else None
    m = np.array([0.0, 1.25, 1.25, 0.0])
    for _ in range(50):
        for mm in (None, m):
            pre = F.forward(y, scale, shift, act, res, mm, ROWS)["pre"]
            bad = (np.abs(pre) < 0.05) | (np.abs(pre - 6.0) < 0.05)
            y = np.where(bad, y + 0.13, y)
    return y, scale, shift, res, m, rng.standard_normal((P, C))


@pytest.mark.parametrize("drop_connect", [False, True])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("act", F.ACTS)
def test_backward_is_the_derivative_of_the_float64_forward(act, residual, drop_connect):
    """L = sum(dz * z): dL/dy = dy and dL/dresidual = dres of the reference, against (L(+h) - L(-h)) / 2h per element (the
    function is elementwise, so all elements are perturbed at once).  h = 1e-6: truncation h^2 |f'''| / 6 < 1e-12,
    cancellation 2^-52 |z| / h < 1e-9 — bound 1e-7 relative to max(1, |value|)."""
    y, scale, shift, res, m, dz = _inputs(act, residual)
    m = m if drop_connect else None
    fwd = F.forward(y, scale, shift, act, res, m, ROWS)
    bwd = F.backward(dz, scale, act, fwd, m, ROWS)
    h = 1e-6
    z = lambda yy, rr: F.forward(yy, scale, shift, act, rr, m, ROWS)["z"]
    fd_y = dz * (z(y + h, res) - z(y - h, res)) / (2 * h)
    assert np.all(np.abs(fd_y - bwd["dy"]) <= 1e-7 * np.maximum(1.0, np.abs(fd_y)))
    if residual:
        fd_r = dz * (z(y, res + h) - z(y, res - h)) / (2 * h)
        assert np.all(np.abs(fd_r - bwd["dres"]) <= 1e-7 * np.maximum(1.0, np.abs(fd_r)))
        if drop_connect:     # a dropped image: no gradient into the BatchNorm branch, the skip gradient untouched
            assert np.all(bwd["dy"][:ROWS] == 0) and np.any(bwd["dres"][:ROWS] != 0)
    if act in ("relu", "relu6"):
        assert 0 < (bwd["g"] != 0).sum() < bwd["g"].size      # the gate opens and closes on these inputs
    acc = F.backward(dz, scale, act, fwd, m, ROWS, dres0=np.ones((P, C)))
    assert np.array_equal(acc["dres"], bwd["dres"] + 1.0) and np.array_equal(acc["dy"], bwd["dy"])


def test_a_live_batchnorm_backward_is_rejected():
    """the test has teeth: the mean / xhat terms of a training-mode BatchNorm are far outside the bound"""
    y, scale, shift, res, m, dz = _inputs("none", False)
    fwd = F.forward(y, scale, shift, "none")
    bwd = F.backward(dz, scale, "none", fwd)
    live = scale * (dz - dz.mean(0))
    h = 1e-6
    fd = dz * (F.forward(y + h, scale, shift, "none")["z"] - F.forward(y - h, scale, shift, "none")["z"]) / (2 * h)
    assert np.all(np.abs(fd - bwd["dy"]) <= 1e-7 * np.maximum(1.0, np.abs(fd)))
    assert not np.all(np.abs(fd - live) <= 1e-7 * np.maximum(1.0, np.abs(fd)))


@pytest.mark.parametrize("storage", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", F.ACTS)
def test_storage_form_follows_the_float64_form(act, storage):
    """fp32 arithmetic + storage roundings on storage-valued inputs: z, dy and dres within 2 storage steps of the float64
    values wherever the gate agrees (a rounded pre-activation may fall on the other side of a kink), stored as storage
    values"""
    rng = np.random.default_rng(1)
    q = lambda a: torch.from_numpy(a).to(storage).to(torch.float32).numpy()
    y, res, dz = q(rng.uniform(-3, 3, (P, C))), q(rng.uniform(-2, 2, (P, C))), q(rng.standard_normal((P, C)))
    scale, shift = rng.uniform(0.5, 2.0, C).astype(np.float32), rng.uniform(-1, 1, C).astype(np.float32)
    f64 = F.forward(y, scale, shift, act, res)
    b64 = F.backward(dz, scale, act, f64)
    f32 = F.forward(y, scale, shift, act, res, storage=storage, fp=np.float32)
    b32 = F.backward(dz, scale, act, f32, storage=storage, fp=np.float32)
    eps = 2.0 ** -7 if storage == torch.bfloat16 else 2.0 ** -10
    same_gate = (b64["g"] != 0) == (b32["g"] != 0)
    assert same_gate.mean() > 0.95
    # the pre-activation carries the rounding of the BatchNorm output u (half a step of |u|) and, in front of swish, of the
    # sum (half a step of |pre|): dpre <= eps (|u| + |pre|) with room for the fp32 operations; |act'| <= 1.1, |swish''| <= 0.5
    u = y.astype(np.float64) * scale + shift
    dpre = eps * (np.abs(u) + np.abs(f64["pre"]))
    dgate = 0.5 * dpre if act == "swish" else 0.0
    for a, b, extra in ((f32["z"], f64["z"], 1.1 * dpre), (b32["dy"], b64["dy"], np.abs(dz * scale) * dgate),
                        (b32["dres"], b64["dres"], np.abs(dz) * dgate)):
        assert a.dtype == np.float32 and np.array_equal(q(a.astype(np.float64)), a)
        assert np.all((np.abs(a - b) <= eps * np.abs(b) + extra + 1e-30) | ~same_gate)


def test_gate_bits_layout():
    z = np.zeros((2, 16), dtype=np.float32)
    z[0, 0], z[0, 9], z[1, 7], z[1, 8] = 1.0, 6.0, 5.5, 0.0
    assert F.gate_bits(z, "relu").tolist() == [1, 2, 128, 0]
    assert F.gate_bits(z, "relu6").tolist() == [1, 0, 128, 0]


def test_fold_matches_fold_bn():
    from retinanet.model.forward import fold_bn
    g = torch.Generator().manual_seed(3)
    v = {"bn/gamma": torch.rand(32, generator=g) + 0.5, "bn/beta": torch.randn(32, generator=g),
         "bn/moving_mean": torch.randn(32, generator=g), "bn/moving_variance": torch.rand(32, generator=g) + 0.25}
    scale, shift, _ = fold_bn(v, "bn", None, 1e-3, torch.device("cpu"))
    want = F.fold(v["bn/gamma"].numpy(), v["bn/beta"].numpy(), v["bn/moving_mean"].numpy(), v["bn/moving_variance"].numpy(),
                  1e-3, np.float64)
    np.testing.assert_allclose(scale.numpy(), want[0], rtol=3e-7)
    np.testing.assert_allclose(shift.numpy(), want[1], rtol=1e-6, atol=1e-6)


def _graphs():
    from retinanet.cfg import default_params, efficientnet_params
    from retinanet.model.graph import build_retinanet_graph
    return {"resnet50": build_retinanet_graph(default_params()),
            "efficientnet-b0": build_retinanet_graph(efficientnet_params("efficientnet-b0", input_size=512))}


@pytest.mark.parametrize("net", ["resnet50", "efficientnet-b0"])
def test_bn_freeze_patterns_select_exactly_the_batchnorm_variables_of_their_scope(net):
    """`bn`, `backbone-bn`, `fpn-bn`, `head-bn` (model/builder.py:19-30) on the variable list of the graph: every
    BatchNorm variable of the scope — gamma, beta and both moving statistics, found through the graph's BatchNorm
    table — and nothing else: no kernel, no bias, no BatchNorm of another scope."""
    from retinanet.model.builder import ModelBuilder
    g = _graphs()[net]
    names = list(g.var_specs)
    scopes = F.bn_variable_scopes(g)
    assert all(len(v) >= 8 for v in scopes.values()), {k: len(v) for k, v in scopes.items()}
    want = {"bn": scopes["backbone"] | scopes["fpn"] | scopes["head"], "backbone-bn": scopes["backbone"],
            "fpn-bn": scopes["fpn"], "head-bn": scopes["head"]}
    for key, expect in want.items():
        rx = ModelBuilder.FREEZE_VARS_REGEX[key]
        got = {k for k in names if rx.search(k)}
        assert got == expect, (key, sorted(got ^ expect)[:6])
        assert not any(k.rsplit("/", 1)[-1] in ("kernel", "bias", "depthwise_kernel", "pointwise_kernel") for k in got)
    trainable = [k for k in names if g.var_specs[k].get("trainable", True)]
    frozen = {k for k in trainable if ModelBuilder.FREEZE_VARS_REGEX["bn"].search(k)}
    assert frozen == {k for k in want["bn"] if k.endswith(("/gamma", "/beta"))}
    assert any(k.endswith("kernel") for k in trainable if k not in frozen)


def test_frozen_bn_variables_never_carry_weight_decay():
    """executor.py:308-327 decays variables whose name holds 'kernel' (conv layers) or 'kernel' / 'weight' (other
    layers): no BatchNorm variable does, frozen or not, so a `*-bn` key changes nothing in the decayed set"""
    for g in _graphs().values():
        for names in F.bn_variable_scopes(g).values():
            assert not any("kernel" in k.rsplit("/", 1)[-1] or "weight" in k.rsplit("/", 1)[-1] for k in names)


def _freeze_like_the_executor(net, key):
    """Executor._maybe_freeze_layers / _get_weight_decay_variables on a CPU model: (frozen names, decayed names, model)"""
    from types import SimpleNamespace
    from retinanet.cfg import default_params, efficientnet_params
    from retinanet.executor import Executor
    from retinanet.model.builder import ModelBuilder, RetinaNetModel
    from retinanet.model.graph import build_retinanet_graph, init_variables
    p = default_params(freeze=[key] if key else []) if net == "resnet50" else efficientnet_params("efficientnet-b0", input_size=512)
    if net != "resnet50":
        p.training.freeze_variables = [key] if key else []
    g = build_retinanet_graph(p)
    model = RetinaNetModel(p, g, init_variables(g), "cpu")
    stub = SimpleNamespace(params=p, model_builder=ModelBuilder, _model=model)
    assert Executor._maybe_freeze_layers(stub) == bool(key)
    return model.frozen_variable_names, Executor._get_weight_decay_variables(stub), model


def test_executor_freezes_by_layer_like_the_reference():
    """executor.py:154-176 sets `trainable = False` on the LAYER that owns a matching variable.  ResNet's BatchNorm layers are
    layers of their own, so `backbone-bn` freezes exactly their variables, the kernels stay trainable and the weight-decay
    list is what it is without the key (no BatchNorm variable is ever decayed).  `fpn`, `box-head` and `class-head` are ONE
    custom layer each (model/builder.py RetinaNetModel.layers): `fpn-bn` / `head-bn` / `bn` freeze them whole, kernels
    included, as in the reference — frozen BatchNorm alone inside those layers is reached with variable-level patterns
    (TrainEngine(frozen_regexes=...), RetinaNetModel.freeze)."""
    _, decayed_all, model = _freeze_like_the_executor("resnet50", None)
    scopes = F.bn_variable_scopes(model.graph)
    frozen, decayed, _ = _freeze_like_the_executor("resnet50", "backbone-bn")
    assert frozen == scopes["backbone"] and decayed == decayed_all
    assert not any("normalization" in n for n in decayed_all)
    frozen, decayed, _ = _freeze_like_the_executor("resnet50", "fpn-bn")
    assert frozen == {k for k in model.variables if k.startswith("fpn/")}
    assert set(decayed) == {k for k in decayed_all if not k.startswith("fpn/")}
    frozen, _, _ = _freeze_like_the_executor("resnet50", "head-bn")
    assert frozen == {k for k in model.variables if k.startswith(("box-head/", "class-head/"))}
    # EfficientNet: stem and every block are one layer each
    frozen, _, m = _freeze_like_the_executor("efficientnet-b0", "backbone-bn")
    assert frozen == {k for k in m.variables if k.startswith("efficientnet-b0/")}
