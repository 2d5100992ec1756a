"""CPU: the FPN builder with the weighted FeatureFusion modes, and the teeth of tests/fusion_ref.py."""
import pytest
import torch

import act_ref as A
import fusion_ref as FR
import pyramid_ref as R

DTYPES = [torch.bfloat16, torch.float16]
MODES = ["fast_attention", "fast_channel_attention"]


def _graph(mode):
    from retinanet.cfg import default_params
    from retinanet.model.graph import build_retinanet_graph, init_variables
    p = default_params(input_size=640)
    p.architecture.feature_fusion.fusion_mode = mode
    g = build_retinanet_graph(p)
    return p, g, init_variables(g)


def _trainable(g, v):
    return [k for k in v if g.var_specs[k].get("trainable", True)]


# ---- graph ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_weighted_modes_register_two_variables_per_fusion(mode):
    _, g0, v0 = _graph("sum")
    p, g, v = _graph(mode)
    ff = p.architecture.feature_fusion
    F = int(ff.filters)
    names = [n for level in range(ff.min_level + 1, ff.max_level + 1) for n in FR.var_names(level)]
    assert len(names) == 8 and names[0] == ("fpn/p3-in-fusion-with-p4-in-upsampled/"
                                            "p3-in-fusion-with-p4-in-upsampled-lower-level-weight")
    assert names[-1] == "fpn/p6-in-fusion-with-p7-in-upsampled/p6-in-fusion-with-p7-in-upsampled-upper-level-weight"
    assert [k for k in v if k not in v0] == names and [k for k in v0 if k not in v] == []
    shape = (1,) if mode == "fast_attention" else (F,)
    for n in names:
        assert tuple(v[n].shape) == shape and v[n].dtype == torch.float32 and bool((v[n] == 1).all())
        assert g.var_specs[n].get("trainable", True)
    t0, t = _trainable(g0, v0), _trainable(g, v)
    assert len(t) == len(t0) + 8 == 303
    per = 1 if mode == "fast_attention" else F
    assert sum(v[k].numel() for k in t) == sum(v0[k].numel() for k in t0) + 8 * per == 34389556 + 8 * per
    op = next(o for o in g.ops if o["op"] == "topdown")
    assert op["fusion"] == mode
    assert [n for pair in op["fusion_vars"] for n in pair] == names
    for k in v0:   # every other variable is what 'sum' builds
        assert torch.equal(v[k], v0[k]), k


def test_sum_mode_graph_is_unchanged():
    _, g, v = _graph("sum")
    t = _trainable(g, v)
    assert len(t) == 295 and sum(v[k].numel() for k in t) == 34389556
    op = next(o for o in g.ops if o["op"] == "topdown")
    assert sorted(op) == ["act", "ins", "op", "outs"]
    assert not [k for k in g.var_specs if "fusion" in k]


def test_unknown_mode_raises_the_reference_assertion():
    with pytest.raises(AssertionError, match="Requested unsupported mode: bogus, available modes are: "
                                             r"\['sum', 'fast_attention', 'fast_channel_attention'\]"):
        _graph("bogus")


# ---- the forward reference ---------------------------------------------------------------------------------------------
def _sweep_pair(dtype):
    lo = A.sweep(dtype)                                              # every finite value of the type
    up = R.grid(lo.shape, torch.Generator().manual_seed(5), dtype)   # multiples of 1/4 in [-2, 2]
    return lo, up


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", FR.WEIGHT_PAIRS)
def test_forward_reference_is_torchs_per_op_arithmetic(dtype, w):
    lo, up = _sweep_pair(dtype)
    k = FR.Coef([w[0]], [w[1]], dtype)
    assert FR.same_values(FR.fuse_z(lo, up, k), FR.fuse_torch(lo, up, [w[0]], [w[1]]))
    if w == (1.0, 1.0):
        assert float(k.s) == 2.0    # 2 + 1e-4 rounds to 2 in both types


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", [FR.WEIGHT_PAIRS[1], FR.WEIGHT_PAIRS[4], (0.45, 1.2)])
def test_coefficient_form_is_rejected(dtype, w):
    """in * (a_l / s) + up * (a_u / s) with one rounding is another function: it differs from the contract on 8 000 to
    20 000 of the 65 536 inputs for every pair whose quotients a / s are no powers of two.  (For (1, 1), (-0.3, 0.5) and
    (0, 0) they are 1/2, 0, 1 or 2^-k-exact and the two forms coincide: those pairs cannot tell them apart.)"""
    lo, up = _sweep_pair(dtype)
    k = FR.Coef([w[0]], [w[1]], dtype)
    want, other = FR.fuse_z(lo, up, k), FR.fuse_coefficient_form(lo, up, k)
    assert not FR.same_values(other, want)
    differ = int((other.view(torch.int16) != want.view(torch.int16)).sum())
    assert differ > 1000, differ


# ---- the backward reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", ["none", "relu", "relu6"])
def test_backward_reference_equals_autograd(mode, act):
    g = torch.Generator().manual_seed(11)
    N, H0, W0, C, L = 2, 8, 4, 8, 3
    ins = [torch.randn((N, H0 >> l, W0 >> l, C), generator=g, dtype=FR.F64) * 3 for l in range(L)]
    douts = [torch.randn(ins[l].shape, generator=g, dtype=FR.F64) for l in range(L)]
    n = 1 if mode == "fast_attention" else C
    ws = [[torch.rand((n,), generator=g, dtype=FR.F64) * 2 + 0.1 for _ in range(2)] for _ in range(L - 1)]
    ws[0][0][0] = -0.4     # a weight <= 0: its gradient is exactly 0
    if n > 1:
        ws[1][1][3] = 0.0
    leaves = [t.requires_grad_(True) for t in ins] + [w.requires_grad_(True) for pair in ws for w in pair]
    outs = FR.topdown_exact(ins, ws, act)
    sum((o * d).sum() for o, d in zip(outs, douts)).backward()
    with torch.no_grad():
        coefs = [FR.exact_coef(*pair) for pair in ws]
        dins, dws, gs = FR.topdown_bwd(douts, ins, [o.detach() for o in outs], coefs, ws, act, None)
    for l in range(L):
        assert (dins[l] - ins[l].grad).abs().max() <= 1e-12 * ins[l].grad.abs().max(), l
    for j in range(L - 1):
        # Where the PARTNER weight is <= 0 the gradient is S (s - a) / s^2 with s - a = 1e-4 left of a cancellation: the
        # float64 subtraction alone is off by 1e-16 / 1e-4 = 1e-12 of the result, in this formula and in autograd's alike.
        # Those elements are judged relative to the size of the formula's terms, max(|Sl|, |Su|) / s, as the GPU test
        # judges dw; every other element relative to the gradient itself.
        Sl, Su, _, _ = FR.level_sums(gs[j], ins[j].detach(), outs[j + 1].detach())
        if n == 1:
            Sl, Su = Sl.sum().reshape(1), Su.sum().reshape(1)
        scale = torch.maximum(Sl.abs(), Su.abs()) / coefs[j][2]
        for got, w, partner in zip(dws[j], ws[j], ws[j][::-1]):
            err, well = (got - w.grad).abs(), partner.detach() > 0
            assert bool((err[~well] <= 1e-12 * scale[~well]).all()), j
            if bool(well.any()):
                assert err[well].max() <= 1e-12 * w.grad[well].abs().max(), j
    assert float(dws[0][0][0]) == 0.0 and float(ws[0][0].grad[0]) == 0.0
    assert len(leaves) == L + 2 * (L - 1)


def test_whole_network_reference_falls_back_to_the_oracle_for_sum():
    """FusedRefModel is oracle/model_ref.py's RefModel wherever the fusion mode is 'sum'"""
    from model_ref import RefModel
    from retinanet.cfg import default_params
    from retinanet.model.graph import build_retinanet_graph, init_variables
    p = default_params(input_size=128)
    p.architecture.backbone.depth = 14
    v = init_variables(build_retinanet_graph(p))
    x = torch.randn((1, 128, 128, 3), generator=torch.Generator().manual_seed(2))
    a, b = RefModel(p, v, emulate_bf16=True)(x), FR.FusedRefModel(p, v, emulate_bf16=True)(x)
    for key in ("class-predictions", "box-predictions"):
        for lv in a[key]:
            assert torch.equal(a[key][lv], b[key][lv])
    p.architecture.feature_fusion.fusion_mode = "fast_channel_attention"
    v = init_variables(build_retinanet_graph(p))
    c = FR.FusedRefModel(p, v, emulate_bf16=True)(x)
    assert not torch.equal(a["box-predictions"]["3"], c["box-predictions"]["3"])   # ones: (x + up) / 2, not x + up
