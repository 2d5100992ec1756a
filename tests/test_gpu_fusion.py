"""GPU: the weighted FPN top-down fusion (FeatureFusion modes fast_attention / fast_channel_attention) from the kernels
(rn_fpn_topdown_fused, rn_fpn_fused_bwd_level, rn_fpn_fused_bwd_finalize) up through the inference engine, the training
engine and the optimizer step, against tests/fusion_ref.py.

The forward is compared BIT FOR BIT with the per-op fp32-plus-rounding reference (one rounding per TF op); swish on top of
the exact pre-activation with act_ref's swish slack.  The backward tensors follow pyramid_ref's acceptance rule against
float64; the weight-gradient sums are bounded by the length of the fp32 addition chains of the reduction."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import act_ref as A
import fusion_ref as FR
import pyramid_ref as R

pytestmark = pytest.mark.gpu

H16 = torch.bfloat16
_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BUILDS = ["bf16", "f16"]
MODES = ["fast_attention", "fast_channel_attention"]
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _storage_type(request):
    global H16
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    H16 = _DT[params.get("build", "bf16")]
    yield
    H16 = torch.bfloat16


def _lib():
    from retinanet import _C
    return _C.lib(H16 == torch.float16)


def _weights(mode, C, pairs):
    """one fusion's (w_l, w_u) f32: per channel cycling through `pairs`, or the first pair as two scalars"""
    n = 1 if mode == "fast_attention" else C
    return (torch.tensor([pairs[c % len(pairs)][0] for c in range(n)], dtype=torch.float32),
            torch.tensor([pairs[c % len(pairs)][1] for c in range(n)], dtype=torch.float32))


def _random_weights(mode, C, g, fusions):
    """per fusion (w_l, w_u) in [-0.3, 2]; the first element of fusion 0's lower weight negative, of its upper weight 0"""
    n = 1 if mode == "fast_attention" else C
    ws = [[torch.rand((n,), generator=g) * 2.3 - 0.3 for _ in range(2)] for _ in range(fusions)]
    ws[0][0][0] = -0.25
    if n > 1:
        ws[0][1][1] = 0.0
    elif fusions > 1:
        ws[1][1][0] = 0.0
    return [tuple(pair) for pair in ws]


class Fused:
    """device side of one rn_fpn_topdown_fused call: weights, coefficient blocks, outputs pre-filled with a sentinel"""

    def __init__(self, cuda, ins, ws, act, mode):
        from retinanet import _C
        lib = _lib()
        self.L, (self.N, self.H0, self.W0, self.C) = len(ins), ins[0].shape
        self.mode_id = _C.FUSION_IDS[mode]
        self.ins = [t.to(cuda).contiguous() for t in ins]
        self.outs = [torch.full_like(t, SENTINEL) for t in self.ins[:-1]] + [self.ins[-1]]
        self.w = [(a.to(cuda), b.to(cuda)) for a, b in ws]
        self.coef = [torch.zeros((lib.rn_fpn_fusion_coef_bytes(self.C),), dtype=torch.uint8, device=cuda) for _ in ws]
        self.args = (_C.ptr_array(self.ins), _C.ptr_array(self.outs), _C.ptr_array([w[0] for w in self.w]),
                     _C.ptr_array([w[1] for w in self.w]), _C.ptr_array(self.coef), self.L, self.N, self.H0, self.W0,
                     self.C, _C.ACT_IDS[act], self.mode_id)
        self.launches = lib.rn_fpn_topdown_fused_launches(self.L, self.N, self.H0, self.W0, self.C)

    def run(self):
        from retinanet import _C
        _C.check(_lib().rn_fpn_topdown_fused(*self.args, _C.current_stream()), "rn_fpn_topdown_fused")
        torch.cuda.synchronize()
        return [o.cpu() for o in self.outs]


def _coefs(ws):
    return [FR.Coef(w_l, w_u, H16) for w_l, w_u in ws]


# ---- 1. forward on every input -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", A.ACTS)
def test_fused_forward_on_every_input(cuda, build, mode, act):
    """Two levels; in[0] holds every finite value of the storage type, in[1] multiples of 1/4.  The five weight pairs
    (initial, generic, a negative, both zero, one zero) cycle over the channels (fast_channel_attention) or take one
    launch each (fast_attention).  none / relu / relu6: bit for bit, infinities where the formula overflows included.
    swish: act_ref's rule with its swish slack around swish(z), z the exact pre-activation; where z is infinite the
    stored value is +inf for +inf and NaN for -inf (x sigmoid(x) = -inf * 0, in the kernel as in float64)."""
    N, H, W, C = 1, 32, 32, A.C
    x = A.sweep(H16).reshape(N, H, W, C)
    coarse = R.grid((N, H // 2, W // 2, C), torch.Generator().manual_seed(5), H16)
    rounds = [FR.WEIGHT_PAIRS] if mode == "fast_channel_attention" else [[p] for p in FR.WEIGHT_PAIRS]
    for pairs in rounds:
        ws = [_weights(mode, C, pairs)]
        f = Fused(cuda, [x, coarse], ws, act, mode)
        assert f.launches == 1
        got = f.run()[0]
        z = FR.fuse_z(x, R.up(coarse, 2), _coefs(ws)[0])
        what = f"rn_fpn_topdown_fused {mode} {act} {pairs[0] if len(pairs) == 1 else 'five pairs'}"
        if act != "swish":
            want = R.act_fwd(z.float(), act).to(H16)
            differ = int((got.view(torch.int16) != want.view(torch.int16)).sum())
            print(f"{what}: {differ} of {got.numel()} bit patterns differ (signed zeros included)")
            assert FR.same_values(got, want), (what, differ)
            continue
        zf = R.f64(z)
        fin = torch.isfinite(zf)
        ref = torch.where(fin, A.act_fwd(torch.where(fin, zf, torch.zeros_like(zf)), act), torch.zeros_like(zf))
        ok, ratio, outside, worst = A.check(torch.where(fin, got, torch.zeros_like(got)), ref, H16,
                                            A.value_slack(ref, act))
        print(f"{what}: worst |got - ref| / bound = {ratio:.4f}, {outside} outside, {int((~fin).sum())} infinite z")
        assert ok, (what, ratio, outside, zf.reshape(-1)[worst].item())
        gf = got.float()
        assert bool((gf[zf == float("inf")] == float("inf")).all()) and bool(torch.isnan(gf[zf == float("-inf")]).all())


# ---- 2. chains -----------------------------------------------------------------------------------------------------------
def _chain_case(cuda, L, N, H0, W0, C, mode, seed, launches):
    g = torch.Generator().manual_seed(seed)
    ins = [R.grid((N, H0 >> l, W0 >> l, C), g, H16, lim=16) for l in range(L)]
    ws = _random_weights(mode, C, g, L - 1)
    f = Fused(cuda, ins, ws, "relu", mode)
    assert f.launches == launches, f.launches
    got = f.run()
    want = FR.topdown_fwd(ins, _coefs(ws), "relu")
    for l in range(L):
        assert FR.same_values(got[l], want[l]), (l, int((got[l].view(torch.int16) != want[l].view(torch.int16)).sum()))
    assert not bool((got[0] == SENTINEL).all())


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, 40, 256])
def test_fused_forward_chain_five_levels(cuda, build, mode, C):
    """L = 5, N = 2, 32 x 16, other weights in every fusion: every level bit for bit; the single-launch form (every
    thread walks its chain down from the coarsest level)"""
    _chain_case(cuda, 5, 2, 32, 16, C, mode, 41 + C, launches=1)


@pytest.mark.parametrize("build", BUILDS)
def test_fused_forward_chain_in_one_stage_launches(cuda, build):
    """The smallest pyramid the other launch form takes: 2^21 sixteen-byte groups on the finest level (N = 4, 128 x 128,
    C = 256), L = 3 — two launches of one stage per element behind the preparation kernel"""
    assert 4 * 128 * 128 * (256 // 8) == 1 << 21
    assert _lib().rn_fpn_topdown_fused_launches(3, 4, 128, 64, 256) == 1      # half of it: still the single launch
    _chain_case(cuda, 3, 4, 128, 128, 256, "fast_channel_attention", 47, launches=2)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("build", BUILDS)
def test_fused_forward_chain_in_the_training_launch_form(cuda, build):
    """The form the bench and training shapes take (more than three levels, 2^21 or more groups on the finest): a first
    launch for the coarse rest that starts above level 0 — here levels [2, 3), its level search and coefficient cache
    beginning at lo = 2 — then the two finest levels as one-stage launches.  L = 4 at N = 4, 128 x 128, C = 256 is the
    smallest pyramid that takes it.  fast_attention, so that both modes run a cut form."""
    _chain_case(cuda, 4, 4, 128, 128, 256, "fast_attention", 53, launches=3)
    torch.cuda.empty_cache()


def test_fused_forward_validates_like_its_neighbours(cuda):
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(2)
    ins = [R.grid((1, 8 >> l, 8 >> l, 16), g, H16) for l in range(2)]
    f = Fused(cuda, ins, [_weights("fast_attention", 16, FR.WEIGHT_PAIRS[1:2])], "relu", "fast_attention")
    st = _C.current_stream()
    a = list(f.args)
    for i, bad in ((9, 12), (7, 9), (11, 0), (11, 3), (5, 1)):     # C % 8, H0 that does not halve, modes, one level
        b = list(a)
        b[i] = bad
        assert lib.rn_fpn_topdown_fused(*b, st) == _C.RN_EINVAL, (i, bad)
    b = list(a)
    b[4] = None
    assert lib.rn_fpn_topdown_fused(*b, st) == _C.RN_EINVAL
    torch.cuda.synchronize()
    assert bool((f.outs[0] == SENTINEL).all())
    assert lib.rn_fpn_topdown_fused_launches(2, 1, 9, 8, 16) == 0 and lib.rn_fpn_fusion_coef_bytes(16) == 14 * 16


# ---- 3. backward levels ----------------------------------------------------------------------------------------------------
def _reduction_depth(P, C, scalar):
    """Longest chain of fp32 additions a product g * x passes through in the two-stage reduction (csrc/rn_fusion.hip): a
    workgroup is PR = 256 / CB pixels x CB = min(C / 8, 256) channel groups, at most 1024 workgroups along the pixels; a
    thread adds its own pixels in order (ceil(P / (workgroups * PR)) additions), a tree over the PR pixel rows follows
    (ceil(log2 PR)), stage 2 adds every 16th workgroup row in order (ceil(workgroups / 16)) and ends in a tree over 16
    (4); fast_attention adds the channels: every 256th in order, then a tree over 256 (ceil(C / 256) + 8)."""
    CB = min(C // 8, 256)
    PR = 256 // CB
    rows = min(-(-P // PR), 1024)
    d = -(-P // (rows * PR)) + math.ceil(math.log2(PR)) + -(-rows // 16) + 4
    return d + (-(-C // 256) + 8 if scalar else 0), rows


def _bwd_level(cuda, lib, j, L, douts, g_prev, coef_prev, f, act, inplace, stream=None):
    """one rn_fpn_fused_bwd_level (+ finalize below the top) on device tensors -> dict of device results"""
    from retinanet import _C
    N, H, W, C = douts[j].shape
    st = _C.current_stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
    din = torch.full_like(douts[j], SENTINEL)
    if j == L - 1:
        _C.check(lib.rn_fpn_fused_bwd_level(_C.ptr(douts[j]), _C.ptr(g_prev), _C.ptr(coef_prev), None, None, None, None,
                                            None, _C.ptr(din), None, 0, N, H, W, C, _C.RN_ACT_NONE, st), "bwd top")
        return dict(din=din)
    dout = douts[j].clone()
    g = dout if inplace else torch.full_like(dout, SENTINEL)
    nb = lib.rn_fpn_fused_bwd_workspace_bytes(N, H, W, C)
    assert nb == (_reduction_depth(N * H * W, C, False)[1] + 1) * 2 * C * 4
    ws = torch.full((nb,), 0x7f, dtype=torch.uint8, device=cuda)     # NaN-ish garbage: every row read must be written
    n = f.w[j][0].numel()
    sums = torch.full((2, C), SENTINEL, dtype=torch.float32, device=cuda)
    dw = torch.full((2, n), SENTINEL, dtype=torch.float32, device=cuda)
    _C.check(lib.rn_fpn_fused_bwd_level(_C.ptr(dout), _C.ptr(g_prev), _C.ptr(coef_prev), _C.ptr(f.outs[j]),
                                        _C.ptr(f.ins[j]), _C.ptr(f.outs[j + 1]), _C.ptr(f.coef[j]), _C.ptr(g), _C.ptr(din),
                                        _C.ptr(ws), nb, N, H, W, C, _C.ACT_IDS[act], st), "bwd level")
    _C.check(lib.rn_fpn_fused_bwd_finalize(_C.ptr(ws), nb, N, H, W, C, _C.ptr(f.w[j][0]), _C.ptr(f.w[j][1]),
                                           _C.ptr(f.coef[j]), f.mode_id, _C.ptr(sums), dw[0].data_ptr(), dw[1].data_ptr(),
                                           st), "bwd finalize")
    return dict(g=g, din=din, sums=sums, dw=dw)


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", ["none", "relu", "relu6"])
@pytest.mark.parametrize("C", [40, 64])
@pytest.mark.parametrize("L,H0,W0", [(2, 8, 6), (3, 16, 8)])
def test_fused_backward_levels(cuda, build, mode, act, C, L, H0, W0):
    """Every level of the backward, finest first, N = 2; a negative and a zero weight among the channels (or among the
    scalars).  Each level reads the finer level's g as the KERNEL stored it, so a level's reference has no inherited
    uncertainty:
      * g and din inside pyramid_ref's bound |got - ref| <= ulp_s(ref) + n 2^-23 sum|terms| (fusion_ref.level_g: n = 7;
        level_din from the stored g: n = 2); g written in place over dout and out of place: the same bits;
      * Sl, Su against the float64 sums of the exact products g * x: |got - ref| <= d 2^-24 sum|g x| with d the longest
        chain of fp32 additions a term passes through (_reduction_depth; the products are exact in fp32).  At these
        shapes (P <= 256 pixels) d = 1 + 6 + 1 + 4 = 12 for C = 40 and 1 + 5 + 1 + 4 = 11 for C = 64; the formula stays
        below 4 096 for every pyramid level under 2^21 pixels;
      * dw_l, dw_u against the formulas on the kernel's own sums, 1e-5 of max(|Sl|, |Su|) / s; exactly 0 where w <= 0;
      * two runs and a run on a second stream: identical bits."""
    lib = _lib()
    N = 2
    g = torch.Generator().manual_seed(100 * L + C)
    ins = [R.grid((N, H0 >> l, W0 >> l, C), g, H16) for l in range(L)]
    ws = _random_weights(mode, C, g, L - 1)
    f = Fused(cuda, ins, ws, act, mode)
    outs = f.run()
    douts_cpu = [R.grads(t.shape, g, H16) for t in ins]
    douts = [t.to(cuda) for t in douts_cpu]
    ks = [k.f64() for k in _coefs(ws)]
    side = torch.cuda.Stream(device=cuda)
    g_prev = coef_prev = g_prev_cpu = cu_prev = None
    for j in range(L):
        res = _bwd_level(cuda, lib, j, L, douts, g_prev, coef_prev, f, act, inplace=False)
        again = _bwd_level(cuda, lib, j, L, douts, g_prev, coef_prev, f, act, inplace=True)
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = _bwd_level(cuda, lib, j, L, douts, g_prev, coef_prev, f, act, inplace=False, stream=side)
        torch.cuda.synchronize()
        assert _same_bits(res, again), f"level {j}: in place differs from out of place"
        assert _same_bits(res, third), f"level {j}: the second stream differs"
        dout64 = R.f64(douts_cpu[j])
        if j == L - 1:
            ok, ratio, outside = R.check(res["din"].cpu(), FR.level_g(dout64, g_prev_cpu, cu_prev, None, None, H16), H16)
            print(f"top level din: worst ratio {ratio:.4f}")
            assert ok, (j, ratio, outside)
            break
        a_l, a_u, s, c_l, c_u = ks[j]
        ok, ratio, outside = R.check(res["g"].cpu(), FR.level_g(dout64, g_prev_cpu, cu_prev, R.f64(outs[j]), act, H16), H16)
        assert ok, ("g", j, ratio, outside)
        g64 = R.f64(res["g"].cpu())
        ok, ratio2, outside = R.check(res["din"].cpu(), FR.level_din(g64, c_l, H16), H16)
        assert ok, ("din", j, ratio2, outside)
        Sl, Su, Al, Au = FR.level_sums(g64, R.f64(ins[j]), R.f64(outs[j + 1]))
        d, _ = _reduction_depth(N * (H0 >> j) * (W0 >> j), C, False)
        assert d <= 4096
        got = res["sums"].cpu().double()
        worst = max(float(((got[0] - Sl).abs() / (d * 2.0 ** -24 * Al).clamp_min(1e-300)).max()),
                    float(((got[1] - Su).abs() / (d * 2.0 ** -24 * Au).clamp_min(1e-300)).max()))
        print(f"level {j} {mode} C={C}: g {ratio:.4f}, din {ratio2:.4f}, sums {worst:.4f} of the bound (d = {d})")
        assert bool(((got[0] - Sl).abs() <= d * 2.0 ** -24 * Al).all()) and \
            bool(((got[1] - Su).abs() <= d * 2.0 ** -24 * Au).all()), worst
        w_l, w_u = ws[j][0].double(), ws[j][1].double()
        want_l, want_u = FR.weight_grads(got[0], got[1], a_l, a_u, s, w_l, w_u)
        dw = res["dw"].cpu().double()
        St, Ut = (got[0].sum().reshape(1), got[1].sum().reshape(1)) if mode == "fast_attention" else (got[0], got[1])
        tol = 1e-5 * torch.maximum(St.abs(), Ut.abs()) / s
        assert bool(((dw[0] - want_l).abs() <= tol).all()) and bool(((dw[1] - want_u).abs() <= tol).all()), \
            (j, float(((dw[0] - want_l).abs() / tol.clamp_min(1e-300)).max()))
        assert bool((dw[0][w_l <= 0] == 0).all()) and bool((dw[1][w_u <= 0] == 0).all())
        g_prev, coef_prev, g_prev_cpu, cu_prev = res["g"], f.coef[j], g64, c_u.expand(C) if c_u.numel() == 1 else c_u
    assert float(ws[0][0][0]) < 0


@pytest.mark.parametrize("build", BUILDS)
def test_fused_backward_refuses_swish(cuda, build):
    """with `out` given the level would need swish' of a sum it does not have: RN_EINVAL before anything is launched, din
    and g keep their contents (the pattern of test_fpn_topdown_backward_refuses_swish)"""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(4)
    ins = [R.grid((1, 4 >> l, 8 >> l, 16), g, H16) for l in range(2)]
    f = Fused(cuda, ins, [_weights("fast_channel_attention", 16, FR.WEIGHT_PAIRS)], "swish", "fast_channel_attention")
    f.run()
    N, H, W, C = ins[0].shape
    dout = R.grads(ins[0].shape, g, H16).to(cuda)
    gbuf, din = torch.full_like(dout, 3.0), torch.full_like(dout, 3.0)
    nb = lib.rn_fpn_fused_bwd_workspace_bytes(N, H, W, C)
    ws = torch.zeros((nb,), dtype=torch.uint8, device=cuda)
    a = [_C.ptr(dout), None, None, _C.ptr(f.outs[0]), _C.ptr(f.ins[0]), _C.ptr(f.outs[1]), _C.ptr(f.coef[0]),
         _C.ptr(gbuf), _C.ptr(din), _C.ptr(ws), nb, N, H, W, C, _C.RN_ACT_SWISH, _C.current_stream()]
    assert lib.rn_fpn_fused_bwd_level(*a) == _C.RN_EINVAL
    assert b"swish" in lib.rn_last_error()
    torch.cuda.synchronize()
    assert bool((din == 3.0).all()) and bool((gbuf == 3.0).all())
    a[10] = nb - 1                                # a workspace one byte short
    a[15] = _C.RN_ACT_RELU
    assert lib.rn_fpn_fused_bwd_level(*a) == _C.RN_ENOMEM
    a[10], a[14] = nb, 12                         # C % 8
    assert lib.rn_fpn_fused_bwd_level(*a) == _C.RN_EINVAL
    a[14], a[12] = C, 3                           # a level that does not halve
    assert lib.rn_fpn_fused_bwd_level(*a) == _C.RN_EINVAL
    a[12], a[4] = H, None                         # a null tensor
    assert lib.rn_fpn_fused_bwd_level(*a) == _C.RN_EINVAL
    torch.cuda.synchronize()
    assert bool((din == 3.0).all()) and bool((gbuf == 3.0).all())


def test_train_engine_refuses_a_swish_fpn_in_the_weighted_modes(cuda):
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=128, activation="swish")
    p.architecture.batch_norm.use_sync = False
    p.architecture.feature_fusion.fusion_mode = "fast_attention"
    builder = ModelBuilder(p, "train", device=cuda)
    model = builder()
    with pytest.raises(NotImplementedError, match="top-down op fpn_td3 .* 'swish'"):
        TrainEngine(model, 2, frozen_regexes=[builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables])


def test_train_engine_refuses_live_fusion_weights_under_frozen_laterals(cuda):
    """fusion weights that train while a lateral conv of the FPN is frozen and nothing below it needs a gradient: the
    level's din has no buffer to go to — the engine says so when it is built"""
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=128)
    p.architecture.batch_norm.use_sync = False
    p.architecture.backbone.depth = 14
    p.architecture.feature_fusion.fusion_mode = "fast_channel_attention"
    model = ModelBuilder(p, "train", device=cuda)()
    everything_but = re.compile(r"^(?!.*-level-weight$)(?!((box-head)|(class-head)|(fpn/p\d-out)))")
    with pytest.raises(NotImplementedError, match="fusion weights .* frozen"):
        TrainEngine(model, 2, frozen_regexes=[everything_but])


# ---- 4. serving ------------------------------------------------------------------------------------------------------------
def _randomize(model, seed, fusion_seed):
    g = torch.Generator().manual_seed(seed)
    for k, v in model.variables.items():
        if k.endswith("/gamma"):
            v.copy_((torch.rand(v.shape, generator=g) * 0.5 + 0.75).to(v.device))
        elif k.endswith("/beta") or k.endswith("/moving_mean"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
        elif k.endswith("/moving_variance"):
            v.copy_((torch.rand(v.shape, generator=g) * 0.5 + 0.75).to(v.device))
    _randomize_fusion(model, fusion_seed)
    model._refresh()


def _randomize_fusion(model, seed):
    g = torch.Generator().manual_seed(seed)
    names = [k for k in model.variables if k.endswith("-level-weight")]
    assert len(names) == 8
    for i, k in enumerate(names):
        v = model.variables[k]
        w = torch.rand(v.shape, generator=g) * 2.3 - 0.3
        if i == 2:
            w[0] = -0.2
        v.copy_(w.to(v.device))
    assert any(float(model.variables[k].min()) < 0 for k in names)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("balanced", [False, True], ids=["plain", "balanced"])
def test_serving_with_weighted_fusion(cuda, tmp_path, mode, balanced):
    """ResNet-14, 128 x 128, B = 2, fusion weights in [-0.3, 2]: predictions against the CPU restatement with the weighted
    fpn() (max <= 0.08 scale + 1e-3, mean <= 0.01 scale + 1e-4); eager = graph replay bit for bit; after load_weights of
    other fusion weights the SAME captured graph gives what a fresh eager run gives; detections bit-equal to the oracle's
    post-processing of the same head outputs."""
    import oracle as o
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    size, B = 128, 2
    p = default_params(input_size=size, balanced=balanced)
    p.architecture.backbone.depth = 14
    p.architecture.feature_fusion.fusion_mode = mode
    p.inference.score_threshold = 0.005
    builder = ModelBuilder(p, "val", device=cuda)
    model = builder()
    _randomize(model, 3, 17)
    images = torch.randn((B, size, size, 3), generator=torch.Generator().manual_seed(1337))
    xd = images.to(cuda)
    eager, graphed = model.inference_engine(B), model.inference_engine(B, capture_graph=True)
    preds = {k: {lv: t.clone() for lv, t in d.items()} for k, d in eager(xd).items()}
    replay = {k: {lv: t.clone() for lv, t in d.items()} for k, d in graphed(xd).items()}
    torch.cuda.synchronize()
    ref = FR.FusedRefModel(p, model.variables, emulate_bf16=True)(images)
    for key in ("box-predictions", "class-predictions"):
        for lv in "34567":
            got, want = preds[key][lv].float().cpu(), ref[key][lv]
            scale, err = want.abs().max().item(), (got - want).abs()
            assert err.max().item() <= 0.08 * scale + 1e-3, (key, lv, err.max().item(), scale)
            assert err.mean().item() <= 0.01 * scale + 1e-4, (key, lv, err.mean().item(), scale)
            assert torch.equal(preds[key][lv], replay[key][lv]), (key, lv)
    # detections: the HIP post-processing of these head outputs against the oracle's
    infer = builder.add_post_processing_stage(model)
    det = {k: v.cpu().numpy().copy() for k, v in infer(xd).items()}
    logits = np.concatenate([preds["class-predictions"][l].cpu().numpy().reshape(B, -1, 80) for l in "34567"], 1)
    enc = np.concatenate([preds["box-predictions"][l].cpu().numpy().reshape(B, -1, 4) for l in "34567"], 1)
    an = o.generate_anchors(size, size, 3, 7, p.anchor_params.areas, p.anchor_params.aspect_ratios, p.anchor_params.scales)
    wb, ws, wc, wv = o.postprocess(logits, enc, an, size, size, score_threshold=0.005)
    np.testing.assert_array_equal(det["valid_detections"], wv)
    np.testing.assert_array_equal(det["classes"], wc)
    np.testing.assert_array_equal(det["scores"], ws)
    np.testing.assert_array_equal(det["boxes"], wb)
    # other fusion weights through save_weights / load_weights: in place, the captured graph is not captured again
    captured = graphed._graph
    assert captured is not None
    other = ModelBuilder(p, "val", device=cuda)()
    for k, v in model.variables.items():
        other.variables[k].copy_(v)
    _randomize_fusion(other, 29)
    prefix = str(tmp_path / "weights")
    other.save_weights(prefix)
    model.load_weights(prefix)
    names = [k for k in model.variables if k.endswith("-level-weight")]
    assert all(torch.equal(model.variables[k], other.variables[k]) for k in names)
    replay2 = {k: {lv: t.clone() for lv, t in d.items()} for k, d in graphed(xd).items()}
    assert graphed._graph is captured
    fresh = other.inference_engine(B)(xd)
    torch.cuda.synchronize()
    changed = False
    for key in ("box-predictions", "class-predictions"):
        for lv in "34567":
            assert torch.equal(replay2[key][lv], fresh[key][lv]), (key, lv)
            changed = changed or not torch.equal(replay2[key][lv], replay[key][lv])
    assert changed


# ---- 5. / 6. training ------------------------------------------------------------------------------------------------------
def _setup(cuda, mode, size, B, balanced, seed=3, depth=26, precision="mixed_bfloat16"):
    """the set-up of test_gpu_train_step.py::_setup (ResNet-26, small last-BN gammas, stem + block group 1 frozen) with a
    weighted fusion mode and random fusion weights"""
    from make_golden import synth_gt
    from retinanet.cfg import default_params
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=size, balanced=balanced, precision=precision)
    p.architecture.batch_norm.use_sync = False
    p.architecture.backbone.depth = depth
    p.architecture.feature_fusion.fusion_mode = mode
    builder = ModelBuilder(p, "train", device=cuda, seed=seed)
    model = builder()
    g = torch.Generator().manual_seed(seed)
    for k, v in model.variables.items():
        if k.endswith("/gamma"):
            zero_init = model.graph.bns[k[:-len("/gamma")]]["gamma_zero"]
            lo, span = (0.1, 0.2) if zero_init else (0.75, 0.5)
            v.copy_((torch.rand(v.shape, generator=g) * span + lo).to(cuda))
        elif k.endswith("/beta"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(cuda))
        elif "head" in k and k.endswith("/kernel"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.02).to(cuda))
        elif k.endswith("-level-weight"):
            v.copy_((torch.rand(v.shape, generator=g) * 1.5 + 0.5).to(cuda))
    eng = TrainEngine(model, B, frozen_regexes=[re.compile(r"^(conv2d|batch_normalization)(_[1-7])?/")])
    enc = LabelEncoder(p, device=cuda)
    rng = np.random.default_rng(seed)
    gts = [synth_gt(rng, int(rng.integers(2, 9)), size) for _ in range(B)]
    Gmax = max(x[0].shape[0] for x in gts)
    gb, gc, cnt = np.zeros([B, Gmax, 4], np.float32), np.zeros([B, Gmax], np.float32), np.zeros([B], np.int32)
    for i, (b, c) in enumerate(gts):
        gb[i, :len(b)], gc[i, :len(c)], cnt[i] = b, c, len(b)
    targets = enc.encode_batch(torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(cnt))
    images = torch.randn((B, size, size, 3), generator=g)
    return p, model, eng, targets, images


def _rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _engine_grad(eng, k):
    got = eng._pview(k, eng.G)
    if k.endswith("/kernel"):
        c = eng.g.convs[k[:-len("/kernel")]]
        got = got.reshape(c["cout"], c["k"], c["k"], c["cin"]).permute(1, 2, 3, 0)
    return got.cpu()


def _gradient_rows(grad_of, ref, names, join_scalars):
    """name -> (cosine, norm ratio) against ref's gradients; join_scalars: the eight one-element fusion weights as ONE
    8-vector (a cosine of scalars is a sign)"""
    rows, fused = {}, []
    for k in names:
        if k.endswith("/bias") and "prediction" not in k:
            continue   # bias in front of BatchNorm: analytically zero gradient, pure rounding noise
        want = ref.leaf[k].grad
        got = grad_of(k).reshape(want.shape)
        if join_scalars and k.endswith("-level-weight"):
            fused.append((got.reshape(-1), want.reshape(-1)))
            continue
        rows[k] = (_cos(got, want), got.double().norm().item() / (want.double().norm().item() + 1e-30))
    if fused:
        got, want = torch.cat([f[0] for f in fused]), torch.cat([f[1] for f in fused])
        assert got.numel() == 8
        rows["fusion-weights"] = (_cos(got, want), got.double().norm().item() / (want.double().norm().item() + 1e-30))
    return rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["mixed_bfloat16", "mixed_float16"])
def test_backward_wiring_with_weighted_fusion(cuda, mode, precision):
    """test_backward_wiring_dense_upstream's set-up and acceptance at (256, 4, balanced, frozen initial layers, auto) with
    a weighted FPN: forward error <= 1.3 x the float32-restatement floor + 0.005, every tensor's gradient cosine within
    0.06 of its floor, the median within 0.015, gradient norm ratios with median |r - 1| < 0.03 and maximum < 0.35, the
    two prediction kernels' cosines above 0.995 — the fusion weights among the rows (fast_attention: as one 8-vector)."""
    p, model, eng, targets, images = _setup(cuda, mode, 256, 4, True, precision=precision)
    assert eng.f16 == (precision == "mixed_float16")
    ref = FR.FusedRefTrainer(p, model.variables, frozen_names=eng.frozen, emulate_bf16=True)
    ref32 = FR.FusedRefTrainer(p, model.variables, frozen_names=eng.frozen, emulate_bf16=True, dtype=torch.float32)
    preds = eng.forward(images.to(cuda))
    g = torch.Generator().manual_seed(99)
    up = {k: {lv: torch.randn(preds[k][lv].shape, generator=g) for lv in preds[k]} for k in preds}
    eng.backward({k: {lv: t.to(cuda) for lv, t in d.items()} for k, d in up.items()})
    torch.cuda.synchronize()
    rp, rp32 = ref.forward_train(images), ref32.forward_train(images)
    floor_fwd = max(_rel(rp32[k][lv].detach(), rp[k][lv].detach()) for k in up for lv in up[k])
    got_fwd = max(_rel(preds[k][lv].float().cpu(), rp[k][lv].detach()) for k in up for lv in up[k])
    print(f"forward error {got_fwd:.4f}, floor {floor_fwd:.4f}")
    assert got_fwd <= 1.3 * floor_fwd + 0.005, (got_fwd, floor_fwd)
    sum((rp[k][lv] * up[k][lv].double()).sum() for k in up for lv in up[k]).backward()
    sum((rp32[k][lv] * up[k][lv]).sum() for k in up for lv in up[k]).backward()
    assert set(eng.train_names) == set(ref.leaf)
    fusion_names = [k for k in eng.train_names if k.endswith("-level-weight")]
    assert len(fusion_names) == 8
    join = mode == "fast_attention"
    rows = _gradient_rows(lambda k: _engine_grad(eng, k), ref, eng.train_names, join)
    floor = _gradient_rows(lambda k: ref32.leaf[k].grad, ref, eng.train_names, join)
    for k in rows:
        if "level-weight" in k or k == "fusion-weights":
            print(f"{k[-48:]}: cosine {rows[k][0]:.4f} (floor {floor[k][0]:.4f}), norm ratio {rows[k][1]:.4f}")
    assert ("fusion-weights" in rows) == join and (join or all(k in rows for k in fusion_names))
    worst = sorted((rows[k][0] - floor[k][0], k, rows[k][0], floor[k][0]) for k in rows)
    assert worst[0][0] > -0.06, worst[:5]
    med, med_floor = np.median([r[0] for r in rows.values()]), np.median([r[0] for r in floor.values()])
    assert med > med_floor - 0.015, (med, med_floor)
    # the magnitudes, as test_backward_wiring_dense_upstream judges them: a wrong constant factor in the wiring (another
    # fusion's coefficient block, a missed 1 / s) leaves every cosine alone and shows here
    ratios = np.array([r[1] for r in rows.values()])
    print(f"norm ratios: median |r - 1| {np.median(np.abs(ratios - 1)):.4f}, range {ratios.min():.4f} .. {ratios.max():.4f}")
    assert np.median(np.abs(ratios - 1)) < 0.03 and np.abs(ratios - 1).max() < 0.35, (ratios.min(), ratios.max())
    # the layers next to the loss see almost no accumulated rounding noise
    assert rows["class-head/class-head-prediction-conv2d/kernel"][0] > 0.995
    assert rows["box-head/box-head-prediction-conv2d/kernel"][0] > 0.995


@pytest.mark.parametrize("mode", MODES)
def test_train_step_moves_and_decays_the_fusion_weights(cuda, tmp_path, mode):
    """One train_step with weight decay on.  Losses and the l2 term against FusedRefTrainer.step / weight_decay (the l2
    term counts the fusion weights: without them it is off by alpha * sum(w^2) / 2 of eight weights, which the test
    checks to be more than ten times the tolerance — the test fails if they are left out of the decay set).  The optimizer
    stages replayed in float64 from the engine's own raw gradients, as test_train_step_losses_and_optimizer_arithmetic
    does, with the decay term on kernels AND fusion weights: V, P, E of every fusion weight.  A checkpoint written after
    the step restores them bit for bit."""
    p, model, eng, targets, images = _setup(cuda, mode, 256, 4, True)
    assert p.training.use_weight_decay
    ref = FR.FusedRefTrainer(p, model.variables, frozen_names=eng.frozen, emulate_bf16=True)
    opt = model.optimizer
    lr, dec, mom, clip = opt.lr(0), opt.ema_decay(0), opt.momentum, float(opt.clipnorm)
    alpha = p.training.weight_decay_alpha
    fusion = [k for k in eng.train_names if k.endswith("-level-weight")]
    assert len(fusion) == 8 and all(eng.var_kind[k][0] == "fusion" for k in fusion)
    xd = images.to(cuda)
    w0 = eng.P.clone()
    # the raw gradients of this very step: every kernel is deterministic, train_step recomputes the same ones
    preds = eng.forward(xd)
    model.loss(targets, preds, compute_grads=True, grad_scale=1.0)
    eng.backward(model.loss.grads)
    raw = eng.G.clone()
    out = eng.train_step(xd, targets)
    torch.cuda.synchronize()
    want = ref.step(images, targets["_flat"]["class-targets"].cpu().numpy(), targets["_flat"]["box-targets"].cpu().numpy(),
                    float(targets["num-positives"].sum().item()), lr)
    for k in ("box-loss", "class-loss", "weighted-loss"):
        assert out[k].item() == pytest.approx(want["losses"][k], rel=0.03), k
    l2 = float(ref.weight_decay().detach())
    l2_without = l2 - sum(alpha * 0.5 * float((ref.leaf[k].detach() ** 2).sum()) for k in fusion)
    print(f"l2-regularization {out['l2-regularization'].item():.8f}, reference {l2:.8f}, without fusion weights {l2_without:.8f}")
    assert out["l2-regularization"].item() == pytest.approx(l2, rel=1e-5)
    assert abs(l2 - l2_without) > 10 * 1e-5 * l2, "the fusion weights' share is too small for this check to see"
    parts = {}
    for k in eng.train_names:
        off, n = eng.p_off[k]
        gk = raw[off:off + n].double().cpu()
        if k.endswith("/kernel") or k.endswith("-level-weight"):
            gk = gk + alpha * w0[off:off + n].double().cpu()
        parts[k] = gk * (clip / max(gk.norm().item(), clip))
    gn = float(np.sqrt(sum(v.norm().item() ** 2 for v in parts.values())))
    F = clip / max(gn, clip)
    assert eng.metrics[1].item() == pytest.approx(gn, rel=1e-4)
    assert eng.metrics[0].item() == pytest.approx(gn * F, rel=1e-4)
    for k in fusion + eng.train_names[::23]:
        off, n = eng.p_off[k]
        w0k = w0[off:off + n].double().cpu()
        v1 = -lr * parts[k] * F
        w1 = w0k + v1
        e1 = w0k * dec + (1 - dec) * w1
        torch.testing.assert_close(eng.V[off:off + n].double().cpu(), v1, rtol=1e-4, atol=1e-7)
        torch.testing.assert_close(eng.P[off:off + n].double().cpu(), w1, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(eng.E[off:off + n].double().cpu(), e1, rtol=1e-5, atol=1e-6)
    for k in fusion:
        off, n = eng.p_off[k]
        assert not torch.equal(eng.P[off:off + n], w0[off:off + n]), k        # they move
        assert float(raw[off:off + n].abs().max()) > 0, k
    # checkpoint: weights, momentum and moving average of the fusion weights come back bit for bit
    prefix = str(tmp_path / "weights_step_1")
    eng.save_checkpoint(prefix)
    _, model2, eng2, _, _ = _setup(cuda, mode, 256, 4, True)
    for k in fusion:
        assert not torch.equal(eng2._pview(k), eng._pview(k))
    eng2.restore_checkpoint(prefix)
    assert eng2.step_count == 1
    for k in fusion:
        for arena in ("P", "V", "E"):
            assert torch.equal(eng2._pview(k, getattr(eng2, arena)), eng._pview(k, getattr(eng, arena))), (k, arena)
        assert torch.equal(model2.variables[k].reshape(-1), eng._pview(k))


def test_gradient_joins_match_the_graph(cuda):
    """Build only.  The fast_attention engine at batch 2: the planner's record of who writes every activation-gradient
    buffer (engine.joins.writers) against the count of readers taken from the graph alone (join_counts.py).  The weighted
    top-down backward overwrites din of every level below the top, so it must be the first writer of each; the top level
    passes through, its gradient is updated in place behind the output conv's data gradient."""
    from join_counts import check_joins
    p, model, eng, targets, images = _setup(cuda, "fast_attention", 256, 2, True)
    check_joins(eng)
    top = next(o for o in eng.ops if o["op"] == "topdown")
    assert top.get("fusion") and id(top) in eng.fusion_state and top["ins"][-1] == top["outs"][-1]
    writers = eng.joins.writers
    assert all(writers[n][0] == "topdown" and "topdown" not in writers[n][1:] for n in top["ins"][:-1])
    assert writers[top["ins"][-1]][0].startswith("dgrad:") and writers[top["ins"][-1]][1:] == ["topdown"], writers[top["ins"][-1]]
