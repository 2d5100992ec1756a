"""Every forward site of an activation and every gradient gate of the library against float64 (act_ref.py), on EVERY
input a 16-bit tensor can hold: `A.sweep()` — all finite values of the storage type, one [1024, 64] tensor — is fed
through each kernel arranged so that the value in front of the activation is exactly the input (BatchNorm with mean 0 /
invstd 1 / scale 1 / shift 0 written by hand, identity convolution weights, a zero coarse pyramid level).

Acceptance (derivation in act_ref.py): every element
    |got - ref| <= ulp_s(ref) / 2 + slack,   slack = 2^-16 |ref| + 1e-30 (swish value), 2^-20 (swish derivative)
ref the UNROUNDED float64 value; relu / relu6 / none and their 0 / 1 gates bit for bit (zeros by value); below the
smallest normal storage value the rounded reference or a zero.  Inputs below -88.7 (bfloat16 only): 1 + e^-x overflows
fp32 and the kernels return -0 where the value is about -2e-37; the 1e-30 floor accepts that.  Every check prints its
worst |got - ref| / bound and the input it occurs at before it asserts.

Forward sites: rn_bn_apply (all four activations, with and without a zero residual, with the gate bit mask),
rn_depthwise_conv2d_nhwc_fwd (k = 1, weight 1), rn_conv2d_nhwc_fwd with identity weights on each of its kernels (128-row
tiles of 64 and 128 columns, conv_big, conv_halo 256 x 256 and 512 x 128 — the kernel id is asserted), rn_fpn_topdown.
Gates: rn_bn_bwd_reduce + rn_bn_bwd_apply with dz = 1, so that dres = rs(act'(.)) per element, in every gate mode
bn_gate_mode() can return (none, relu / relu6 from u, from z, from the bit mask, swish, swish behind a residual add,
and the generic mode of a problem whose segments disagree on having a residual); then the sums (bsums, dgamma, dbeta)
and dy / dres on small shapes with random gradients for act x residual x dres_accumulate.  rn_act_bwd and
rn_fpn_topdown_bwd_level cannot compute swish' from their arguments: they must refuse, and so must TrainEngine."""
import ctypes

import pytest
import torch

import act_ref as A
import pyramid_ref as R

pytestmark = pytest.mark.gpu

H16 = torch.bfloat16
_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BUILDS = ["bf16", "f16"]
ACTS = ["none", "relu", "relu6", "swish"]
P0 = (1 << 16) // A.C        # rows of the sweep tensor


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


def _rs(v):
    """float64 -> storage (one rounding), as float64; an overflow cannot happen in these tests"""
    r = R.round_storage(v, H16)
    assert bool(torch.isfinite(r).all())
    return r


def _within(got, ref, slack, x, what):
    """print the figure and the input it occurs at, then assert the rule on every element"""
    ok, ratio, outside, worst = A.check(got.cpu(), ref, H16, slack)
    at = x.reshape(-1)[worst].item()
    print(f"{what} [{'f16' if H16 == torch.float16 else 'bf16'}]: worst |got - ref| / bound = {ratio:.4f} at input {at!r}, "
          f"{outside} of {got.numel()} outside")
    assert ok, (what, "worst ratio", ratio, "at input", at, "got", got.cpu().reshape(-1)[worst].item(), "ref",
                ref.reshape(-1)[worst].item(), "elements outside", outside)


def _check_value(got, pre, act, what):
    """got: stored act(pre); pre: the float64 value in front of the activation (a storage value)"""
    if act == "swish":
        ref = A.act_fwd(pre, act)
        _within(got, ref, A.value_slack(ref, act), pre, what)
    else:
        want = A.act_fwd(pre, act).to(H16)
        assert A.same_values(got.cpu(), want), (what, int((got.cpu().float() != want.float()).sum()))


# ---- BatchNorm problems on given tensors ---------------------------------------------------------------------------------
def _identity_fwd(C, cuda):
    """rn_bn_segment.fwd = [mean 0 | invstd 1 | scale 1 | shift 0]: u = y exactly"""
    return torch.tensor([0.0, 1.0, 1.0, 0.0], device=cuda).repeat_interleave(C).reshape(4, C).contiguous()


def _bn_problem(cuda, act, segs):
    """segs: dicts with y [P, C] and fwd [4, C] (device), optional residual, dz, dres0 (initial dres), mask (bool: attach a
    bit mask), accumulate.  Returns (problem, per-segment tensors, workspace)."""
    from retinanet import _C
    p = _C.BnProblem()
    p.num_segments, p.act, p.bessel, p.eps, p.momentum, p.count_scale = len(segs), _C.ACT_IDS[act], 1, 1e-3, 0.99, 1.0
    T = []
    for i, s in enumerate(segs):
        P, C = s["y"].shape
        t = {"y": s["y"].to(cuda).contiguous(), "fwd": s["fwd"].to(cuda).float().contiguous()}
        t["z"] = torch.full_like(t["y"], 7.0)
        t["dy"] = torch.full_like(t["y"], 7.0)
        for k in ("residual", "dz"):
            t[k] = None if s.get(k) is None else s[k].to(cuda).contiguous()
        t["dres"] = torch.full_like(t["y"], 7.0) if s.get("dres0") is None else s["dres0"].to(cuda).clone()
        t["mask"] = torch.full((P * C // 8,), 0xA5, dtype=torch.uint8, device=cuda) if s.get("mask") else None
        t["bsums"] = torch.zeros((2, C), dtype=torch.float32, device=cuda)
        t["dgamma"], t["dbeta"] = torch.zeros((C,), device=cuda), torch.zeros((C,), device=cuda)
        d = p.seg[i]
        d.y, d.z, d.dy, d.dres, d.fwd, d.bsums = (t["y"].data_ptr(), t["z"].data_ptr(), t["dy"].data_ptr(),
                                                  t["dres"].data_ptr(), t["fwd"].data_ptr(), t["bsums"].data_ptr())
        d.residual = None if t["residual"] is None else t["residual"].data_ptr()
        d.dz = None if t["dz"] is None else t["dz"].data_ptr()
        d.act_mask = None if t["mask"] is None else t["mask"].data_ptr()
        d.dgamma, d.dbeta = t["dgamma"].data_ptr(), t["dbeta"].data_ptr()
        d.P, d.C, d.dres_accumulate = P, C, int(bool(s.get("accumulate")))
        T.append(t)
    ws = torch.zeros((max(int(_lib().rn_bn_workspace_bytes(ctypes.byref(p))), 256),), dtype=torch.uint8, device=cuda)
    return p, T, ws


def _bn_forward(p):
    from retinanet import _C
    _C.check(_lib().rn_bn_apply(ctypes.byref(p), _C.current_stream()), "rn_bn_apply")
    torch.cuda.synchronize()


def _bn_backward(p, ws):
    from retinanet import _C
    st = _C.current_stream()
    _C.check(_lib().rn_bn_bwd_reduce(ctypes.byref(p), _C.ptr(ws), ws.numel(), st), "rn_bn_bwd_reduce")
    _C.check(_lib().rn_bn_bwd_apply(ctypes.byref(p), st), "rn_bn_bwd_apply")
    torch.cuda.synchronize()


def _mask_bits(mask, shape):
    return ((mask.cpu().view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).reshape(shape)


# ---- forward sweeps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("act", ACTS)
def test_bn_apply_on_every_input(cuda, build, act, residual):
    """z = act(rs(rs(y) + 0)) = act(y); with rn_bn_segment.act_mask the bits are act'(stored z) != 0 (0xff: swish, none)"""
    x = A.sweep(H16)
    seg = {"y": x, "fwd": _identity_fwd(A.C, cuda), "mask": True,
           "residual": torch.zeros_like(x) if residual else None}
    p, T, _ = _bn_problem(cuda, act, [seg])
    _bn_forward(p)
    z = T[0]["z"].cpu()
    _check_value(z, R.f64(x), act, f"rn_bn_apply {act} residual={residual}")
    bits = _mask_bits(T[0]["mask"], z.shape)
    want = torch.ones_like(bits) if act in ("swish", "none") else (A.act_deriv(R.f64(z), act) != 0).to(torch.uint8)
    assert torch.equal(bits, want), (act, int((bits != want).sum()))
    if act in ("relu", "relu6"):
        assert 0 < int(want.sum()) < want.numel()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("act", ["swish", "relu"])
def test_depthwise_conv_on_every_input(cuda, build, act):
    """k = 1, weight 1, scale 1, shift 0: the DepthwiseConv2D output and the BatchNorm output are the input itself"""
    from retinanet import _C
    lib = _lib()
    x = A.sweep(H16)
    N, H, W, C = 1, 32, P0 // 32, A.C
    xd = x.to(cuda)
    wf = torch.ones((1, 1, C, 1), device=cuda)
    wd = torch.empty((1, C), dtype=H16, device=cuda)
    st = _C.current_stream()
    _C.check(lib.rn_pack_depthwise_weight(_C.ptr(wf), 1, C, _C.ptr(wd), st), "pack")
    y = torch.full((P0, C), 7.0, dtype=H16, device=cuda)
    sc, sh = torch.ones((C,), device=cuda), torch.zeros((C,), device=cuda)
    p = _C.DwProblem()
    p.k, p.stride, p.pad_top, p.pad_left, p.act, p.num_segments = 1, 1, 0, 0, _C.ACT_IDS[act], 1
    sg = p.seg[0]
    sg.x, sg.w, sg.y, sg.scale, sg.shift = xd.data_ptr(), wd.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr()
    sg.N, sg.H, sg.W, sg.C, sg.Ho, sg.Wo = N, H, W, C, H, W
    _C.check(lib.rn_depthwise_conv2d_nhwc_fwd(ctypes.byref(p), st), "dw")
    torch.cuda.synchronize()
    _check_value(y.cpu(), R.f64(x), act, f"rn_depthwise_conv2d_nhwc_fwd {act}")


CONV_SWEEPS = [
    # k, channels, rn_launch_opts, kernel id (rn_conv_kernel_id), tile rows
    (1, 64, {}, 0, 128),                                   # conv_fwd_kernel, 64-column tiles
    (3, 64, {}, 0, 128),
    (1, 256, {"conv_tile": 1}, 0, 128),                    # conv_fwd_kernel, 128-column tiles
    (3, 64, {"conv_tile": 3}, 3, 512),                     # conv_halo_kernel, 512 x 128 tiles
    (1, 256, {"conv_tile": 2}, 1, 256),                    # conv_big_kernel
    (3, 256, {"conv_tile": 2}, 2, 256),                    # conv_halo_kernel, 256 x 256 tiles
    (3, 256, {"conv_tile": 2, "conv_no_halo": 1}, 1, 256),
]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("k,C,opts,kid,rows", CONV_SWEEPS, ids=[f"k{c[0]}-c{c[1]}-kernel{c[3]}-{i}" for i, c in enumerate(CONV_SWEEPS)])
def test_conv_swish_epilogue_on_every_input(cuda, build, k, C, opts, kid, rows):
    """identity weights (a 1x1 conv, or a 3x3 whose centre tap is the identity): the accumulator is the input, exactly —
    every other product is a finite value times 0.  An MFMA may flush subnormal inputs: the rule accepts a zero there."""
    from retinanet import _C
    lib = _lib()
    x = A.sweep(H16).reshape(-1, C)
    P = x.shape[0]
    H = 32 if P == 1024 else 16
    N, W = 1, P // H
    w = torch.zeros((k, k, C, C))
    w[k // 2, k // 2] = torch.eye(C)
    wf = w.to(cuda).contiguous()
    cinp = lib.rn_conv_cin_pad(C)
    wp = torch.empty((lib.rn_conv_cout_pad(C), k, k, cinp), dtype=H16, device=cuda)
    st = _C.current_stream()
    _C.check(lib.rn_pack_conv_weight(_C.ptr(wf), k, k, C, C, cinp, _C.ptr(wp), st), "pack")
    xd = x.to(cuda).contiguous()
    y = torch.full((P, C), 7.0, dtype=H16, device=cuda)
    p = _C.ConvProblem()
    p.opts = _C.LaunchOpts(**opts)
    p.R = p.S = k
    p.stride_h = p.stride_w = 1
    p.pad_top = p.pad_left = k // 2
    p.act, p.out_dtype, p.num_segments = _C.RN_ACT_SWISH, _C.RN_DT_BF16, 1
    sg = p.seg[0]
    sg.x, sg.w, sg.y = xd.data_ptr(), wp.data_ptr(), y.data_ptr()
    sg.N, sg.H, sg.W, sg.Cin, sg.pix_stride, sg.Ho, sg.Wo, sg.Cout = N, H, W, C, C, H, W, C
    assert lib.rn_conv_kernel_id(ctypes.byref(p)) == kid and lib.rn_conv_tile_rows(ctypes.byref(p)) == rows
    _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), st), "conv")
    torch.cuda.synchronize()
    # a flushed subnormal INPUT gives swish(0) = 0 where the value is about x / 2: below the smallest normal as well
    _check_value(y.cpu(), R.f64(x), "swish", f"rn_conv2d_nhwc_fwd k={k} C={C} kernel {kid}")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("act", ACTS)
def test_fpn_topdown_on_every_input(cuda, build, act):
    """two levels, the coarse one all zeros: out[0] = act(rs(in[0] + 0))"""
    from retinanet import _C
    x = A.sweep(H16)
    N, H, W, C = 1, 32, P0 // 32, A.C
    ins = [x.reshape(N, H, W, C).to(cuda), torch.zeros((N, H // 2, W // 2, C), dtype=H16, device=cuda)]
    outs = [torch.full_like(ins[0], 7.0), ins[1]]
    _C.check(_lib().rn_fpn_topdown(_C.ptr_array(ins), _C.ptr_array(outs), 2, N, H, W, C, _C.ACT_IDS[act],
                                   _C.current_stream()))
    torch.cuda.synchronize()
    _check_value(outs[0].cpu().reshape(P0, C), R.f64(x), act, f"rn_fpn_topdown {act}")


# ---- gate sweeps ---------------------------------------------------------------------------------------------------------
def _const(x, v):
    t = torch.full_like(x, v)
    assert t.float()[0, 0].item() == v, "the residual is a storage value"
    return t


# (id, act, per segment: None = no residual, else the constant residual; bit mask)
GATE_MODES = [
    ("G_NONE", "none", [None], False),
    ("G_NONE-residual", "none", [0.5], False),
    ("G_U_RELU", "relu", [None], False),
    ("G_U_RELU6", "relu6", [None], False),
    ("G_Z_RELU", "relu", [0.5], False),
    ("G_Z_RELU-minus3", "relu", [-3.0], False),
    ("G_Z_RELU6", "relu6", [0.5], False),
    ("G_Z_RELU6-minus3", "relu6", [-3.0], False),
    ("G_MASK-relu", "relu", [0.5], True),
    ("G_MASK-relu6", "relu6", [-3.0], True),
    ("G_SWISH", "swish", [None], False),
    ("G_SWISH_RES", "swish", [0.5], False),
    ("G_SWISH_RES-minus3", "swish", [-3.0], False),
    ("G_SWISH_RES-two-segments", "swish", [0.5, -3.0], False),
    ("G_GENERIC-relu", "relu", [0.5, None], False),
    ("G_GENERIC-relu6", "relu6", [None, -3.0], False),
    ("G_GENERIC-swish", "swish", [0.5, None], False),
    ("G_GENERIC-swish-minus3", "swish", [None, -3.0], False),
]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode,act,residuals,masked", GATE_MODES, ids=[m[0] for m in GATE_MODES])
def test_bn_backward_gate_on_every_input(cuda, build, mode, act, residuals, masked):
    """dz = 1, dres_accumulate = 0: dres = rs(act'(.)), no sum touches it.  The gate is taken at v = rs(rs(y) + residual)
    for swish — the value rn_bn_apply fed to swish — and on the stored z for relu / relu6 (z itself is pinned against
    rs(act(y + residual)) first).  dy, bsums, dgamma, dbeta are not asserted here: sums over every value of the type."""
    x = A.sweep(H16)
    segs = [{"y": x, "fwd": _identity_fwd(A.C, cuda), "dz": torch.ones_like(x), "mask": masked,
             "residual": None if r is None else _const(x, r)} for r in residuals]
    p, T, ws = _bn_problem(cuda, act, segs)
    _bn_forward(p)
    zs = [t["z"].cpu() for t in T]
    if masked:
        for t in T:
            t["z"].fill_(float("nan"))          # with the bit mask the backward passes must not look at z
    _bn_backward(p, ws)
    for i, (r, t, z) in enumerate(zip(residuals, T, zs)):
        what = f"{mode} segment {i} residual {r}"
        pre = R.f64(x) if r is None else R.f64(x) + r
        got = t["dres"].cpu()
        if act == "swish":
            v = _rs(pre)
            ref = A.act_deriv(v, act)
            _within(got, ref, A.deriv_slack(ref, act), x, f"bn backward gate {what}")
        else:
            want_z = _rs(A.act_fwd(pre, act)).to(H16)
            assert A.same_values(z, want_z), (what, "z")
            want = A.act_deriv(R.f64(want_z), act).to(H16)
            assert A.same_values(got, want), (what, int((got.float() != want.float()).sum()))
            if act != "none":
                assert 0 < int(want.float().sum()) < want.numel()


# ---- the sums, dy and dres on small shapes ------------------------------------------------------------------------------
MATRIX_SHAPES = [(2, 9, 7, 64), (1, 5, 5, 256), (3, 4, 4, 8), (1, 6, 6, 144)]     # 144 channels: the slabs that are not 64 wide
_HAS_RES = {"no": (False,) * 4, "yes": (True,) * 4, "mixed": (True, False, True, False)}


def _matrix_inputs(residual):
    """Built once per (storage type, residual pattern) and never modified.  y, residual: multiples of 1/4 in [-2, 2];
    scale: a multiple of 1/2 in [-2, 2] without 0; shift: a multiple of 1/8 in [-1, 1] — so u = y*scale + shift and
    u + residual are multiples of 1/8 below 8, exact in fp32 and in both storage types: the value in front of the
    activation is the same number in the kernel and in the reference, and the only inexact step of the gate is swish'."""
    key = (H16, residual)
    if key not in _matrix_inputs.cache:
        g = torch.Generator().manual_seed(1234 + len(residual))
        segs = []
        for (N, H, W, C), has in zip(MATRIX_SHAPES, _HAS_RES[residual]):
            P = N * H * W
            sc = torch.randint(1, 5, (C,), generator=g).float() / 2 * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
            sh = torch.randint(-8, 9, (C,), generator=g).float() / 8
            fwd = torch.stack([torch.randn((C,), generator=g) * 0.5, torch.rand((C,), generator=g) + 0.5, sc, sh])
            segs.append({"y": R.grid((P, C), g, H16), "fwd": fwd, "dz": R.grads((P, C), g, H16),
                         "residual": R.grid((P, C), g, H16) if has else None, "dres0": R.grads((P, C), g, H16)})
        _matrix_inputs.cache[key] = segs
    return _matrix_inputs.cache[key]


_matrix_inputs.cache = {}


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("residual", ["no", "yes", "mixed"])
@pytest.mark.parametrize("act", ACTS)
def test_bn_backward_sums_and_gradients(cuda, build, act, residual, accumulate):
    """g = dz * act'(.) with the gate of the header (relu / relu6: from the stored z; swish: at rs(rs(u) + residual), or
    at u without a residual — the same number here, see _matrix_inputs).
      bsums[0] = dbeta = sum g, bsums[1] = dgamma = sum g xhat: fp32 outputs, |got - ref| <= n 2^-23 sum|terms| with
        n = rows + 4 (the sum, and the <= 4 roundings of a term: xhat is two operations), plus 2^-20 per term times the
        term's other factors for the swish gate (act_ref.DERIV_SLACK);
      dy = rs(scale (g - bsums[0]/n - xhat bsums[1]/n)) with the kernel's own bsums, dres = rs(g [+ dres]): per element
        by pyramid_ref.check, 8 and 2 fp32 operations, the swish slack scaled by |scale dz| and |dz|."""
    segs = [dict(s, accumulate=accumulate) for s in _matrix_inputs(residual)]
    p, T, ws = _bn_problem(cuda, act, segs)
    _bn_forward(p)
    _bn_backward(p, ws)
    gslack = A.DERIV_SLACK if act == "swish" else 0.0
    missed = []          # every output that misses its bound, so that one failure shows all of them (sums, dy and dres)
    for i, (s, t) in enumerate(zip(segs, T)):
        what = f"{act} residual={residual} accumulate={accumulate} segment {i}"
        y, dz, fwd = R.f64(s["y"]), R.f64(s["dz"]), s["fwd"].to(R.F64)
        n = y.shape[0]
        u = y * fwd[2] + fwd[3]
        pre = u if s["residual"] is None else _rs(u) + R.f64(s["residual"])
        assert torch.equal(_rs(pre), pre) and torch.equal(pre.float().to(R.F64), pre), "exact in front of the activation"
        z = t["z"].cpu()
        _check_value(z, pre, act, f"z {what}")
        gate = A.act_deriv(pre, act) if act == "swish" else A.act_deriv(R.f64(z), act)
        g = dz * gate
        xhat = (y - fwd[0]) * fwd[1]
        bs = t["bsums"].cpu().to(R.F64)
        for j, (name, term, other) in enumerate((("bsums[0]", g, dz), ("bsums[1]", g * xhat, dz * xhat))):
            ref = term.sum(0)
            bound = (n + 4) * 2.0 ** -23 * term.abs().sum(0) + gslack * other.abs().sum(0)
            err = (bs[j] - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            print(f"{name} {what}: worst error / bound = {ratio:.4f}")
            if not bool((err <= bound).all()):
                missed.append((name, what, "worst error / bound", ratio, "worst error", float(err.max()),
                               "sum there", float(ref[err.argmax()])))
        assert torch.equal(t["dbeta"].cpu(), t["bsums"][0].cpu()) and torch.equal(t["dgamma"].cpu(), t["bsums"][1].cpu())
        # dy from the kernel's own fp32 sums (their accuracy is asserted above)
        inv_n = float(torch.tensor(1.0 / n, dtype=torch.float32))
        k1, k2 = bs[0] * inv_n, bs[1] * inv_n
        want = fwd[2] * (g - k1 - xhat * k2)
        ref = R.Ref(_rs(want), fwd[2].abs() * (g.abs() + k1.abs() + (xhat * k2).abs()), 8, fwd[2].abs() * dz.abs() * gslack)
        ok, ratio, outside = R.check(t["dy"].cpu(), ref, H16)
        print(f"dy {what}: worst |got - ref| / bound = {ratio:.4f}, {outside} of {want.numel()} outside")
        if not ok:
            missed.append(("dy", what, "worst ratio", ratio, "elements outside", outside))
        old = R.f64(s["dres0"]) if accumulate else torch.zeros_like(g)
        ref = R.Ref(_rs(g + old), g.abs() + old.abs(), 2, dz.abs() * gslack)
        ok, ratio, outside = R.check(t["dres"].cpu(), ref, H16)
        print(f"dres {what}: worst |got - ref| / bound = {ratio:.4f}, {outside} of {want.numel()} outside")
        if not ok:
            missed.append(("dres", what, "worst ratio", ratio, "elements outside", outside))
    assert not missed, missed


# ---- what cannot be computed is refused ---------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_act_bwd_refuses_swish(cuda, build):
    """swish' is no function of z: RN_EINVAL before any launch, dy keeps its contents"""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(3)
    z, dz = R.grid((64,), g, H16).to(cuda), R.grads((64,), g, H16).to(cuda)
    dy = torch.full_like(dz, 3.0)
    assert lib.rn_act_bwd(_C.ptr(dz), _C.ptr(z), _C.ptr(dy), 64, _C.RN_ACT_SWISH, _C.current_stream()) == _C.RN_EINVAL
    assert b"swish" in lib.rn_last_error()
    torch.cuda.synchronize()
    assert bool((dy == 3.0).all())
    _C.check(lib.rn_act_bwd(_C.ptr(dz), _C.ptr(z), _C.ptr(dy), 64, _C.RN_ACT_RELU, _C.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(dy.cpu(), dz.cpu() * R.act_mask(z.cpu().float(), "relu").to(H16))


@pytest.mark.parametrize("build", BUILDS)
def test_fpn_topdown_backward_refuses_swish(cuda, build):
    """with `out` given the level would need swish' of a sum it does not have: RN_EINVAL, din keeps its contents;
    without `out` there is no gate and act is not looked at"""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(4)
    N, H, W, C = 1, 4, 6, 16
    dout, out = R.grads((N, H, W, C), g, H16).to(cuda), R.grid((N, H, W, C), g, H16).to(cuda)
    din = torch.full_like(dout, 3.0)
    a = (_C.ptr(dout), None, _C.ptr(out), _C.ptr(din), N, H, W, C, _C.RN_ACT_SWISH, _C.current_stream())
    assert lib.rn_fpn_topdown_bwd_level(*a) == _C.RN_EINVAL
    assert b"swish" in lib.rn_last_error()
    torch.cuda.synchronize()
    assert bool((din == 3.0).all())
    a = (_C.ptr(dout), None, None, _C.ptr(din), N, H, W, C, _C.RN_ACT_SWISH, _C.current_stream())
    _C.check(lib.rn_fpn_topdown_bwd_level(*a))
    torch.cuda.synchronize()
    assert torch.equal(din.cpu().view(torch.int16), dout.cpu().view(torch.int16))


def test_train_engine_refuses_a_swish_fpn(cuda):
    """architecture.activation.type = 'swish' reaches the FPN's top-down op: the engine must say so when it plans the
    backward pass, not train with a gate of 1"""
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=128, activation="swish")
    p.architecture.batch_norm.use_sync = False
    builder = ModelBuilder(p, "train", device=cuda)
    model = builder()
    assert any(op["op"] == "topdown" and op["act"] == "swish" for op in model.graph.ops)
    with pytest.raises(NotImplementedError, match="top-down op fpn_td3 .* 'swish'"):
        TrainEngine(model, 2, frozen_regexes=[builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables])
