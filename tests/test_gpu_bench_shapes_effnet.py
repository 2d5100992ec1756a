"""Per-launch parity AT THE BENCH'S EXACT SHAPES for the EfficientNet-B3 path (BASELINE configs[4], bench.py `extra.config4`).

tests/test_gpu_bench_shapes.py / _more.py pin the ResNet engine launch by launch.  Here the same is done for the configs[4]
training engine — EfficientNet-B3 at 640 x 640, 32 images, `mixed_float16`, so every launch goes to librnet_hip_f16.so —
and its serving engine (batch 8): every DISTINCT launch of
  (a) the implicit-GEMM convs (forward / data gradient / weight gradient: the channel-padded 1 x 1 layers of 24 / 40 input
      channels, the separable pointwise convs, the grouped head levels, the BatchNorm partial sums of their epilogues),
  (b) the depthwise convs (forward, stride-2 data gradients through rn_upsample_zero2x and the tap-reversed filter, the
      accumulating `residual` form, multi-segment head launches, grids that run their grid-stride loop more than once;
      the weight gradient),
  (c) the squeeze-excite forward / backward (the slab plans of the pooling kernels are picked from the batch's chunk count:
      the forms of 32 images exist at no smaller batch),
  (d) the BatchNorm passes (swish groups, the stochastic-depth `sample_scale` groups; slab plans again from the batch),
  (e) the serving engine's depthwise (folded BatchNorm + swish epilogue) and in-place squeeze-excite launches
is re-issued through the C ABI on fresh seeded tensors of the launch's own geometry and compared with a float64 evaluation
on the GPU through torch (an independent code path) that rounds to the storage type where include/rnet_hip.h says a 16-bit
tensor exists.

Tolerances are stated in steps of the storage type: u = 2^-8 (bfloat16) or 2^-11 (IEEE half) relative.  Where the kernel
and the reference share every rounding point, a stored element may sit one step (2u of its value) off where an fp32 sum
straddles a rounding boundary, on a small fraction of the elements; f32 outputs (weight gradients, parameter gradients of
the squeeze-excite and BatchNorm layers) are compared at 1e-3 of their largest entry or tighter.
"""
import ctypes
import zlib

import pytest
import torch

from test_gpu_bench_shapes import _check_conv_launch, _check_wgrad_launch, _conv_sig, _pad_input, _tap_views, _wgrad_sig
from test_gpu_bench_shapes_more import _bn_sig, _drop_engine_tensors

pytestmark = pytest.mark.gpu

STEP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoff of the storage type


def _rb(t, h16):
    """round a float64 tensor to the 16-bit storage type (through fp32, like the kernels' fp32 values)"""
    return t.float().to(h16).double()


def _close_h16(got, want, h16, frac=0.03, what="", carried=None):
    """got: a stored 16-bit tensor; want: the float64 reference rounded where the kernel rounds.  Every element within one
    step (2u of its value) plus u of the tensor's range (sums that cancel); the mean error within u/2 of the range; fewer
    than `frac` of the elements off at all.  For bfloat16 this is tests/test_gpu_bench_shapes.py::_close_bf16.
    carried: per-element bound of a one-step flip at an EARLIER rounding point carried to the output (chained roundings)."""
    u = STEP[h16]
    got, want = got.double(), want.double()
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs()
    excess = err - (2 * u * want.abs() + u * scale + (carried if carried is not None else 0.0))
    assert not (excess > 0).any(), (what, "outside one step", int((excess > 0).sum()), excess.max().item() / scale)
    assert err.mean().item() <= 0.5 * u * scale, (what, "mean error / range", err.mean().item() / scale)
    off = (got != want).double().mean().item()
    assert off < frac, (what, "fraction off", off)


def _gen(cuda, name):
    return torch.Generator(device=cuda).manual_seed(zlib.crc32(name.encode()) % (2 ** 31))


# ---- restated launch plans (coverage asserts) ---------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def slab_plan(C8, chunk_groups):
    """(channel groups per slab, slabs per pixel row): rn_train.hip:235-256 bn_slab_plan (chunk_groups = the segment's row
    chunks) and rn_depthwise.hip:557-581 se_slab_plan (chunk_groups = N * chunks) — the same policy, 256 threads"""
    old_n = (C8 + 7) // 8

    def score(n):
        g = _cdiv(C8, n)
        return C8 * (256 // g) / (n * 256)
    sg, ns = (C8 if C8 < 8 else 8), old_n
    if C8 >= 8 and C8 / (8.0 * old_n) >= 0.95:
        return sg, ns
    best = 0.0
    for n in range(1, old_n + 1):
        g = _cdiv(C8, n)
        if g > 64 or (g < 8 and n > 1):
            continue
        best = max(best, score(n))
    for n in range(1, old_n + 1):
        g = _cdiv(C8, n)
        if g > 64 or (g < 8 and n > 1) or score(n) < best - 0.01:
            continue
        if chunk_groups * n >= 512 or C8 < 8:
            return g, n
    return sg, ns


def bn_chunks_of(P, C):
    """rn_train.hip:629-637 without ext_chunks (the re-issued problems compute their own stage-1 partials)"""
    want = 2048 // _cdiv(C, 64)
    want = 256 if want < 256 else want
    rpc = max(_cdiv(_cdiv(P, want), 32) * 32, 32)
    return _cdiv(P, rpc)


def se_chunks(HW):
    """rn_depthwise.hip:583-591"""
    chunks = min(max(_cdiv(HW, 1024), 1), 32)
    rows = _cdiv(_cdiv(HW, chunks), 32) * 32
    return _cdiv(HW, rows)


def bn_plan(P, C):
    return slab_plan(C // 8, bn_chunks_of(P, C))


def se_plan(N, HW, C):
    return slab_plan(C // 8, N * se_chunks(HW))


def _wide_form(plan, C):
    """a slab form other than the 64-channel one (C8 >= 8 only: narrower layers always take the whole pixel)"""
    return C // 8 >= 8 and plan[0] != 8


EPI_RUNTIME = 8


def dw_epi(p):
    """the epilogue variant rn_depthwise_conv2d_nhwc_fwd compiles in (rn_depthwise.hip:191-196)"""
    s0 = p.seg[0]
    epi = (1 if (s0.scale or s0.shift) else 0) | (2 if s0.residual else 0) | (4 if p.act == 3 else 0)
    for i in range(1, p.num_segments):
        s = p.seg[i]
        if ((1 if (s.scale or s.shift) else 0) | (2 if s.residual else 0)) != (epi & 3):
            epi = EPI_RUNTIME
    return epi


def dw_items(p):
    """work items of a depthwise forward launch: 4-pixel strips x 8-channel groups (rn_depthwise.hip:184)"""
    return sum(s.N * s.Ho * _cdiv(s.Wo, 4) * (s.C // 8) for s in (p.seg[i] for i in range(p.num_segments)))


# ---- depthwise ----------------------------------------------------------------------------------------------------------
def _dw_sig(kind, p, ups=()):
    segs = tuple((s.N, s.H, s.W, s.C, s.Ho, s.Wo, bool(s.scale), bool(s.shift), bool(s.residual))
                 for s in (p.seg[i] for i in range(p.num_segments)))
    return (kind, p.k, p.stride, p.pad_top, p.pad_left, p.act, segs, tuple(u[2:] for u in ups))


def _dw_taps(xp, k, stride, Ho, Wo):
    for r, c, v in _tap_views(xp, k, k, stride, Ho, Wo):
        yield r * k + c, v


def _check_dw_launch(cuda, lib, h16, name, kind, p, ups):
    """re-issue one depthwise forward ("fwd") or data-gradient ("dgrad") launch on fresh tensors of its geometry"""
    from retinanet import _C
    g = _gen(cuda, name)
    st = _C.current_stream()
    k = p.k
    q = _C.DwProblem()
    q.k, q.stride, q.pad_top, q.pad_left, q.act, q.num_segments = k, p.stride, p.pad_top, p.pad_left, p.act, p.num_segments
    per_seg = []
    for i in range(p.num_segments):
        s, d = p.seg[i], q.seg[i]
        t = {}
        master = torch.randn((k * k, s.C), generator=g, device=cuda) / k      # f32 [k*k][C] (the Keras [k,k,C,1] order)
        w = torch.empty((k * k, s.C), dtype=h16, device=cuda)
        if kind == "fwd":
            t["x"] = torch.randn((s.N, s.H, s.W, s.C), generator=g, device=cuda).to(h16)
            _C.check(lib.rn_pack_depthwise_weight(_C.ptr(master), k, s.C, _C.ptr(w), st), name)
            src = t["x"]
        else:
            # the forward layer this gradient belongs to: stride 2 when the engine zero-upsamples dy first
            t["s"] = 2 if ups else 1
            Hf, Wf = (ups[i][3], ups[i][4]) if ups else (s.H, s.W)
            t["dy"] = (torch.randn((s.N, Hf, Wf, s.C), generator=g, device=cuda)
                       * (torch.rand((s.N, Hf, Wf, 1), generator=g, device=cuda) < 0.7)).to(h16)
            _C.check(lib.rn_pack_depthwise_weight_flip(_C.ptr(master), k, s.C, _C.ptr(w), st), name)
            src = t["dy"]
            if ups:
                assert tuple(ups[i][2:]) == (s.N, Hf, Wf, s.C, s.H, s.W), name
                src = torch.full((s.N, s.H, s.W, s.C), float("nan"), dtype=h16, device=cuda)
                _C.check(lib.rn_upsample_zero2x(_C.ptr(t["dy"]), _C.ptr(src), s.N, Hf, Wf, s.C, s.H, s.W, st), name)
        t["w16"] = master.to(h16).double()
        y = torch.full((s.N, s.Ho, s.Wo, s.C), float("nan"), dtype=h16, device=cuda)
        if s.scale:
            t["scale"] = torch.rand((s.C,), generator=g, device=cuda) + 0.5
        if s.shift:
            t["shift"] = torch.randn((s.C,), generator=g, device=cuda) * 0.1
        if s.residual:
            t["res"] = torch.randn((s.N, s.Ho, s.Wo, s.C), generator=g, device=cuda).to(h16)
            if s.residual == s.y:          # the accumulating data gradients: residual = the gradient buffer itself
                y.copy_(t["res"])
        d.x, d.w, d.y = src.data_ptr(), w.data_ptr(), y.data_ptr()
        d.scale = t["scale"].data_ptr() if "scale" in t else None
        d.shift = t["shift"].data_ptr() if "shift" in t else None
        d.residual = (y.data_ptr() if s.residual == s.y else t["res"].data_ptr()) if s.residual else None
        d.N, d.H, d.W, d.C, d.Ho, d.Wo = s.N, s.H, s.W, s.C, s.Ho, s.Wo
        t.update(y=y, w=w, src=src)
        per_seg.append(t)
    _C.check(lib.rn_depthwise_conv2d_nhwc_fwd(ctypes.byref(q), st), name)
    torch.cuda.synchronize()
    for i, t in enumerate(per_seg):
        s = p.seg[i]
        if kind == "fwd":
            # y = sum over taps x[p + tap] * w[tap]: gather
            xp = _pad_input(t["x"].double(), k, k, p.stride, p.pad_top, p.pad_left, s.Ho, s.Wo)
            acc = torch.zeros((s.N, s.Ho, s.Wo, s.C), dtype=torch.float64, device=cuda)
            for tap, v in _dw_taps(xp, k, p.stride, s.Ho, s.Wo):
                acc += v * t["w16"][tap]
            del xp
        else:
            # the adjoint of the forward layer: scatter dy[o] * w[tap] to x[o * stride + tap - pad] (the kernel gathers with
            # the tap-reversed filter over the zero-upsampled dy)
            sf = t["s"]
            pt, pl = k - 1 - p.pad_top, k - 1 - p.pad_left
            dy = t["dy"].double()
            Hf, Wf = dy.shape[1], dy.shape[2]
            Hp, Wp = max((Hf - 1) * sf + k, pt + s.H), max((Wf - 1) * sf + k, pl + s.W)
            accp = torch.zeros((s.N, Hp, Wp, s.C), dtype=torch.float64, device=cuda)
            for r in range(k):
                for c in range(k):
                    accp[:, r:r + sf * (Hf - 1) + 1:sf, c:c + sf * (Wf - 1) + 1:sf, :] += dy * t["w16"][r * k + c]
            acc = accp[:, pt:pt + s.H, pl:pl + s.W, :].contiguous()
            del accp, dy
        v = acc
        affine = "scale" in t or "shift" in t
        carried = None
        if affine:
            # two chained rounding points (the conv output, then the BatchNorm output in front of swish): a one-step flip of
            # either, where an fp32 sum straddles a boundary, reaches the output through |scale| and |swish'| <= 1.1
            sc = t["scale"].double() if "scale" in t else 1.0
            v = _rb(v, h16) * sc + (t["shift"].double() if "shift" in t else 0.0)
            carried = 2 * STEP[h16] * 1.1 * (_rb(acc, h16).abs() * abs(sc) + v.abs())
        if "res" in t:
            v = (_rb(v, h16) if affine else v) + t["res"].double()
        if p.act == 3:       # swish on the 16-bit BatchNorm output
            v = _rb(v, h16)
            v = v * torch.sigmoid(v)
        elif p.act == 1:
            v = v.relu()
        assert p.act in (0, 1, 3), name
        _close_h16(t["y"], _rb(v, h16), h16, what=(name, i), carried=carried)
        del acc, v


def _check_dw_wgrad_launch(cuda, lib, h16, name, p):
    from retinanet import _C
    g = _gen(cuda, name)
    k = p.k
    q = _C.DwProblem()
    q.k, q.stride, q.pad_top, q.pad_left, q.act, q.num_segments = k, p.stride, p.pad_top, p.pad_left, 0, p.num_segments
    C = p.seg[0].C
    want = torch.zeros((k * k, C), dtype=torch.float64, device=cuda)
    keep = []
    for i in range(p.num_segments):
        s, d = p.seg[i], q.seg[i]
        x = torch.randn((s.N, s.H, s.W, s.C), generator=g, device=cuda).to(h16)
        dy = (torch.randn((s.N, s.Ho, s.Wo, s.C), generator=g, device=cuda)
              * (torch.rand((s.N, s.Ho, s.Wo, 1), generator=g, device=cuda) < 0.7)).to(h16)
        d.x, d.y, d.w = x.data_ptr(), dy.data_ptr(), None
        d.N, d.H, d.W, d.C, d.Ho, d.Wo = s.N, s.H, s.W, s.C, s.Ho, s.Wo
        keep += [x, dy]
        xp = _pad_input(x.double(), k, k, p.stride, p.pad_top, p.pad_left, s.Ho, s.Wo)
        dyd = dy.double()
        for tap, v in _dw_taps(xp, k, p.stride, s.Ho, s.Wo):
            want[tap] += (v * dyd).sum(dim=(0, 1, 2))
        del xp, dyd
    nbytes = lib.rn_depthwise_wgrad_workspace_bytes(ctypes.byref(q))
    assert nbytes == lib.rn_depthwise_wgrad_workspace_bytes(ctypes.byref(p)) > 0, name
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=cuda)
    ws.fill_(0x7f)
    dw = torch.full((k * k, C), 7.0, dtype=torch.float32, device=cuda)
    st = _C.current_stream()
    _C.check(lib.rn_depthwise_conv2d_nhwc_wgrad(ctypes.byref(q), _C.ptr(dw), _C.ptr(ws), ws.numel(), st), name)
    torch.cuda.synchronize()
    first = dw.clone()
    scale = want.abs().max().item()
    torch.testing.assert_close(dw.double(), want, rtol=1e-3, atol=1e-3 * scale)
    _C.check(lib.rn_depthwise_conv2d_nhwc_wgrad(ctypes.byref(q), _C.ptr(dw), _C.ptr(ws), ws.numel(), st), name)
    torch.cuda.synchronize()
    assert torch.equal(dw, first), name       # deterministic two-stage reduction: the same bits


# ---- squeeze-excite -----------------------------------------------------------------------------------------------------
def se_tensors(cuda, g, N, HW, C, se, h16):
    """fresh operands of one SE layer: x [N][HW][C], W1 [se][C], b1, W2 [C][se], b2, dy (16-bit where the ABI says so)"""
    x = (torch.randn((N, HW, C), generator=g, device=cuda) + 0.3).to(h16)
    w1 = (torch.randn((se, C), generator=g, device=cuda) * (2.0 / C) ** 0.5).to(h16)
    b1 = torch.randn((se,), generator=g, device=cuda) * 0.1
    w2 = (torch.randn((C, se), generator=g, device=cuda) * (2.0 / se) ** 0.5).to(h16)
    b2 = torch.randn((C,), generator=g, device=cuda) * 0.1
    dy = (torch.randn((N, HW, C), generator=g, device=cuda)
          * (torch.rand((N, HW, 1), generator=g, device=cuda) < 0.7)).to(h16)
    return x, w1, b1, w2, b2, dy


def se_state_views(state, N, C, se):
    """pooled [N][C], gate [N][C], h1 [N][se], a [N][se] (f32) at the front of the state buffer (rn_depthwise.hip:683-685)"""
    f = state.view(torch.float32)
    nc = N * C
    return (f[:nc].view(N, C), f[nc:2 * nc].view(N, C), f[2 * nc:2 * nc + N * se].view(N, se),
            f[2 * nc + N * se:2 * nc + 2 * N * se].view(N, se))


def check_se_forward(x, y, state, w1, b1, w2, b2, h16, what):
    """y = x * gate with pooled, h1, swish(h1) and gate 16-bit (rnet_hip.h:721-735, efficientnet.py:252-265).  Each stage is
    checked against float64 from the kernel's own stored input of that stage (one step where an fp32 sum straddles), then
    y end to end against the reference that never looks at the kernel."""
    N, HW, C = x.shape
    se = w1.shape[0]
    pooled, gate, h1, a = (t.double() for t in se_state_views(state, N, C, se))
    xd = x.double()
    W1, W2 = w1.double(), w2.double()
    pooled_ref = _rb(xd.sum(1) / HW, h16)
    _close_h16(pooled, pooled_ref, h16, what=(what, "pooled"))
    h1_ref = _rb(pooled @ W1.t() + b1.double(), h16)
    _close_h16(h1, h1_ref, h16, what=(what, "h1"))
    a_ref = _rb(h1 * torch.sigmoid(h1), h16)
    _close_h16(a, a_ref, h16, what=(what, "swish(h1)"))
    gate_ref = _rb(torch.sigmoid(_rb(a @ W2.t() + b2.double(), h16)), h16)
    _close_h16(gate, gate_ref, h16, what=(what, "gate"))
    # x * gate of two 16-bit values is exact in fp32: one rounding, the same as the reference's
    _close_h16(y.double(), _rb(xd * gate[:, None, :], h16), h16, frac=1e-3, what=(what, "y"))
    # end to end
    h1_full = _rb(pooled_ref @ W1.t() + b1.double(), h16)
    a_full = _rb(h1_full * torch.sigmoid(h1_full), h16)
    g_full = _rb(torch.sigmoid(_rb(a_full @ W2.t() + b2.double(), h16)), h16)
    want = _rb(xd * g_full[:, None, :], h16)
    err = (y.double() - want).abs()
    u = STEP[h16]
    assert (err <= 2 * u * want.abs() + 1e-30).double().mean().item() > 0.97, (what, "y end to end")
    assert (err <= 8 * u * want.abs() + u * want.abs().max()).all(), (what, "y end to end, max")
    return pooled, gate, h1, a


def check_se_backward(x, dy, dx, state, w1, w2, dw1, db1, dw2, db2, h16, what):
    """rn_squeeze_excite_bwd: dgate = sum_hw dy * x, dh2 = dgate * g(1 - g), dh1 = (W2^T dh2) * swish'(h1), dp = W1^T dh1,
    dx = dy * g + dp / HW, parameter gradients summed over the images — through the 16-bit values of `state`"""
    N, HW, C = x.shape
    se = w1.shape[0]
    pooled, gate, h1, a = (t.double() for t in se_state_views(state, N, C, se))
    dyd = dy.double()
    dgate = (dyd * x.double()).sum(1)
    dh2 = dgate * gate * (1 - gate)
    sg = torch.sigmoid(h1)
    dh1 = (dh2 @ w2.double()) * (sg + h1 * sg * (1 - sg))
    dp = dh1 @ w1.double()
    for nm, got, want in (("dw1", dw1, dh1.t() @ pooled), ("db1", db1, dh1.sum(0)), ("dw2", dw2, dh2.t() @ a),
                          ("db2", db2, dh2.sum(0))):
        scale = want.abs().max().item()
        torch.testing.assert_close(got.double(), want.reshape(got.shape), rtol=1e-3, atol=2e-4 * scale,
                                   msg=lambda m, nm=nm: f"{what} {nm}: {m}")
    _close_h16(dx.double(), _rb(dyd * gate[:, None, :] + dp[:, None, :] / HW, h16), h16, what=(what, "dx"))


def _check_se_launch(cuda, lib, h16, name, N, HW, C, se):
    """one forward + backward pair of the training engine's geometry (the backward reads the forward's state)"""
    from retinanet import _C
    g = _gen(cuda, name)
    x, w1, b1, w2, b2, dy = se_tensors(cuda, g, N, HW, C, se, h16)
    nbytes = lib.rn_se_workspace_bytes(N, C)
    state = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=cuda)     # NaN floats where nothing was written
    ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=cuda)
    y = torch.full_like(x, float("nan"))
    st = _C.current_stream()
    _C.check(lib.rn_squeeze_excite_fwd(_C.ptr(x), _C.ptr(y), N, HW, C, _C.ptr(w1), _C.ptr(b1), _C.ptr(w2), _C.ptr(b2), se,
                                       _C.ptr(state), nbytes, st), name)
    dx = torch.full_like(x, float("nan"))
    grads = [torch.full(shp, float("nan"), device=cuda) for shp in ((se, C), (se,), (C, se), (C,))]
    _C.check(lib.rn_squeeze_excite_bwd(_C.ptr(x), _C.ptr(dy), _C.ptr(dx), N, HW, C, _C.ptr(w1), _C.ptr(w2), se, _C.ptr(state),
                                       *[_C.ptr(t) for t in grads], _C.ptr(ws), nbytes, st), name)
    torch.cuda.synchronize()
    check_se_forward(x, y, state, w1, b1, w2, b2, h16, name)
    check_se_backward(x, dy, dx, state, w1, w2, *grads, h16, name)


# ---- BatchNorm (with swish and stochastic-depth factors) ----------------------------------------------------------------
def check_bn_problem_h16(cuda, lib, h16, p, name, dz_inf=False):
    """_check_bn_problem of tests/test_gpu_bench_shapes_more.py in steps of the storage type, extended to the swish groups
    (forward rb(u) * sigmoid(rb(u)); backward through swish' recomputed from the fp32 pre-activation u, as the kernel does)
    and to the per-image stochastic-depth factors `sample_scale` (forward rb(rb(u) * m); the gradient g * m enters the
    sums and dy, dres gets g: rn_train.hip:198, 500-512, 577-587).  dz_inf: one dz element is +inf, and the parameter
    gradients must come out non-finite (the loss-scale skip relies on it) — no other check."""
    from retinanet import _C
    g = torch.Generator(device=cuda).manual_seed(zlib.crc32(repr(_bn_sig(p)).encode()) % (2 ** 31))
    q = _C.BnProblem()
    q.num_segments, q.act, q.bessel, q.eps, q.momentum, q.count_scale = p.num_segments, p.act, p.bessel, p.eps, p.momentum, 1.0
    T = []
    for i in range(p.num_segments):
        s, d = p.seg[i], q.seg[i]
        P, C = int(s.P), int(s.C)
        t = {"y": (torch.randn((P, C), generator=g, device=cuda) * 1.5 + 0.3).to(h16),
             "dz": (torch.randn((P, C), generator=g, device=cuda)
                    * (torch.rand((P, 1), generator=g, device=cuda) < 0.8)).to(h16),
             "gamma": torch.rand((C,), generator=g, device=cuda) + 0.5, "beta": torch.randn((C,), generator=g, device=cuda) * 0.3,
             "mm": torch.randn((C,), generator=g, device=cuda), "mv": torch.rand((C,), generator=g, device=cuda) + 0.5}
        if dz_inf:
            t["dz"][P // 2, C // 3] = float("inf")
        t["mm0"], t["mv0"] = t["mm"].clone(), t["mv"].clone()
        t["z"], t["dy"] = torch.full_like(t["y"], float("nan")), torch.full_like(t["y"], float("nan"))
        if s.residual:
            t["res"] = torch.randn((P, C), generator=g, device=cuda).to(h16)
        if s.dres:
            t["dres"] = torch.randn((P, C), generator=g, device=cuda).to(h16)
            t["dres0"] = t["dres"].clone()
        if s.act_mask:
            t["mask"] = torch.full((P * C // 8,), 0xA5, dtype=torch.uint8, device=cuda)
        if s.sample_scale:
            rows = int(s.rows_per_sample)
            assert rows > 0 and P % rows == 0, name
            nimg = P // rows
            # drop_connect factors: 0 for a dropped image, 1 / survival_prob for a kept one
            keep = torch.rand((nimg,), generator=g, device=cuda) < 0.8
            t["m"] = keep.float() / 0.85
            t["m"][0], t["m"][-1] = 0.0, 1.0 / 0.85
            d.sample_scale, d.rows_per_sample = t["m"].data_ptr(), rows
        for k, shape in (("sums", (2, C)), ("bsums", (2, C)), ("fwd", (4, C))):
            t[k] = torch.zeros(shape, dtype=torch.float32, device=cuda)
        t["dgamma"], t["dbeta"] = torch.zeros((C,), device=cuda), torch.zeros((C,), device=cuda)
        d.y, d.z, d.dz, d.dy = t["y"].data_ptr(), t["z"].data_ptr(), t["dz"].data_ptr(), t["dy"].data_ptr()
        d.residual = t["res"].data_ptr() if "res" in t else None
        d.dres = t["dres"].data_ptr() if "dres" in t else None
        d.act_mask = t["mask"].data_ptr() if "mask" in t else None
        d.sums, d.bsums, d.fwd = t["sums"].data_ptr(), t["bsums"].data_ptr(), t["fwd"].data_ptr()
        d.gamma, d.beta, d.moving_mean, d.moving_var = (t["gamma"].data_ptr(), t["beta"].data_ptr(), t["mm"].data_ptr(),
                                                        t["mv"].data_ptr())
        d.dgamma, d.dbeta = t["dgamma"].data_ptr(), t["dbeta"].data_ptr()
        d.P, d.C, d.dres_accumulate = P, C, s.dres_accumulate
        T.append(t)
    ws = torch.zeros((max(lib.rn_bn_workspace_bytes(ctypes.byref(q)), 256),), dtype=torch.uint8, device=cuda)
    st = _C.current_stream()
    _C.check(lib.rn_bn_stats_finalize(ctypes.byref(q), _C.ptr(ws), ws.numel(), st), name)
    _C.check(lib.rn_bn_apply(ctypes.byref(q), st), name)
    if all("mask" in t for t in T):
        torch.cuda.synchronize()
        zs = [t["z"].clone() for t in T]
        for t in T:
            t["z"].fill_(float("nan"))       # with the bit mask the backward passes must not look at z
    else:
        zs = [t["z"] for t in T]
    _C.check(lib.rn_bn_bwd_reduce(ctypes.byref(q), _C.ptr(ws), ws.numel(), st), name)
    _C.check(lib.rn_bn_bwd_apply(ctypes.byref(q), st), name)
    torch.cuda.synchronize()
    if dz_inf:
        for i, t in enumerate(T):
            assert not torch.isfinite(t["dgamma"]).all() and not torch.isfinite(t["dbeta"]).all(), (name, i)
        return
    eps, mom = float(p.eps), float(p.momentum)
    rb = lambda v: _rb(v, h16)      # noqa: E731
    for i, (t, z) in enumerate(zip(T, zs)):
        y = t["y"].double()
        n = y.shape[0]
        mean = y.mean(0)
        var = (y * y).mean(0) - mean * mean
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = t["gamma"].double() * invstd
        shift = t["beta"].double() - mean * scale
        fwd = t["fwd"].double()
        torch.testing.assert_close(fwd[0], mean, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(fwd[1], invstd, rtol=2e-5, atol=0)
        torch.testing.assert_close(fwd[2], scale, rtol=2e-5, atol=0)
        torch.testing.assert_close(fwd[3], shift, rtol=1e-4, atol=2e-5)
        corr = n / (n - 1.0) if p.bessel else 1.0
        torch.testing.assert_close(t["mm"].double(), t["mm0"].double() * mom + mean * (1 - mom), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(t["mv"].double(), t["mv0"].double() * mom + var * corr * (1 - mom), rtol=1e-5, atol=1e-5)
        m = t["m"].double().repeat_interleave(int(p.seg[i].rows_per_sample))[:, None] if "m" in t else None
        # forward with the kernel's own fp32 scale / shift: the rounding points of rn_bn_apply
        uu = y * fwd[2] + fwd[3]
        v = uu
        if "res" in t or m is not None or p.act == _C.RN_ACT_SWISH:
            v = rb(v)
        if m is not None:
            v = rb(v * m)
        if "res" in t:
            v = v + t["res"].double()
            if p.act == _C.RN_ACT_SWISH:
                v = rb(v)
        if p.act == _C.RN_ACT_RELU:
            v = v.relu()
        elif p.act == _C.RN_ACT_RELU6:
            v = v.clamp(0.0, 6.0)
        elif p.act == _C.RN_ACT_SWISH:
            v = v * torch.sigmoid(v)
        want_z = rb(v)
        got_z = z.double()
        _close_h16(got_z, want_z, h16, frac=0.02, what=(name, i, "z"))
        # backward: the gate from the STORED z (relu / relu6), swish' from the unrounded pre-activation
        if p.act == _C.RN_ACT_RELU:
            gate = (got_z > 0).double()
        elif p.act == _C.RN_ACT_RELU6:
            gate = ((got_z > 0) & (got_z < 6)).double()
        elif p.act == _C.RN_ACT_SWISH:
            sg = torch.sigmoid(uu)
            gate = sg + uu * sg * (1 - sg)
        else:
            gate = torch.ones_like(got_z)
        if "mask" in t:
            bits = ((t["mask"].view(-1, 1) >> torch.arange(8, device=cuda, dtype=torch.uint8)) & 1).reshape(got_z.shape)
            assert torch.equal(bits.double(), gate), (name, i)
        gg = t["dz"].double() * gate
        ggm = gg * m if m is not None else gg
        xhat = (y - fwd[0]) * fwd[1]
        sg0, sgx = ggm.sum(0), (ggm * xhat).sum(0)
        bs = t["bsums"].double()
        for nm, got, want in (("bsums0", bs[0], sg0), ("bsums1", bs[1], sgx), ("dbeta", t["dbeta"].double(), sg0),
                              ("dgamma", t["dgamma"].double(), sgx)):
            torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-5 * want.abs().max().item() + 1e-6,
                                       msg=lambda msg, nm=nm: f"{name} {i} {nm}: {msg}")
        want_dy = rb(fwd[2] * (ggm - bs[0] / n - xhat * bs[1] / n))
        _close_h16(t["dy"].double(), want_dy, h16, what=(name, i, "dy"))
        if "dres" in t:
            want_r = rb(gg + (t["dres0"].double() if p.seg[i].dres_accumulate else 0.0))
            _close_h16(t["dres"].double(), want_r, h16, frac=0.01, what=(name, i, "dres"))
        del y, v, uu, want_z, got_z, gg, ggm, xhat, want_dy


# ---- the engines --------------------------------------------------------------------------------------------------------
class _Stub:
    """what the per-launch checks of tests/test_gpu_bench_shapes.py need of the engine"""
    def __init__(self, lib, h16):
        self.lib, self.h16 = lib, h16


def _failure(name, e):
    return (name, str(e).splitlines()[0][:300] if str(e) else "assert")


@pytest.fixture(scope="module")
def train_launches(cuda):
    """the configs[4] training engine exactly as bench.py builds it; its distinct launches; its tensors freed"""
    from retinanet.cfg import efficientnet_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = efficientnet_params("efficientnet-b3", input_size=640)
    p.architecture.batch_norm.use_sync = False
    model = ModelBuilder(p, "train", device=cuda, seed=1337)()
    eng = TrainEngine(model, 32, frozen_regexes=[])
    assert eng.f16 and eng.h16 == torch.float16

    def dedup(items, sig):
        out, seen = [], set()
        for it in items:
            k = sig(it)
            if k not in seen:
                seen.add(k)
                out.append(it)
        return out
    r = {"lib": eng.lib, "h16": eng.h16,
         "convs": dedup(eng.conv_launches, lambda it: _conv_sig(eng, *it)),
         "wgrads": dedup(eng.wgrad_launches, lambda it: _wgrad_sig(*it)),
         "dws": dedup(eng.dw_launches, lambda it: _dw_sig(it[1], it[2], it[3])),
         "dw_wgrads": dedup(eng.dw_wgrad_launches, lambda it: _dw_sig("wgrad", it[1])),
         "ses": dedup(eng.se_launches, lambda it: it[1:]),
         "bns": dedup([(out, grp[0]) for out, grp in eng.bn_groups.items()], lambda it: _bn_sig(it[1])),
         "dw_shapes": {(d["k"], d["stride"]) for d in eng.g.dws.values()}}
    r["keep"] = _drop_engine_tensors(eng)
    del eng, model
    torch.cuda.empty_cache()
    yield r
    torch.cuda.empty_cache()


def test_config4_conv_launches(cuda, train_launches):
    """(a) every distinct implicit-GEMM launch (forward / data gradient / weight gradient) on the half build"""
    r = train_launches
    lib, h16 = r["lib"], r["h16"]
    stub = _Stub(lib, h16)
    # (every training conv feeds a BatchNorm: its activation — swish — runs in rn_bn_apply, checked in (d))
    assert {p.act for _, p in r["convs"]} == {0}
    cins = {p.seg[i].Cin for _, p in r["convs"] for i in range(p.num_segments)}
    assert {24, 40} <= cins, sorted(cins)                                    # channel-padded 1 x 1 layers
    assert any(p.num_segments > 1 for _, p in r["convs"])                   # the grouped head levels
    failures = []
    for name, p in r["convs"]:
        try:
            _check_conv_launch(cuda, stub, name, p, close=lambda got, want: _close_h16(got, want, h16))
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    for name, p in r["wgrads"]:
        try:
            _check_wgrad_launch(cuda, stub, name, p)
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    print(f"configs[4] B=32: {len(r['convs'])} distinct conv launches, {len(r['wgrads'])} distinct weight-gradient launches "
          "checked")
    assert not failures, failures


def test_config4_depthwise_launches(cuda, train_launches):
    """(b) every distinct depthwise forward / data-gradient / weight-gradient launch"""
    r = train_launches
    lib, h16 = r["lib"], r["h16"]
    fwd = [(n, p, u) for n, kind, p, u in r["dws"] if kind == "fwd"]
    dgr = [(n, p, u) for n, kind, p, u in r["dws"] if kind == "dgrad"]
    # coverage: every (k, stride) of the network forward and as weight gradient; stride-2 data gradients through the
    # zero-upsampling; the accumulating form; multi-segment launches; grids that loop (> 32768 workgroups of 256 items)
    assert {(p.k, p.stride) for _, p, _ in fwd} == r["dw_shapes"], r["dw_shapes"]
    assert {(p.k, p.stride) for _, p in r["dw_wgrads"]} == r["dw_shapes"], r["dw_shapes"]
    assert r["dw_shapes"] >= {(3, 1), (5, 1), (3, 2), (5, 2)}, r["dw_shapes"]
    assert {p.k for _, p, u in dgr if u} == {3, 5}, "stride-2 data gradients"
    assert any(p.seg[i].residual for _, p, _ in dgr for i in range(p.num_segments)), "accumulating data gradient"
    assert any(p.num_segments > 1 for _, p, _ in fwd) and any(p.num_segments > 1 for _, p, _ in dgr)
    assert any(p.num_segments > 1 for _, p in r["dw_wgrads"])
    assert any(dw_items(p) > 32768 * 256 for _, p, _ in fwd + dgr), "a grid-stride loop that runs more than once"
    n_runtime = sum(dw_epi(p) == EPI_RUNTIME for _, p, _ in fwd + dgr)
    failures = []
    for kind, launches in (("fwd", fwd), ("dgrad", dgr)):
        for name, p, ups in launches:
            try:
                _check_dw_launch(cuda, lib, h16, name, kind, p, ups)
            except AssertionError as e:
                failures.append(_failure(name, e))
            torch.cuda.empty_cache()
    for name, p in r["dw_wgrads"]:
        try:
            _check_dw_wgrad_launch(cuda, lib, h16, name, p)
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    print(f"configs[4] B=32: {len(fwd)} forward + {len(dgr)} data-gradient depthwise launches ({n_runtime} with the run-time "
          f"epilogue), {len(r['dw_wgrads'])} depthwise weight-gradient launches checked")
    assert not failures, failures


def test_config4_squeeze_excite_launches(cuda, train_launches):
    """(c) every distinct squeeze-excite geometry, forward and backward (one pair per geometry: the backward reads the
    state the forward wrote); at least one launch on a pooling slab form other than the 64-channel one"""
    r = train_launches
    lib, h16 = r["lib"], r["h16"]
    geo = sorted({it[2:] for it in r["ses"]})
    assert {it[1] for it in r["ses"]} == {"fwd", "bwd"}
    assert {it[2:] for it in r["ses"] if it[1] == "fwd"} == {it[2:] for it in r["ses"] if it[1] == "bwd"}
    plans = {g: se_plan(g[0], g[1], g[2]) for g in geo}
    assert any(_wide_form(plans[g], g[2]) for g in geo), plans
    failures = []
    for N, HW, C, se in geo:
        name = f"se:{N}x{HW}x{C}/{se}"
        try:
            _check_se_launch(cuda, lib, h16, name, N, HW, C, se)
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    print(f"configs[4] B=32: {len(geo)} distinct squeeze-excite geometries (forward + backward) checked, slab plans "
          f"{sorted(set(plans.values()))}")
    assert not failures, failures


def test_config4_batchnorm_launches(cuda, train_launches):
    """(d) every distinct BatchNorm problem of the engine, the swish and stochastic-depth groups included"""
    from retinanet import _C
    r = train_launches
    lib, h16 = r["lib"], r["h16"]
    probs = r["bns"]
    sigs = [_bn_sig(pb) for _, pb in probs]
    assert any(pb.act == _C.RN_ACT_SWISH for _, pb in probs)
    assert any(s[6] for sig in sigs for s in sig[3]), "a sample_scale (stochastic depth) group"
    plans = {(int(pb.seg[i].P), int(pb.seg[i].C)): bn_plan(int(pb.seg[i].P), int(pb.seg[i].C))
             for _, pb in probs for i in range(pb.num_segments)}
    assert any(_wide_form(v, C) for (P, C), v in plans.items()), plans
    failures = []
    for name, pb in probs:
        try:
            check_bn_problem_h16(cuda, lib, h16, pb, name)
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    wide = sorted({(C, v) for (P, C), v in plans.items() if _wide_form(v, C)})
    print(f"configs[4] B=32: {len(probs)} distinct BatchNorm problems checked; slab forms other than 64 channels: {wide}")
    assert not failures, failures


def test_config4_serving_launches(cuda):
    """(e) the configs[4] serving engine at batch 8: its depthwise launches (folded BatchNorm + swish) and its in-place
    squeeze-excite launches"""
    from retinanet import _C
    from retinanet.cfg import efficientnet_params
    from retinanet.model import ModelBuilder
    p = efficientnet_params("efficientnet-b3", input_size=640)
    p.architecture.batch_norm.use_sync = False
    model = ModelBuilder(p, "val", device=cuda, seed=1337)()
    eng = model.inference_engine(8)
    assert eng.f16
    lib, h16 = eng.lib, eng.h16
    dws, seen = [], set()
    for name, pd in eng.dw_launches:
        sig = _dw_sig("fwd", pd)
        if sig not in seen:
            seen.add(sig)
            dws.append((name, pd))
    ses = sorted(set(s[1:] for s in eng.se_launches))
    assert dws and ses
    epis = sorted({dw_epi(pd) for _, pd in dws})
    assert 5 in epis, epis        # folded BatchNorm + swish
    keep = eng._keep
    eng.t.clear()
    del eng
    model._engines.clear()
    torch.cuda.empty_cache()
    failures = []
    for name, pd in dws:
        try:
            _check_dw_launch(cuda, lib, h16, name, "fwd", pd, [])
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    st = _C.current_stream()
    for N, HW, C, se in ses:
        name = f"se_inplace:{N}x{HW}x{C}/{se}"
        try:
            g = _gen(cuda, name)
            x, w1, b1, w2, b2, _ = se_tensors(cuda, g, N, HW, C, se, h16)
            x0 = x.clone()
            nbytes = lib.rn_se_workspace_bytes(N, C)
            ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=cuda)
            _C.check(lib.rn_squeeze_excite_inplace(_C.ptr(x), N, HW, C, _C.ptr(w1), _C.ptr(b1), _C.ptr(w2), _C.ptr(b2), se,
                                                   _C.ptr(ws), nbytes, st), name)
            torch.cuda.synchronize()
            check_se_forward(x0, x, ws, w1, b1, w2, b2, h16, name)
        except AssertionError as e:
            failures.append(_failure(name, e))
        torch.cuda.empty_cache()
    del keep
    print(f"configs[4] serving B=8: {len(dws)} distinct depthwise launches (epilogue variants {epis}), {len(ses)} distinct "
          "in-place squeeze-excite launches checked")
    assert not failures, failures
