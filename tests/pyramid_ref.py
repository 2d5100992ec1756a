"""Float64 references of the small NHWC kernels around the convolutions, and the rule that compares a kernel with them.

Every operation is written from its definition on CPU float64 tensors in NHWC layout: max-pool (forward / backward), the
FPN top-down pass (forward / backward), BalanceFeatures (forward / backward), the stride-2 placement kernels
(zero-insertion upsample, scatter-add, depth-to-space), the activation gate and the row reduction.  A tensor is rounded
to the 16-bit storage type exactly where the kernel stores one (`round_storage`: ONE round-to-nearest-even from float64,
not through float32).

The acceptance rule (derived, not tuned)
----------------------------------------
A kernel output element is `got = rs(s32)`: `rs` rounds to storage, `s32` is an fp32 evaluation of a sum of n terms
(a product with 1/L counts as one more operation).  The reference is `ref = rs(s)`, s the exact sum.
  * fp32 evaluation: |s32 - s| <= (n - 1) u (1 + u)^(n-1) sum|terms| with u = 2^-24, which is below n 2^-23 sum|terms|
    for every n used here (n <= 600).
  * the two roundings: |got - s32| <= ulp(s32) / 2 and |ref - s| <= ulp(s) / 2.  With `ulp_s(ref)` taken as
    eps * max(|ref|, smallest normal), eps = 2^-7 (bfloat16, 8 significant bits) or 2^-10 (half, 11 bits) — between
    one and two times the spacing of ref's own binade, hence at least the spacing on either side of ref — the two
    halves add up to at most ulp_s(ref).  Below the smallest normal the spacing is constant, eps * smallest normal.
So      |got - ref| <= ulp_s(ref) + n 2^-23 sum|terms|                                            (`Ref.bound`)
`sum|terms|` is computed by the reference next to the value.  Where an element reads an intermediate that the kernel
itself rounded to storage (the scratch `davg` of the BalanceFeatures backward, the finer level's `din` of the top-down
backward, the coarser `out` of the top-down forward, `avg` of the BalanceFeatures forward), the kernel's copy of that
intermediate may sit one storage step away from the reference's; the element's bound grows by `ulp_s(intermediate)`
times the factor the formula applies to it (`Ref.extra`: summed over the window for a sum-pool, times 1/L for the
average, the window's maximum for a max-pool, times the gate).  No element is exempt.

What the rule cannot tell apart: a `davg` that is NOT rounded to storage differs from the rounded one by at most half a
storage step per element, which is inside the one-step `extra` every reader of `davg` is granted.  The rule therefore
accepts an unrounded `davg` (test_pyramid_ref_cpu.py pins that this is so); the scratch itself is compared directly.

Pure data movement and routing (max-pool forward, upsample, depth-to-space without accumulate, casts, the activation
gate) has no rounding: those are compared bit for bit, not through `Ref.bound`.
"""
from typing import NamedTuple

import torch

F64 = torch.float64
# significant bits, exponent of the subnormal spacing, machine epsilon, smallest normal, largest finite
_FMT = {torch.bfloat16: (8, -133, 2.0 ** -7, 2.0 ** -126, float(torch.finfo(torch.bfloat16).max)),
        torch.float16: (11, -24, 2.0 ** -10, 2.0 ** -14, 65504.0)}


def round_storage(x, dtype):
    """float64 -> the nearest value of `dtype` (ties to even), returned as float64.  One rounding.  dtype None: no
    rounding (the exact formula, for the comparison with autograd)."""
    if dtype is None:
        return x
    p, qmin, _, _, big = _FMT[dtype]
    _, e = torch.frexp(x)                                    # |x| in [2^(e-1), 2^e)
    step = torch.exp2(torch.clamp(e - p, min=qmin).to(F64))  # spacing of dtype in x's binade (a power of two: exact)
    r = torch.round(x / step) * step                         # torch.round: half to even
    return torch.where(r.abs() > big, torch.sign(r) * float("inf"), r)


def ulp_s(ref, dtype):
    if dtype is None:
        return torch.zeros_like(ref)
    _, _, eps, tiny, _ = _FMT[dtype]
    return eps * ref.abs().clamp_min(tiny)


class Ref(NamedTuple):
    value: torch.Tensor      # float64, holding values of the storage type (or exact fp64 sums for fp32 outputs)
    terms: torch.Tensor      # sum of |terms| per element
    n: int                   # fp32 operations per element
    extra: object = 0.0      # uncertainty inherited from rounded intermediates (module docstring)

    def bound(self, dtype):
        return ulp_s(self.value, dtype) + self.n * 2.0 ** -23 * self.terms + self.extra


def check(got, ref, dtype):
    """(every element inside `ref.bound`, largest |got - ref| / bound, number of elements outside).  A NaN or a shape
    mismatch is a miss; the ratio is what a failing test prints."""
    if got.shape != ref.value.shape:
        return False, float("inf"), got.numel()
    inside = (got.to(F64) - ref.value).abs_().div_(ref.bound(dtype))
    outside = int((~(inside <= 1.0)).sum())
    return outside == 0, float(inside.max()), outside


def accept(got, ref, dtype):
    """True when EVERY element of `got` is inside `ref.bound`: the acceptance rule of the module docstring."""
    return check(got, ref, dtype)[0]


def through_fp32(ref, dtype):
    """The reference's value as a kernel that keeps exact fp32 sums would store it: float64 -> float32 -> storage."""
    return ref.value.to(torch.float32).to(dtype)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def grid(shape, g, dtype, lim=8):
    """activations on a coarse grid, integers in [-lim, lim] / 4: equal values (ties, exact 0, exact 6) are frequent"""
    return torch.randint(-lim, lim + 1, shape, generator=g, dtype=torch.int8).to(dtype).div_(4.0)   # exact


def grads(shape, g, dtype):
    return torch.randn(shape, generator=g).to(dtype)


def f64(t):
    return t.to(F64)


# ---- geometry -------------------------------------------------------------------------------------------------------
def same_geometry(size, k, stride):
    """TF 'SAME': (output size, pad before).  3x3 / stride 2 pads 0 before an even size and 1 before an odd one."""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2


def _first(mask, last=False):
    """Of the True entries along the last axis keep the first (or the last) one."""
    m = mask.flip(-1) if last else mask
    keep = m & (m.cumsum(-1, dtype=torch.int16) == 1)
    return keep.flip(-1) if last else keep


def _windows(t, f):
    """[N, H, W, C] -> [N, H/f, W/f, C, f*f], window positions in row-major order (dy * f + dx)."""
    N, H, W, C = t.shape
    return t.reshape(N, H // f, f, W // f, f, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // f, W // f, C, f * f)


def _unwindows(w, f):
    N, Hc, Wc, C, _ = w.shape
    return w.reshape(N, Hc, Wc, C, f, f).permute(0, 1, 4, 2, 5, 3).reshape(N, Hc * f, Wc * f, C)


def sumpool(t, f):
    return t if f == 1 else _windows(t, f).sum(-1)


def maxpool_exact(t, f):
    return t if f == 1 else _windows(t, f).amax(-1)


def up(t, f):
    """nearest-neighbour upsample by f"""
    return t if f == 1 else t.repeat_interleave(f, 1).repeat_interleave(f, 2)


def window_argmax_onehot(t, f, pick="first"):
    """[N, H, W, C] one-hot of the first (last) maximum of every non-overlapping f x f window, row-major."""
    if f == 1:
        return torch.ones_like(t, dtype=torch.bool)
    w = _windows(t, f)
    return _unwindows(_first(w == w.amax(-1, keepdim=True), last=(pick == "last")), f)


# ---- max-pool, any k / stride / top-left pad, padded taps at -inf ---------------------------------------------------
def _padded(x, k, stride, pt, pl, Ho, Wo, fill):
    N, H, W, C = x.shape
    Hp, Wp = max((Ho - 1) * stride + k, pt + H), max((Wo - 1) * stride + k, pl + W)
    xp = torch.full((N, Hp, Wp, C), fill, dtype=x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp


def _tap(xp, r, s, stride, Ho, Wo):
    return xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]


def maxpool_fwd(x, k, stride, pt, pl, Ho, Wo):
    xp = _padded(x, k, stride, pt, pl, Ho, Wo, float("-inf"))
    out = torch.full((x.shape[0], Ho, Wo, x.shape[3]), float("-inf"), dtype=x.dtype)
    for r in range(k):
        for s in range(k):
            out = torch.maximum(out, _tap(xp, r, s, stride, Ho, Wo))
    return out


def maxpool_argmax(x, k, stride, pt, pl, Ho, Wo, pick="first"):
    """per window the tap index r * k + s of its first (last) maximum among the taps inside the image"""
    xp = _padded(x, k, stride, pt, pl, Ho, Wo, float("-inf"))
    best = torch.full((x.shape[0], Ho, Wo, x.shape[3]), float("-inf"), dtype=x.dtype)
    arg = torch.full(best.shape, -1, dtype=torch.int16)
    for r in range(k):
        for s in range(k):
            v = _tap(xp, r, s, stride, Ho, Wo)
            take = (v > best) if pick == "first" else ((v >= best) & (v > float("-inf")))
            best = torch.where(take, v, best)
            arg = torch.where(take, torch.tensor(r * k + s, dtype=torch.int16), arg)
    return arg


def maxpool_bwd(x, dy, k, stride, pt, pl, dtype, dx0=None, pick="first"):
    """dx = rs(dx0 + sum over the windows whose first maximum this pixel is of dy)."""
    N, H, W, C = x.shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    arg = maxpool_argmax(x, k, stride, pt, pl, Ho, Wo, pick)
    g = _padded(torch.zeros_like(x), k, stride, pt, pl, Ho, Wo, 0.0)
    a = torch.zeros_like(g)
    for r in range(k):
        for s in range(k):
            hit = arg == r * k + s
            _tap(g, r, s, stride, Ho, Wo).add_(torch.where(hit, dy, torch.zeros_like(dy)))
            _tap(a, r, s, stride, Ho, Wo).add_(torch.where(hit, dy.abs(), torch.zeros_like(dy)))
    g, a = g[:, pt:pt + H, pl:pl + W], a[:, pt:pt + H, pl:pl + W]
    if dx0 is not None:
        g, a = g + dx0, a + dx0.abs()
    return Ref(round_storage(g, dtype), a, (-(-k // stride)) ** 2 + 1)


# ---- FPN top-down -----------------------------------------------------------------------------------------------------
def act_fwd(v, act):
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "relu6":
        return v.clamp(0.0, 6.0)
    assert act in (None, "none")
    return v


def act_mask(z, act, lo_inclusive=False, hi_inclusive=False):
    """relu: z > 0; relu6: 0 < z < 6; none: 1 (the *_inclusive switches build deliberately wrong references)"""
    if act in (None, "none"):
        return torch.ones_like(z)
    m = (z >= 0) if lo_inclusive else (z > 0)
    if act == "relu6":
        m = m & ((z <= 6) if hi_inclusive else (z < 6))
    return m.to(z.dtype)


def topdown_fwd(ins, act, dtype):
    """out[L-1] = in[L-1]; out[l] = rs(act(in[l] + up2(out[l+1])))"""
    L = len(ins)
    outs = [None] * L
    outs[L - 1] = Ref(ins[L - 1], ins[L - 1].abs(), 1)
    for l in range(L - 2, -1, -1):
        c = outs[l + 1]
        u = up(c.value, 2)
        extra = up(ulp_s(c.value, dtype), 2) if l + 1 < L - 1 else 0.0
        outs[l] = Ref(round_storage(act_fwd(ins[l] + u, act), dtype), ins[l].abs() + u.abs(), 2, extra)
    return outs


def topdown_bwd(douts, outs, acts, dtype, lo_inclusive=False, hi_inclusive=False):
    """din[l] = rs((dout[l] + sum2x2(din[l-1])) * mask(out[l])), finest level first; the finer din in its rounded form.
    outs[l] None or acts[l] none: no gate."""
    dins = []
    for l, d in enumerate(douts):
        m = torch.ones_like(d) if outs[l] is None else act_mask(outs[l], acts[l], lo_inclusive, hi_inclusive)
        if l == 0:
            dins.append(Ref(round_storage(d * m, dtype), d.abs() * m, 1))
            continue
        f = dins[l - 1]
        s = d + sumpool(f.value, 2)
        dins.append(Ref(round_storage(s * m, dtype), (d.abs() + sumpool(f.value.abs(), 2)) * m, 5,
                        sumpool(ulp_s(f.value, dtype), 2) * m))
    return dins


# ---- BalanceFeatures --------------------------------------------------------------------------------------------------
def balance_fwd(ins, mid, dtype):
    """avg = rs(mean over levels of {max-pooled finer, the middle, upsampled coarser}); out[l] = rs(in[l] + avg resized
    back: upsampled for finer levels, max-pooled for coarser ones).  Returns (avg, [out])."""
    L = len(ins)
    rs = [maxpool_exact(t, 1 << (mid - l)) if l <= mid else up(t, 1 << (l - mid)) for l, t in enumerate(ins)]
    avg = Ref(round_storage(sum(rs) / L, dtype), sum(r.abs() for r in rs) / L, L + 1)
    u = ulp_s(avg.value, dtype)
    outs = []
    for l, t in enumerate(ins):
        f = 1 << abs(l - mid)
        back, eu = (up(avg.value, f), up(u, f)) if l <= mid else (maxpool_exact(avg.value, f), maxpool_exact(u, f))
        outs.append(Ref(round_storage(t + back, dtype), t.abs() + back.abs(), 2, eu))
    return avg, outs


def balance_bwd(douts, ins, avg, mid, dtype, pick="first", drop_level=None, round_davg=True):
    """With avg and in as GIVEN tensors:
         davg   = rs(sum_{l<=mid} sumpool_f(dout_l) + sum_{l>mid} scatter(dout_l -> first maximum of avg in its f x f window))
         din_l  = rs(dout_l + (1/L) sumpool_f(davg))                                          l >= mid
         din_l  = rs(dout_l + (1/L) davg at the parent, where this pixel is the first maximum of in_l in its window)   l < mid
    Returns (davg, [din]).  pick / drop_level / round_davg build deliberately wrong references."""
    L = len(douts)
    s = torch.zeros_like(avg)
    a = torch.zeros_like(avg)
    n = 0
    for l, d in enumerate(douts):
        if l == drop_level:
            continue
        if l <= mid:
            f = 1 << (mid - l)
            s, a, n = s + sumpool(d, f), a + sumpool(d.abs(), f), n + f * f
        else:
            f = 1 << (l - mid)
            hot = window_argmax_onehot(avg, f, pick).to(F64)
            s, a, n = s + hot * up(d, f), a + hot * up(d.abs(), f), n + 1
    davg = Ref(round_storage(s, dtype) if round_davg else s, a, n)
    u = ulp_s(davg.value, dtype)
    dins = []
    for l, d in enumerate(douts):
        if l >= mid:
            f = 1 << (l - mid)
            dins.append(Ref(round_storage(d + sumpool(davg.value, f) / L, dtype),
                            d.abs() + sumpool(davg.value.abs(), f) / L, 1 + 2 * f * f, sumpool(u, f) / L))
        else:
            f = 1 << (mid - l)
            hot = window_argmax_onehot(ins[l], f, pick).to(F64)
            dins.append(Ref(round_storage(d + hot * up(davg.value, f) / L, dtype),
                            d.abs() + hot * up(davg.value.abs(), f) / L, 3, hot * up(u, f) / L))
    return davg, dins


# ---- stride-2 placement, the gate, the row sum --------------------------------------------------------------------------
def upsample_zero2x(x, Ho, Wo):
    """y[n, 2h, 2w] = x[n, h, w], zero elsewhere; Ho in {2H - 1, 2H}"""
    y = torch.zeros((x.shape[0], Ho, Wo, x.shape[3]), dtype=x.dtype)
    y[:, ::2, ::2] = x[:, :(Ho + 1) // 2, :(Wo + 1) // 2]
    return y


def scatter_add2x(x, y0, dtype):
    """y[n, 2h, 2w] = rs(y0 + x) there, y0 untouched elsewhere"""
    z = upsample_zero2x(x, y0.shape[1], y0.shape[2])
    v = y0.clone()
    v[:, ::2, ::2] = round_storage((y0 + z)[:, ::2, ::2], dtype)
    return Ref(v, y0.abs() + z.abs(), 2)


def depth_to_space2x(x):
    """y[n, 2i + a, 2j + b, c] = x[n, i, j, (2a + b) C + c]"""
    N, H, W, C4 = x.shape
    C = C4 // 4
    return x.reshape(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C)


def depth_to_space2x_add(x, y0, dtype):
    z = depth_to_space2x(x)
    return Ref(round_storage(y0 + z, dtype), y0.abs() + z.abs(), 2)


def reduce_rows(src, add):
    """dst[c] = add + sum_r src[r, c]: an fp32 output, so the bound is n 2^-23 sum|terms| alone"""
    return src.sum(0) + add, src.abs().sum(0) + abs(add), src.shape[0] + 1
