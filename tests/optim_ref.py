"""Float64 reference of the optimizer kernels (csrc/rn_optim.hip), the arena layout they walk, the inputs of their tests
and the rule that compares a kernel with the reference.

The reference
-------------
Written from the training step of the project this one restates (executor.py:401-441, optimizers/builder.py:45-54) on
float64 tensors; a tensor is a segment of a flat arena, `Layout.elem` lists the arena indices of all tensor elements
("packed" order) and `Layout.seg` the tensor of each.
  stage 1   t = g * unscale + wdc * w on the weight-decayed tensors, t = g * unscale on the others    (executor.py:417-430:
            LossScaleOptimizer.get_unscaled_gradients, the gradient of alpha * l2_loss(w) / R)
  stage 2   f_i = c / max(||t_i||, c)             tf.clip_by_norm                                      (executor.py:403)
            gn = sqrt(sum_i (f_i ||t_i||)^2), F = c / max(gn, c)      tf.clip_by_global_norm over the CLIPPED tensors
            l2 = alpha / 2 * sum over the decayed tensors of ||w||^2                                   (executor.py:296-299)
  stage 3   g' = f_i F t, or the correction (f_i F - 1) t
  stage 4   v' = m v - lr g ; w' = w + v'   or, nesterov, w' = w + m v' - lr g                         (builder.py:45, Keras SGD)
            e' = e - (1 - d)(e - w')                                                                   (builder.py:51-54)
Every scalar the kernel receives as a C float (lr, momentum, ema_decay, wd_coeff, wd_alpha, unscale, clip) enters as its
float32 value (`f32`), and 1 - d is the float32 difference, as the kernel forms it.

About "only a per-tensor factor fires": a tensor that tf.clip_by_norm clips has norm c afterwards, so the global norm of
the clipped tensors is at least c and exceeds it as soon as any other tensor is not zero.  With real gradients the global
factor therefore fires whenever a per-tensor factor does; the regime `only257` is "exactly one per-tensor factor differs
from 1, the one of tensor 257", and the global factor fires with it.

The acceptance rule (derived, not tuned)
----------------------------------------
u = 2^-24 is the unit roundoff of fp32.  The library is built with -ffp-contract=off: every product is rounded.
Element-wise fp32 expressions use `pyramid_ref.Ref` with dtype=None: |got - ref| <= n 2^-23 sum|terms| for n operations
(the rigorous bound is n u (1 + u)^n sum|terms|, half of it).  n per output:
  stage 1            3   (g * unscale, wdc * w, the add)
  v'                 3   (m v, lr g, the subtraction)
  w' plain           4   (v', the add)
  w' nesterov        7   (v', m v', lr g, the subtraction, the add)
  e'            n_w + 3  (e - w', the product with the float32 (1 - d), the subtraction)
Block sums.  A block is `chunk` elements over 256 threads.  A thread squares and adds at most k = chunk / 256 + 1
elements in fp32 (chunk / 256 from the 16-byte body and one from the scalar tail).  All terms are >= 0, the first add is
exact, so every square carries at most k roundings and the thread's sum has relative error below (1 + u)^k - 1 < k 2^-23.
From there everything is double: the wave, block, tensor and global sums are fewer than 2^12 additions on any path, a
relative 2^-41 that is carried as `EPS_D`.  With eps_sq = k 2^-23 + EPS_D the relative bounds follow line by line:
  tensor norm  (float)sqrt(sq)         eps_norm = eps_sq / 2 + u + EPS_D       (sqrt halves, the cast rounds once)
  factor       c / fmaxf(norm, c)      eps_f    = eps_norm + u                 (exactly 1 when it does not fire)
  clipped norm norm * f                eps_cn   = eps_norm + eps_f + u
  global norm  (float)sqrt(sum cn^2)   eps_gn   = eps_cn + u + EPS_D           (metrics[1])
  global factor c / fmaxf(gn, c)       eps_F    = eps_gn + u                   (metrics[2])
  gn * F                               eps_m0   = eps_gn + eps_F + u           (metrics[0])
  factor[t] *= F                       eps_ft   = eps_f + eps_F + u
  l2 metric    (float)(alpha/2 * sum)  eps_l2   = eps_sq + u + EPS_D           (metrics[3])
  clipped gradient element  t * factor : one more rounding on top of eps_ft relative to |t f|:
                                        Ref(value, |value|, n = 1, extra = eps_ft |value|)
  correction element  (factor - 1) * t : the subtraction and the product round once each (n = 2, terms |(f - 1) t|); the
                                        factor's own error is absolute: extra = eps_ft f |t|
(products of (1 + eps) are linearised; every eps here is below 2^-17, the quadratic terms are below EPS_D.)
Each stage is compared GIVEN the kernel's own output of the stage before it: the norms and factors are taken in float64
from the kernel's stage-1 tensor, the SGD reference reads the device G, w, v, e.  One stage's allowance never covers
another's error.  Copies (local_copy, untouched slots, a factor of exactly 1) and the 16-bit cast of the kernel's own fp32
weight are compared bit for bit.

Input margins: every tensor norm and the global norm of every input set lies farther than 1e-3 c from c (`margins`,
asserted in test_optim_ref_cpu.py), 500 times eps_gn, so float32 and float64 agree on which factors fire.
"""
from typing import NamedTuple

import numpy as np
import torch

from pyramid_ref import F64, Ref

U = 2.0 ** -24
EPS_D = 2.0 ** -41
SENTINEL = -1234.5     # what reserved / padding slots hold before a launch (exact in fp32)
SENTINEL16 = -3.5      # the same for the 16-bit arena (exact in bfloat16 and half)


def f32(x):
    """the value a C float parameter receives"""
    return float(np.float32(x))


def chunk():
    from retinanet import _C
    return int(_C.lib().rn_optim_chunk())


# ---- layout -----------------------------------------------------------------------------------------------------------
class Layout(NamedTuple):
    segs: np.ndarray          # the engine's _SEG_DTYPE records
    block_seg: np.ndarray     # int32, tensor of every block
    total: int                # floats in P / G / V / E
    total16: int              # elements in Pbf
    untouched: torch.Tensor   # arena indices no kernel may write: the reserved G[0:4], padding, the slack at the end
    untouched16: torch.Tensor
    elem: torch.Tensor        # arena index of every tensor element, tensor after tensor
    seg: torch.Tensor         # its tensor
    wd: torch.Tensor          # float64 0 / 1 per tensor element
    chunk: int

    @property
    def n_segs(self):
        return len(self.segs)

    @property
    def n_blocks(self):
        return len(self.block_seg)

    def rng(self, i):
        """(first arena index, one past the last) of tensor i"""
        o = int(self.segs["offset"][i])
        return o, o + int(self.segs["size"][i])

    def copies(self):
        """(fp32 arena offset, 16-bit arena offset, size) of every tensor with a 16-bit copy"""
        return [(int(s["offset"]), int(s["bf"]), int(s["size"])) for s in self.segs if s["bf"] >= 0]


def build_layout(sizes, wd, has16, chunk_, skew=None, skew16=None):
    """The segment table the way TrainEngine._alloc_params lays the arenas out: the first fp32 offset is 4 (G[0:4] are
    reserved), every fp32 offset is rounded up to 4, a separate 16-bit counter is rounded up to 8 after every tensor,
    bf16_offset = -1 where there is no 16-bit copy.  skew / skew16 (layout B only): floats inserted in front of tensor i
    AFTER the rounding, which is how a tensor gets an offset the engine never produces.  Four floats (eight 16-bit
    elements) of slack follow the last tensor, so that a tail loop one element too long stays inside the arena."""
    from retinanet.model.train_engine import _SEG_DTYPE
    assert _SEG_DTYPE.itemsize == 40, "struct OptSeg"
    n = len(sizes)
    skew = skew or [0] * n
    skew16 = skew16 or [0] * n
    segs = np.zeros((n,), dtype=_SEG_DTYPE)
    block_seg, off, bf_off, nblk = [], 4, 0, 0
    for i, size in enumerate(sizes):
        off += skew[i]
        bfo = -1
        if has16[i]:
            bf_off += skew16[i]
            bfo = bf_off
            bf_off += size
        bf_off = (bf_off + 7) // 8 * 8
        nb = (size + chunk_ - 1) // chunk_
        segs[i] = (off, size, int(wd[i]), nblk, nb, 0, bfo)
        block_seg += [i] * nb
        off = (off + size + 3) // 4 * 4
        nblk += nb
    total, total16 = off + 4, bf_off + 8
    used = torch.zeros((total,), dtype=torch.bool)
    used16 = torch.zeros((total16,), dtype=torch.bool)
    for s in segs:
        used[int(s["offset"]):int(s["offset"] + s["size"])] = True
        if s["bf"] >= 0:
            used16[int(s["bf"]):int(s["bf"] + s["size"])] = True
    sz = torch.from_numpy(segs["size"].astype(np.int64))
    seg = torch.repeat_interleave(torch.arange(n), sz)
    start = torch.from_numpy(segs["offset"].astype(np.int64))
    first = torch.cumsum(sz, 0) - sz
    elem = start[seg] + (torch.arange(int(sz.sum())) - first[seg])
    assert int(used.sum()) == elem.numel() and bool(used[elem].all()), "tensors overlap"
    wde = torch.from_numpy(segs["wd"].astype(np.float64))[seg]
    return Layout(segs, np.asarray(block_seg, dtype=np.int32), total, total16, (~used).nonzero().flatten(),
                  (~used16).nonzero().flatten(), elem, seg, wde, chunk_)


ALONE = 257     # layout A: the tensor whose per-tensor factor fires alone
NAN_AT = 258    # layout A: a non-decayed tensor behind the first 256, where the NaN case puts its NaN
NINE = 260      # layout A: the 9-block tensor


def layout_a(chunk_):
    """Engine-like, 300 tensors: block-boundary sizes, tiny ones, the rest from a seeded integers(1, 700)."""
    rs = np.random.default_rng(20240)
    n = 300
    sizes = [int(x) for x in rs.integers(1, 700, n)]
    wd = [int(x) for x in rs.integers(0, 2, n)]
    has16 = [bool(w and rs.random() < 0.7) for w in wd]      # some decayed tensors have no 16-bit copy
    for i, s in zip((3, 17, 40, 90, 150), (chunk_, chunk_ + 1, chunk_ - 1, 3 * chunk_ + 5, 17 * chunk_ - 3)):
        sizes[i], wd[i], has16[i] = s, 1, True
    for i, s in zip(range(60, 67), (1, 2, 3, 4, 5, 6, 7)):
        sizes[i] = s
    has16[150] = False                                       # the largest tensor: decayed, no copy
    wd[10], has16[10] = 0, True                              # a non-decayed tensor with a copy
    wd[61], has16[61] = 1, True
    wd[64], has16[64] = 1, True
    sizes[NINE], wd[NINE], has16[NINE] = 9 * chunk_ + 2, 1, True    # > 8 blocks: the remainder of the unroll-8 loop
    sizes[ALONE], wd[ALONE], has16[ALONE] = 301, 1, True
    sizes[NAN_AT], wd[NAN_AT], has16[NAN_AT] = 33, 0, False
    return build_layout(sizes, wd, has16, chunk_)


B_MIXED = 4     # layout B: aligned fp32 offset, unaligned 16-bit offset


def layout_b(chunk_):
    """Offsets the engine never produces: fp32 offsets 1, 2, 3 mod 4 (a multi-block tensor among them), and one
    multi-block tensor with an aligned fp32 offset and an unaligned 16-bit offset (the second clause of `vec` in the SGD
    kernel); aligned tensors in between as the control."""
    sizes = [5, 2 * chunk_ + 3, 37, 300, chunk_ + 7, 9, 64, 4, 1]
    wd = [1, 1, 0, 1, 1, 0, 1, 0, 1]
    has16 = [True, True, False, True, True, True, True, False, True]
    skew = [1, 2, 3, 0, 0, 1, 0, 3, 2]
    skew16 = [0, 3, 0, 0, 2, 1, 0, 0, 5]
    lay = build_layout(sizes, wd, has16, chunk_, skew, skew16)
    assert lay.segs["offset"][B_MIXED] % 4 == 0 and lay.segs["bf"][B_MIXED] % 4 != 0
    assert lay.segs["offset"][1] % 4 != 0 and lay.segs["offset"][3] % 4 == 0 and lay.segs["bf"][3] % 4 == 0
    return lay


# ---- inputs -----------------------------------------------------------------------------------------------------------
ALPHA, REPLICAS = 1e-4, 4
# regime -> (clip, loss scale, norm of tensor ALONE or None).  Tensor norms are 0.2 .. 0.55 or 0.65 .. 1.0, the global norm
# of 300 of them is about 11 (layout A) and about 2 for the 9 tensors of layout B.
REGIMES = {"off": (0.0, 1.0, None), "none": (32.0, 1.0, None), "only257": (8.0, 1024.0, 12.0),
           "global": (1.5, 1.0, None), "both": (0.6, 1024.0, None)}


class Inputs(NamedTuple):
    w: torch.Tensor        # fp32 arenas (sentinel in every slot that is no tensor element)
    g: torch.Tensor        # the gradient as backward leaves it: times the loss scale
    clip: float
    unscale: float
    wdc: float
    alpha: float


def make_inputs(lay, regime, seed=0):
    """Gradients with a chosen norm per tensor (away from every clip the regimes use), weights ~ 0.05 N(0, 1)."""
    clip, scale, alone = REGIMES[regime]
    gen = torch.Generator().manual_seed(1000 + seed)
    n = lay.elem.numel()
    wp = torch.randn((n,), generator=gen, dtype=F64) * 0.05
    gp = torch.randn((n,), generator=gen, dtype=F64)
    r = torch.rand((lay.n_segs,), generator=gen, dtype=F64) * 0.7 + 0.2          # 0.2 .. 0.9
    r = torch.where(r > 0.55, r + 0.1, r)                                         # nothing in 0.55 .. 0.65
    if alone is not None and lay.n_segs > ALONE:
        r[ALONE] = alone
    sq = torch.zeros((lay.n_segs,), dtype=F64).index_add_(0, lay.seg, gp * gp)
    gp = gp * (r / sq.sqrt())[lay.seg] * scale
    w = torch.full((lay.total,), SENTINEL, dtype=torch.float32)
    g = torch.full((lay.total,), SENTINEL, dtype=torch.float32)
    w[lay.elem] = wp.float()
    g[lay.elem] = gp.float()
    return Inputs(w, g, f32(clip), f32(1.0 / scale), f32(ALPHA / REPLICAS), f32(ALPHA))


def two_ranks(lay):
    """two synthetic ranks over the same weights: the clip fires on the first ("both"), nothing fires on the second"""
    a, b = make_inputs(lay, "both", 0), make_inputs(lay, "none", 1)
    return [a, b._replace(w=a.w)]


def sgd_state(lay, seed=0):
    """(v, e) arenas for a given w: a live momentum and a moving average near the weights"""
    gen = torch.Generator().manual_seed(2000 + seed)
    n = lay.elem.numel()
    v = torch.full((lay.total,), SENTINEL, dtype=torch.float32)
    d = torch.full((lay.total,), SENTINEL, dtype=torch.float32)
    v[lay.elem] = torch.randn((n,), generator=gen) * 0.01
    d[lay.elem] = torch.randn((n,), generator=gen) * 0.01
    return v, d


# ---- reference ----------------------------------------------------------------------------------------------------------
class Eps(NamedTuple):
    sq: float
    norm: float
    f: float
    cn: float
    gn: float
    F: float
    m0: float
    ft: float
    l2: float


def eps(chunk_):
    """the relative bounds of the module docstring"""
    k = chunk_ // 256 + 1
    sq = k * 2.0 ** -23 + EPS_D
    norm = sq / 2 + U + EPS_D
    f = norm + U
    cn = norm + f + U
    gn = cn + U + EPS_D
    F = gn + U
    return Eps(sq, norm, f, cn, gn, F, gn + F + U, f + F + U, sq + U + EPS_D)


def pack(lay, arena):
    return arena.detach().cpu()[lay.elem].to(F64)


def stage1(lay, g, w, wdc, unscale):
    """t = g * unscale + wdc * w (decayed tensors), packed"""
    a = pack(lay, g) * unscale
    b = pack(lay, w) * wdc * lay.wd
    return Ref(a + b, a.abs() + b.abs(), 3)


class Clip(NamedTuple):
    norm: torch.Tensor      # ||t_i||
    f: torch.Tensor         # per-tensor factor
    F: float                # global factor
    gn: float               # global norm of the per-tensor clipped tensors
    metrics: list           # [gn F, gn, F, l2, fired, not finite]
    flags: tuple            # (fired or not finite, not finite)

    @property
    def factor(self):
        return self.f * self.F


def _seg_sum(lay, x):
    return torch.zeros((lay.n_segs,), dtype=F64).index_add_(0, lay.seg, x)


def clip_factors(lay, t, w, clip, alpha):
    """Stage 2 from a packed stage-1 tensor t (float64 values) and the arena w."""
    norm = _seg_sum(lay, t * t).sqrt()
    if clip > 0:
        f = clip / norm.clamp_min(clip)
        gn = float(((norm * f) ** 2).sum().sqrt())
        F = clip / max(gn, clip) if gn == gn else float("nan")
    else:
        f = torch.ones_like(norm)
        gn = float((norm ** 2).sum().sqrt())
        F = 1.0
    wp = pack(lay, w)
    l2 = 0.5 * alpha * float((wp * wp * lay.wd).sum())
    finite = bool(torch.isfinite(t).all())
    fired = bool((f != 1.0).any()) or F != 1.0
    return Clip(norm, f, F, gn, [gn * F, gn, F, l2, float(fired), float(not finite)],
                (float(fired or not finite), float(not finite)))


def margins(lay, inp):
    """smallest |norm - clip| / clip over the tensor norms and the global norm (inf with the clip off)"""
    t = stage1(lay, inp.g, inp.w, inp.wdc, inp.unscale).value
    c = clip_factors(lay, t, inp.w, inp.clip, inp.alpha)
    if inp.clip <= 0:
        return float("inf")
    return min(float((c.norm - inp.clip).abs().min()), abs(c.gn - inp.clip)) / inp.clip


def clipped(lay, t, c, e):
    """g' = factor * t, packed.  A factor of exactly 1 leaves no allowance: the element is a copy."""
    fac = c.factor[lay.seg]
    v = t * fac
    return Ref(v, v.abs(), 1, torch.where(fac == 1.0, torch.zeros_like(v), e.ft * v.abs()))


def correction(lay, t, c, e):
    """(factor - 1) * t, packed"""
    fac = c.factor[lay.seg]
    v = (fac - 1.0) * t
    return Ref(v, v.abs(), 2, torch.where(fac == 1.0, torch.zeros_like(v), e.ft * (fac * t).abs()))


def sgd(lay, w, g, v, ema, lr, m, d, nesterov):
    """One Keras SGD step and the moving average from the arenas as GIVEN (the kernel's own, float32 values).  Returns
    packed (w', v', e' or None)."""
    wp, gp, vp = pack(lay, w), pack(lay, g), pack(lay, v)
    mv, lg = m * vp, lr * gp
    v1 = Ref(mv - lg, mv.abs() + lg.abs(), 3)
    if nesterov:
        w1 = Ref(wp + m * v1.value - lg, wp.abs() + abs(m) * v1.terms + lg.abs(), 7)
    else:
        w1 = Ref(wp + v1.value, wp.abs() + v1.terms, 4)
    e1 = None
    if ema is not None:
        ep = pack(lay, ema)
        omd = float(np.float32(1.0) - np.float32(d))
        e1 = Ref(ep - omd * (ep - w1.value), ep.abs() + omd * (ep.abs() + w1.terms), w1.n + 3)
    return w1, v1, e1


def emu_sgd(lay, w, g, v, e, pbf, lr, m, d, nesterov, fault=None):
    """The SGD rule in NumPy float32, the header's op order with one rounding per operation: what the kernel must produce
    bit for bit (test_gpu_optimizer.py) and what the acceptance rule must accept (test_optim_ref_cpu.py).  CPU arenas in,
    new (w, v, e, 16-bit copy) out; `fault` plants one single fault the rule must reject."""
    F32 = np.float32
    w, g, v, e = w.numpy().copy(), g.numpy(), v.numpy().copy(), e.numpy().copy()
    pbf = pbf.clone()
    lr, m, d = F32(lr), F32(m), F32(d)
    for s in lay.segs:
        o, n = int(s["offset"]), int(s["size"])
        sl = slice(o, o + n)
        vel = m * v[sl] - lr * g[sl]
        old = v[sl] if fault == "nesterov_old_v" else vel
        nw = w[sl] + ((m * old - lr * g[sl]) if nesterov else vel)
        v[sl], w[sl] = vel, nw
        k = d if fault == "ema_swapped" else F32(1.0) - d
        e[sl] = e[sl] - k * (e[sl] - nw)
        if s["bf"] >= 0:
            x = torch.from_numpy(nw.copy())
            if fault == "copy_truncates":
                x = (x.view(torch.int32) & -65536).view(torch.float32)
            pbf[int(s["bf"]):int(s["bf"]) + n] = x.to(pbf.dtype)
    return torch.from_numpy(w), torch.from_numpy(v), torch.from_numpy(e), pbf


# ---- the rule -----------------------------------------------------------------------------------------------------------
def ratio(got, ref):
    """largest |got - ref| / bound over the packed elements; a bound of 0 asks for equality (ratio 0 or inf)"""
    diff = (got.to(F64) - ref.value).abs()
    b = ref.bound(None)
    q = torch.where(b > 0, diff / b.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff),
                                                                  torch.full_like(diff, float("inf"))))
    q = torch.where(torch.isnan(diff), torch.full_like(q, float("inf")), q)
    return float(q.max())


def rel(got, want, e):
    """|got - want| / (e |want|) for a scalar; exact agreement asked where want == 0"""
    got, want = float(got), float(want)
    if got != got:
        return float("inf")
    if want == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - want) / (e * abs(want))


def exact(a, b):
    return 0.0 if torch.equal(a, b) else float("inf")


def verify_stage1(lay, inp, t_dev):
    """the stage-1 arena (G after rn_optim_clip_prepare, or its local_copy) against t"""
    t_dev = t_dev.detach().cpu()
    return {"stage1": ratio(t_dev[lay.elem], stage1(lay, inp.g, inp.w, inp.wdc, inp.unscale)),
            "stage1 untouched": exact(t_dev[lay.untouched], inp.g[lay.untouched])}


def verify_clip(lay, inp, t_dev, g_dev, metrics_dev, flags_dev=None):
    """Stages 2 and 3 GIVEN the kernel's own stage-1 arena t_dev: the clipped gradient element-wise, metrics[0..5], the
    flags when given, the slots no kernel may write.  Returns name -> |got - ref| / bound; all must be <= 1."""
    e = eps(lay.chunk)
    t_dev, g_dev, m = t_dev.detach().cpu(), g_dev.detach().cpu(), metrics_dev.detach().cpu().tolist()
    t = t_dev[lay.elem].to(F64)
    c = clip_factors(lay, t, inp.w, inp.clip, inp.alpha)
    out = {"G": ratio(g_dev[lay.elem], clipped(lay, t, c, e)),
           "G untouched": exact(g_dev[lay.untouched], inp.g[lay.untouched]),
           "metrics[0]": rel(m[0], c.metrics[0], e.m0), "metrics[1]": rel(m[1], c.metrics[1], e.gn),
           "metrics[2]": rel(m[2], c.metrics[2], e.F) if c.F != 1.0 else (0.0 if m[2] == 1.0 else float("inf")),
           "metrics[3]": rel(m[3], c.metrics[3], e.l2),
           "metrics[4:6]": 0.0 if m[4:6] == c.metrics[4:6] else float("inf")}
    if flags_dev is not None:
        out["flags"] = 0.0 if tuple(flags_dev.detach().cpu().tolist()) == c.flags else float("inf")
    return out


def verify_correction(lay, inp, t_dev, corr_dev):
    e = eps(lay.chunk)
    t = t_dev.detach().cpu()[lay.elem].to(F64)
    c = clip_factors(lay, t, inp.w, inp.clip, inp.alpha)
    return {"correction": ratio(corr_dev.detach().cpu()[lay.elem], correction(lay, t, c, e))}


def verify_identity(lay, inps, t_devs, summed_dev):
    """sum_r t_r + sum_r correction_r == sum_r f_r t_r, the left side added in fp32 as ((t_0 + t_1) + (c_0 + c_1)): every
    correction brings its 2 operations and its factor's allowance, the three additions one rounding each."""
    e = eps(lay.chunk)
    val = terms = extra = 0.0
    for inp, t_dev in zip(inps, t_devs):
        t = t_dev.detach().cpu()[lay.elem].to(F64)
        c = clip_factors(lay, t, inp.w, inp.clip, inp.alpha)
        cor = correction(lay, t, c, e)
        val = val + t * c.factor[lay.seg]
        terms = terms + t.abs() + cor.terms
        extra = extra + cor.extra
    return {"identity": ratio(summed_dev.detach().cpu()[lay.elem], Ref(val, terms, 2 + 3, extra))}


def verify_sgd(lay, before, after, g_dev, lr, m, d, nesterov, pbf_before=None, pbf_after=None):
    """One SGD launch: before / after = (w, v, e or None) arenas, all as the device held them.  The 16-bit copy is the
    cast of the kernel's OWN new weight, bit for bit; everything that is no tensor element keeps what it held."""
    w1, v1, e1 = sgd(lay, before[0], g_dev, before[1], before[2], lr, m, d, nesterov)
    out = {}
    for name, ref, b, a in (("w", w1, before[0], after[0]), ("v", v1, before[1], after[1]), ("ema", e1, before[2], after[2])):
        if ref is None:
            continue
        b, a = b.detach().cpu(), a.detach().cpu()
        out[name] = ratio(a[lay.elem], ref)
        out[name + " untouched"] = exact(a[lay.untouched], b[lay.untouched])
    if pbf_after is not None:
        pa, pb, wa = pbf_after.detach().cpu(), pbf_before.detach().cpu(), after[0].detach().cpu()
        ok = all(torch.equal(pa[bo:bo + n], wa[o:o + n].to(pa.dtype)) for o, bo, n in lay.copies())
        out["16-bit copy"] = 0.0 if ok else float("inf")
        out["16-bit untouched"] = exact(pa[lay.untouched16], pb[lay.untouched16])
    return out


def worst(ratios):
    return max(ratios.values())
