"""Float64 reference of the accumulate stage of a gradient-accumulation micro-step (rn_optim_clip_apply_accumulate,
csrc/rn_optim.hip), its inputs, a float32 emulation of the header's op order and the rule that compares a kernel with both.
Built on optim_ref.py: the layouts, `make_inputs`, `stage1`, `clip_factors`, `eps`, `ratio`.

The reference
-------------
training.gradient_accumulation_steps = N takes the reference's replicas (executor.py:401-437) one after another on one
device.  Micro-step i has its own stage-1 tensor t_i (its gradient, unscaled, plus its share of the decay gradient) and its
own clip factors f_i = per-tensor factor times global factor, from t_i alone (optim_ref stages 1 and 2).  Stage 3 is
    first:      A = f_0 t_0                  (whatever A held is gone: it is not read)
    otherwise:  A = A + f_i t_i
and the two flag slots A[0] = max over the micro-steps of "a factor != 1 or the norm is not finite", A[1] = max of "not
finite"; A[2:4], padding and the slack behind the last tensor are never written; the gradient arena is not written.

The acceptance rule (derived as in optim_ref's docstring, not tuned)
--------------------------------------------------------------------
Each element is compared GIVEN the kernel's own stage-1 tensor t_i (the gradient arena after the call) and its own previous
accumulator a.  The kernel's fp32 factor sits within eps_ft (relative) of the float64 factor f of that t_i; the product and
the sum round once each (-ffp-contract=off):
    f != 1           Ref(a + f t, |a| + |f t|, n = 2, extra = eps_ft |f t|)
    f != 1, first    Ref(f t, |f t|, n = 1, extra = eps_ft |f t|)      (no sum: optim_ref's clipped gradient element)
    f == 1           Ref(a + t, |a| + |t|, n = 1): the product 1 * t is exact, the factor carries no error
    f == 1, first    a bit-for-bit copy of t: bound 0
A bound cannot see an operation done MORE exactly than the header says (f t kept in double, the sum rounded once: a
contracted multiply-add), so the header's op order is also checked bit for bit: `emu_accumulate` in NumPy float32 from the
kernel's own fp32 factors, which a caller reads through the entry point itself — first != 0 on an arena of ones stores
factor * 1 ("A bits").  The flags are 0 / 1 values compared exactly; the slots nobody may write are compared bit for bit
(they may hold NaN).

Input margins: `micro_inputs` are three micro-steps over the same weights in optim_ref's regimes none / both / none: every
tensor norm and global norm of every micro-step lies farther than 1e-3 c from its clip threshold c (`optim_ref.margins`,
asserted in test_accum_ref_cpu.py), the per-tensor factors fire on the second micro-step and every factor is 1 on the others.
"""
import math

import numpy as np
import torch

import optim_ref as O
from pyramid_ref import F64, Ref

F32 = np.float32
REGIMES = ("none", "both", "none")


def micro_inputs(lay, regimes=REGIMES):
    """one optim_ref.Inputs per micro-step, all over the weights of the first (the weights do not change inside a step)"""
    inps = [O.make_inputs(lay, r, seed) for seed, r in enumerate(regimes)]
    return [x._replace(w=inps[0].w) for x in inps]


def fresh_accumulator(lay):
    """what the last optimizer step may have left behind: NaN in every tensor element and in the flag slots; the sentinel in
    A[2:4], the padding and the end slack"""
    a = torch.full((lay.total,), float("nan"), dtype=torch.float32)
    a[lay.untouched[2:]] = O.SENTINEL
    return a


# ---- reference --------------------------------------------------------------------------------------------------------------
def clip_from_norms(norm, clip, finite=True):
    """optim_ref.clip_factors from the tensor norms alone (float64 [tensors]) — for an arena whose element list is a sample
    (optim_rules_ref.engine_layout), where the caller sums the squares over the whole arena.  metrics[3] is not formed."""
    if clip > 0:
        f = clip / norm.clamp_min(clip)
        gn = float(((norm * f) ** 2).sum().sqrt())
        F = clip / max(gn, clip) if gn == gn else float("nan")
    else:
        f, gn, F = torch.ones_like(norm), float((norm ** 2).sum().sqrt()), 1.0
    fired = bool((f != 1.0).any()) or F != 1.0
    return O.Clip(norm, f, F, gn, [gn * F, gn, F, None, float(fired), float(not finite)],
                  (float(fired or not finite), float(not finite)))


def accumulated(lay, inp, t_dev, prev, first, c=None):
    """(Ref of the accumulator's tensor elements, packed; the float64 Clip of this micro-step) from the kernel's own
    stage-1 arena t_dev and its own previous accumulator prev.  c: the Clip of t_dev when lay.elem is only a sample."""
    e = O.eps(lay.chunk)
    t = O.pack(lay, t_dev)
    if c is None:
        c = O.clip_factors(lay, t, inp.w, inp.clip, inp.alpha)
    fac = c.factor[lay.seg]
    p = fac * t
    one = fac == 1.0
    zero = torch.zeros_like(p)
    extra = torch.where(one, zero, e.ft * p.abs())
    if first:
        return Ref(p, p.abs(), torch.where(one, zero, zero + 1.0), extra), c
    a = O.pack(lay, prev)
    return Ref(a + p, a.abs() + p.abs(), torch.where(one, zero + 1.0, zero + 2.0), extra), c


def flags_after(prev, c, first):
    """A[0:2] after a micro-step whose float64 clip is c"""
    if first:
        return c.flags
    p = prev.detach().cpu()[0:2].tolist()
    return (max(p[0], c.flags[0]), max(p[1], c.flags[1]))


def same_bits(a, b):
    return 0.0 if torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) else float("inf")


def verify(lay, inp, t_dev, prev, got, first, factors=None, metrics=None, c=None):
    """One accumulate launch: prev / got = the accumulator before / after, t_dev = the gradient arena after the call, all as
    the device held them.  factors (optional): the kernel's own fp32 factor per arena element, metrics its metrics — then
    the header's op order is checked bit for bit as well.  c: see `accumulated` (inp may then be None).
    Returns name -> |got - ref| / bound; all must be <= 1."""
    t_dev, prev, got = t_dev.detach().cpu(), prev.detach().cpu(), got.detach().cpu()
    ref, c = accumulated(lay, inp, t_dev, prev, first, c)
    keep = lay.untouched[2:]
    out = {"A": O.ratio(got[lay.elem], ref),
           "A untouched": same_bits(got[keep], prev[keep]),
           "A flags": 0.0 if tuple(got[0:2].tolist()) == tuple(flags_after(prev, c, first)) else float("inf")}
    if factors is not None:
        want = emu_accumulate(lay, t_dev, factors.detach().cpu(), metrics.detach().cpu().tolist(), prev, first)
        out["A bits"] = same_bits(got[lay.elem], want[lay.elem])
        out["A flag bits"] = same_bits(got[0:2], want[0:2])
    return out


# ---- float32 emulation ------------------------------------------------------------------------------------------------------
def emu_stage1(lay, inp):
    """the stage-1 arena in float32: g * unscale, + wdc * w on the decayed tensors"""
    g, w = inp.g.numpy().copy(), inp.w.numpy()
    for s in lay.segs:
        o, n = int(s["offset"]), int(s["size"])
        t = g[o:o + n] * F32(inp.unscale)
        if s["wd"]:
            t = t + F32(inp.wdc) * w[o:o + n]
        g[o:o + n] = t
    return torch.from_numpy(g)


def emu_factors(lay, t_arena, inp):
    """(fp32 factor per arena element — the sentinel outside the tensors —, metrics[6]) the way stage 2 forms them; the
    block sums are fp32 squares added in double (the kernel adds up to chunk / 256 + 1 of them in fp32 first: inside eps_sq)"""
    t, clip = t_arena.numpy(), F32(inp.clip)
    factor = np.ones((lay.n_segs,), dtype=F32)
    tot, fired = 0.0, False
    for i, s in enumerate(lay.segs):
        o, n = int(s["offset"]), int(s["size"])
        with np.errstate(all="ignore"):
            norm = F32(math.sqrt(float((t[o:o + n] * t[o:o + n]).astype(np.float64).sum())))
            f = clip / (norm if norm > clip else clip) if clip > 0 else F32(1.0)     # fmaxf drops a NaN
            cn = norm * f
        factor[i] = f
        fired |= bool(f != 1.0)
        tot += float(cn) * float(cn)
    with np.errstate(all="ignore"):
        gn = F32(math.sqrt(tot)) if tot == tot else F32(np.nan)
        Fg = clip / (gn if gn > clip else clip) if clip > 0 else F32(1.0)
        factor = factor * Fg
        finite = bool(np.isfinite(gn))
        metrics = [float(gn * Fg), float(gn), float(Fg), 0.0, float(fired or Fg != 1.0), float(not finite)]
    arena = np.full((lay.total,), O.SENTINEL, dtype=F32)
    arena[lay.elem.numpy()] = factor[lay.seg.numpy()]
    return torch.from_numpy(arena), metrics


def emu_accumulate(lay, t_arena, factors, metrics, accum, first, fault=None):
    """The accumulate stage in NumPy float32, the header's op order with one rounding per operation: what the kernel must
    produce bit for bit GIVEN its factors.  CPU arenas in, the new accumulator out.  `fault` plants one single fault:
      first_ignored     the stale accumulator is added although first != 0
      flag_overwritten  A[1] = metrics[5] instead of the maximum with what it held
      double_product    f t formed and added in double, rounded once (what a contracted multiply-add does)
    (the fourth fault of test_accum_ref_cpu.py, stale factors, is a caller handing in the factors of another micro-step)"""
    t, f, a = t_arena.numpy(), factors.numpy(), accum.numpy().copy()
    el = lay.elem.numpy()
    use_prev = (not first) or fault == "first_ignored"
    with np.errstate(all="ignore"):
        p = f[el] * t[el]
        if fault == "double_product" and use_prev:
            new = (a[el].astype(np.float64) + f[el].astype(np.float64) * t[el].astype(np.float64)).astype(F32)
        else:
            new = a[el] + p if use_prev else p
    fired = F32(1.0 if (metrics[4] != 0.0 or metrics[5] != 0.0) else 0.0)
    bad = F32(metrics[5])
    f0 = fired if first else max(a[0], fired)
    f1 = bad if (first or fault == "flag_overwritten") else max(a[1], bad)
    a[el] = new
    a[0], a[1] = f0, f1
    return torch.from_numpy(a)
