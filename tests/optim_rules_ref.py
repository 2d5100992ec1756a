"""Float64 reference of rn_optim_step (SGD, Adam, RMSprop, Adagrad of Keras optimizer_v2; the contract is the comment
above rn_optim_step in include/rnet_hip.h), the inputs of its tests and the rule that compares the kernel with the reference.
The arenas and their layout are optim_ref's (`Layout`, `pack`, sentinels); nothing there is changed.

The reference
-------------
One function, `step`, evaluates the header's lines on float64 tensors, in the header's order:
  adam      m' = m + (g - m) c1;  v' = v + (g g - v) c2;  [vhat' = max(vhat, v')];  w' = w - (lr m') / (sqrt(d) + eps)
  rmsprop   rms' = rms + (g g - rms) c1;  [mg' = mg + (g - mg) c1;  d = rms' - mg' mg'];
            momentum:  mom' = momentum mom + (lr g) / sqrt(d + eps);  w' = w - mom'
            plain:     w' = w - (lr g) / (sqrt(d) + eps)
  adagrad   acc' = acc + g g;  w' = w - (lr g) / (sqrt(acc') + eps)
  sgd       v' = momentum v - lr g;  w' = w + v'   or, nesterov,  w' = w + (momentum v' - lr g)
  all       e' = e - omd (e - w')
Every scalar the kernel receives as a C float enters as its float32 value; c1 = 1 - beta1 (or 1 - rho), c2 = 1 - beta2 and
omd = 1 - ema_decay are the float32 differences, as the kernel forms them (`f32_consts=False` takes the exact differences
instead: the form in which the reference is compared with torch.optim).  For Adam `lr` is alpha_t, which the host forms.

The acceptance rule (derived, not tuned)
----------------------------------------
u = 2^-24 is the unit roundoff of fp32.  The library is built with -ffp-contract=off and correctly rounded divide and
root, so every product, sum, root and quotient is ONE rounding: fl(x) = x (1 + d), |d| <= u (a result below the smallest
normal is off by at most 2^-150 instead; `TINY` = 2^-149 is added per operation and never matters at the magnitudes
used).  Each quantity is carried as a pair (value, allowance): the float64 value of the formula on the kernel's OWN
inputs — the device w, g, slots and ema before the step, which are float32 numbers and enter exactly — and an absolute
bound `a` on |kernel's value - value|.  An operation on operands (x, ax), (y, ay) whose exact result on the reference
values is r gives
  inherited   x +- y : ax + ay          x y : |x| ay + |y| ax + ax ay          max(x, y) : max(ax, ay)
              sqrt x : ax / (sqrt x + sqrt(x - ax)) for x > ax  (= sqrt x - sqrt(x - ax), the worst x' in reach: the root is
                       concave), sqrt(x + ax) for x <= ax (the kernel's operand is >= 0 or its root is NaN), 0 for ax = 0
              x / y  : (ax + |r| ay) / (|y| - ay)              (needs |y| > ay; an element where it fails is a miss)
  allowance   a = inherited + u (|r| + inherited) + TINY       (the rounding acts on the kernel's operand values)
That is first-order propagation through the stated op order with the second-order terms kept, so nothing is linearised
away; one u per operation, the root and the quotient counted as one each.  An output is accepted when
|got - value| <= allowance on every element.  No allowance is shared between outputs: m', v', vhat', w', e' are each
compared given the inputs, and the allowance of w' contains those of the slots it reads because the kernel reads its own.
Copies are compared bit for bit: a slot the rule does not use, every arena slot that is no tensor element, all arrays
of a skipped step, and the 16-bit copy, which must be the cast of the kernel's own new fp32 weight.

Input margins.  `centered` subtracts mg'^2 from rms': the inputs are redrawn every step and start from zero slots, which
keeps the initial state's weight in both averages, so d = rms' - mg'^2 stays a sizeable fraction of rms'
(test_optim_rules_cpu.py asserts d > 1e-3 rms' in float64 wherever rms' > 0; an element whose gradient has been exactly
zero so far has rms' = mg' = d = 0 exactly, in fp32 as in float64).
"""
from typing import NamedTuple

import numpy as np
import torch

import optim_ref as O
from pyramid_ref import F64, Ref

U = 2.0 ** -24
TINY = 2.0 ** -149
ADAM, RMSPROP, ADAGRAD, SGD = 1, 2, 3, 4
AMSGRAD, CENTERED, MOMENTUM, NESTEROV = 1, 2, 4, 8
F32 = np.float32


class Rule(NamedTuple):
    """rn_optim_rule with the values the C floats receive"""
    rule: int
    flags: int = 0
    lr: float = O.f32(0.01)
    beta1: float = O.f32(0.9)
    beta2: float = O.f32(0.999)
    rho: float = O.f32(0.9)
    momentum: float = O.f32(0.0)
    epsilon: float = O.f32(1e-7)
    ema_decay: float = O.f32(0.0)

    @property
    def uses(self):
        """(slot1 used, slot2 used)"""
        return (self.rule == ADAM or bool(self.flags & MOMENTUM), bool(self.flags & (AMSGRAD | CENTERED)))


MODES = {"adam": (ADAM, 0), "adam+amsgrad": (ADAM, AMSGRAD), "rmsprop": (RMSPROP, 0), "rmsprop+momentum": (RMSPROP, MOMENTUM),
         "rmsprop+centered": (RMSPROP, CENTERED), "rmsprop+centered+momentum": (RMSPROP, CENTERED | MOMENTUM),
         "adagrad": (ADAGRAD, 0), "sgd": (SGD, 0), "sgd+nesterov": (SGD, NESTEROV)}
BETA1, BETA2, RHO, MOM, EPS, LR, DECAY, ACC0 = 0.9, 0.999, 0.9, 0.9, 1e-7, 0.01, 0.9998, 0.1


def adam_alpha(lr, beta1, beta2, t):
    """alpha_t in float64; t = iterations + 1"""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


def mode_rule(mode, t=1, ema=True, lr=LR):
    """the rule of `mode` at step t (1-based), hyper-parameters of Keras' defaults with momentum 0.9 where the mode has one"""
    rule, flags = MODES[mode]
    step = adam_alpha(lr, BETA1, BETA2, t) if rule == ADAM else lr
    return Rule(rule, flags, O.f32(step), O.f32(BETA1), O.f32(BETA2), O.f32(RHO), O.f32(MOM if flags & MOMENTUM or rule == SGD else 0.0),
                O.f32(EPS), O.f32(DECAY if ema else 0.0))


def slot_init(mode):
    return ACC0 if MODES[mode][0] == ADAGRAD else 0.0


# ---- (value, allowance) arithmetic -------------------------------------------------------------------------------------
class Val:
    __slots__ = ("v", "a")

    def __init__(self, v, a=None):
        self.v = v
        self.a = torch.zeros_like(v) if a is None else a

    @staticmethod
    def _op(r, inherited):
        return Val(r, inherited + U * (r.abs() + inherited) + TINY)

    def __add__(self, o):
        return Val._op(self.v + o.v, self.a + o.a)

    def __sub__(self, o):
        return Val._op(self.v - o.v, self.a + o.a)

    def __mul__(self, o):
        if not isinstance(o, Val):          # an exact scalar
            return Val._op(self.v * o, abs(o) * self.a)
        return Val._op(self.v * o.v, self.v.abs() * o.a + o.v.abs() * self.a + self.a * o.a)

    __rmul__ = __mul__

    def add_scalar(self, c):
        return Val._op(self.v + c, self.a)

    def sqrt(self):
        r = self.v.sqrt()
        lo = (self.v - self.a).clamp_min(0.0).sqrt()
        inh = torch.where(self.v > self.a, self.a / (r + lo).clamp_min(1e-300), (self.v + self.a).sqrt())
        inh = torch.where(self.a > 0, inh, torch.zeros_like(r))
        return Val._op(r, inh)

    def __truediv__(self, o):
        r = self.v / o.v
        room = o.v.abs() - o.a
        # no room: the allowance is NaN, which `optim_ref.ratio` counts as a miss unless the element agrees exactly
        inh = torch.where(room > 0, (self.a + r.abs() * o.a) / room.clamp_min(1e-300), torch.full_like(r, float("nan")))
        inh = torch.where((self.a == 0) & (o.a == 0), torch.zeros_like(r), inh)
        return Val._op(r, inh)

    def maximum(self, o):
        return Val(torch.maximum(self.v, o.v), torch.maximum(self.a, o.a))       # exact: no rounding

    def ref(self):
        return Ref(self.v, torch.zeros_like(self.v), 0, self.a)


def _consts(r, f32_consts):
    b = r.beta1 if r.rule == ADAM else r.rho
    if f32_consts:
        return float(F32(1.0) - F32(b)), float(F32(1.0) - F32(r.beta2)), float(F32(1.0) - F32(r.ema_decay))
    return 1.0 - b, 1.0 - r.beta2, 1.0 - r.ema_decay


def step(r, w, g, s0, s1=None, s2=None, ema=None, f32_consts=True):
    """One step on float64 tensors of any (common) shape.  Returns {"w", "s0", "s1", "s2", "ema"} -> Val, only the arrays
    the rule writes.  `.v` is the float64 reference, `.a` the allowance of the module docstring."""
    c1, c2, omd = _consts(r, f32_consts)
    w, g, s0 = Val(w), Val(g), Val(s0)
    out = {}
    if r.rule == ADAM:
        s1 = Val(s1)
        m = s0 + (g - s0) * c1
        v = s1 + (g * g - s1) * c2
        d = v
        if r.flags & AMSGRAD:
            d = Val(s2).maximum(v)
            out["s2"] = d
        out["s0"], out["s1"] = m, v
        nw = w - (m * r.lr) / d.sqrt().add_scalar(r.epsilon)
    elif r.rule == RMSPROP:
        ms = s0 + (g * g - s0) * c1
        out["s0"] = ms
        d = ms
        if r.flags & CENTERED:
            s2 = Val(s2)
            mg = s2 + (g - s2) * c1
            out["s2"] = mg
            d = ms - mg * mg
        if r.flags & MOMENTUM:
            mom = Val(s1) * r.momentum + (g * r.lr) / d.add_scalar(r.epsilon).sqrt()
            out["s1"] = mom
            nw = w - mom
        else:
            nw = w - (g * r.lr) / d.sqrt().add_scalar(r.epsilon)
    elif r.rule == ADAGRAD:
        acc = s0 + g * g
        out["s0"] = acc
        nw = w - (g * r.lr) / acc.sqrt().add_scalar(r.epsilon)
    elif r.rule == SGD:
        vel = s0 * r.momentum - g * r.lr
        out["s0"] = vel
        nw = w + (vel * r.momentum - g * r.lr) if r.flags & NESTEROV else w + vel
    else:
        raise ValueError(r.rule)
    out["w"] = nw
    if ema is not None:
        e = Val(ema)
        out["ema"] = e - (e - nw) * omd
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def rule_layout(chunk_, skewed):
    """Tensor sizes at every boundary of the kernel's paths (one lane, the tail alone, one 16-byte group, group + tail, one
    sweep of the block, two sweeps + tail, a block less / exactly / more than one element, three blocks), mixed
    weight-decay flags, some tensors without a 16-bit copy.  skewed=False: the offsets the engine produces (the 16-byte
    path).  skewed=True: fp32 offsets 1, 2, 3 mod 4 and unaligned 16-bit offsets (the scalar loop), with aligned tensors in
    between, one of them with an aligned fp32 and an unaligned 16-bit offset."""
    sizes = [1, 3, 4, 5, 255, 1025, chunk_ - 1, chunk_, chunk_ + 1, 2 * chunk_ + 7]
    wd = [1, 0, 1, 1, 0, 1, 1, 0, 1, 1]
    has16 = [True, False, True, True, True, True, False, True, True, True]
    if not skewed:
        return O.build_layout(sizes, wd, has16, chunk_)
    skew = [1, 2, 0, 3, 0, 1, 0, 2, 0, 3]
    skew16 = [0, 0, 3, 0, 1, 0, 0, 0, 2, 5]
    lay = O.build_layout(sizes, wd, has16, chunk_, skew, skew16)
    off, bf = lay.segs["offset"], lay.segs["bf"]
    assert (off % 4 != 0).sum() >= 5 and off[9] % 4 != 0 and off[8] % 4 == 0 and bf[8] % 4 != 0
    assert off[4] % 4 == 0 and off[6] % 4 == 0
    return lay


def gradients(lay, seed):
    """arena of gradients: magnitudes 10^U(-6, 2) with random signs, one element in 16 exactly zero, 1e-6 and 1e2 present"""
    gen = torch.Generator().manual_seed(5000 + seed)
    n = lay.elem.numel()
    mag = torch.pow(10.0, torch.rand((n,), generator=gen, dtype=F64) * 8.0 - 6.0)
    sign = torch.where(torch.rand((n,), generator=gen) < 0.5, -1.0, 1.0).to(F64)
    gp = mag * sign
    gp[torch.rand((n,), generator=gen) < 1.0 / 16] = 0.0
    gp[-1], gp[-2], gp[-3] = 1e-6, -1e2, 0.0
    g = torch.full((lay.total,), O.SENTINEL, dtype=torch.float32)
    g[lay.elem] = gp.float()
    return g


def start_state(lay, mode, h16, seed=0):
    """{"w", "s0", "s1", "s2", "ema", "pbf"}: weights ~ 0.05 N(0, 1), slots at their initial values (what the engine starts
    from), a moving average near the weights; sentinels everywhere else.  s1 / s2 exist for every mode: a rule that does not
    use one must leave it alone."""
    gen = torch.Generator().manual_seed(6000 + seed)
    n = lay.elem.numel()
    st = {k: torch.full((lay.total,), O.SENTINEL, dtype=torch.float32) for k in ("w", "s0", "s1", "s2", "ema")}
    wp = (torch.randn((n,), generator=gen, dtype=F64) * 0.05).float()
    st["w"][lay.elem] = wp
    st["ema"][lay.elem] = wp + torch.randn((n,), generator=gen) * 0.01
    st["s0"][lay.elem] = slot_init(mode)
    st["s1"][lay.elem] = 0.0
    st["s2"][lay.elem] = 0.0
    st["pbf"] = torch.full((lay.total16,), O.SENTINEL16, dtype=h16)
    return st


def engine_layout(eng, sample=True):
    """optim_ref.Layout of a TrainEngine's own arenas, from the segment and block tables it gave the device"""
    from retinanet.model.train_engine import _SEG_DTYPE
    segs = eng.segs_dev.cpu().numpy().view(_SEG_DTYPE).copy()
    total, total16 = eng.P.numel(), eng.Pbf.numel()
    used = torch.zeros((total,), dtype=torch.bool)
    used16 = torch.zeros((total16,), dtype=torch.bool)
    for s in segs:
        used[int(s["offset"]):int(s["offset"] + s["size"])] = True
        if s["bf"] >= 0:
            used16[int(s["bf"]):int(s["bf"] + s["size"])] = True
    sz = torch.from_numpy(segs["size"].astype(np.int64))
    seg = torch.repeat_interleave(torch.arange(len(segs)), sz)
    start = torch.from_numpy(segs["offset"].astype(np.int64))
    first = torch.cumsum(sz, 0) - sz
    elem = start[seg] + (torch.arange(int(sz.sum())) - first[seg])
    assert int(used.sum()) == elem.numel()
    if sample:
        # the arithmetic is compared on every element of the tensors up to 4096 elements and, of the larger ones, on the
        # first and last 64 (the 16-byte body's first lanes, the scalar tail) and every 97th in between — each element is
        # computed alone, so a sample tells what all tell about t, the slots' roles and their initial values; `untouched`
        # and the 16-bit copies still cover the whole arenas
        pos = torch.arange(elem.numel()) - first[seg]
        keep = (sz[seg] <= 4096) | (pos < 64) | (pos >= sz[seg] - 64) | (pos % 97 == 0)
        elem, seg = elem[keep], seg[keep]
    wde = torch.from_numpy(segs["wd"].astype(np.float64))[seg]
    return O.Layout(segs, eng.block_seg_dev.cpu().numpy(), total, total16, (~used).nonzero().flatten(),
                    (~used16).nonzero().flatten(), elem, seg, wde, O.chunk())


def engine_rule(opt, step):
    """the Rule a TrainEngine hands the kernel at optimizer step `step` (0-based: optimizer.iterations before the step)"""
    rule = {"adam": ADAM, "rmsprop": RMSPROP, "adagrad": ADAGRAD, "sgd": SGD}[opt.name]
    flags = (AMSGRAD if opt.name == "adam" and opt.amsgrad else 0) | (NESTEROV if opt.name == "sgd" and opt.nesterov else 0)
    if opt.name == "rmsprop":
        flags = (CENTERED if opt.centered else 0) | (MOMENTUM if opt.momentum > 0 else 0)
    lr = opt.lr(step)
    if rule == ADAM:
        lr = adam_alpha(lr, opt.beta_1, opt.beta_2, step + 1)
    return Rule(rule, flags, O.f32(lr), O.f32(opt.beta_1), O.f32(opt.beta_2), O.f32(opt.rho), O.f32(opt.momentum),
                O.f32(opt.epsilon), O.f32(opt.ema_decay(step) if opt.use_moving_average else 0.0))


# ---- the rule -----------------------------------------------------------------------------------------------------------
def verify(lay, r, before, after, g, ema_on=True):
    """One launch: before / after = the state dicts as the device held them, g the gradient arena.  name -> |got - ref| /
    allowance (0 / inf for the bit-for-bit comparisons); all must be <= 1."""
    cpu = lambda t: t.detach().cpu()
    b = {k: cpu(v) for k, v in before.items() if v is not None}
    a = {k: cpu(v) for k, v in after.items() if v is not None}
    u1, u2 = r.uses
    ref = step(r, O.pack(lay, b["w"]), O.pack(lay, cpu(g)), O.pack(lay, b["s0"]), O.pack(lay, b["s1"]) if u1 else None,
               O.pack(lay, b["s2"]) if u2 else None, O.pack(lay, b["ema"]) if ema_on else None)
    out = {}
    for k in ("w", "s0", "s1", "s2", "ema"):
        if k not in a:
            continue
        if k in ref:
            out[k] = O.ratio(a[k][lay.elem], ref[k].ref())
            out[k + " untouched"] = O.exact(a[k][lay.untouched], b[k][lay.untouched])
        else:
            out[k + " unused"] = O.exact(a[k], b[k])
    if "pbf" in a:
        pa, wa = a["pbf"], a["w"]
        ok = all(torch.equal(pa[bo:bo + n], wa[o:o + n].to(pa.dtype)) for o, bo, n in lay.copies())
        out["16-bit copy"] = 0.0 if ok else float("inf")
        out["16-bit untouched"] = O.exact(pa[lay.untouched16], b["pbf"][lay.untouched16])
    return out


def centered_margin(lay, r, before, g):
    """smallest (rms' - mg'^2) / rms' over the elements with rms' > 0, in float64; inf when the rest is not exactly zero"""
    ref = step(r, O.pack(lay, before["w"]), O.pack(lay, g), O.pack(lay, before["s0"]),
               O.pack(lay, before["s1"]), O.pack(lay, before["s2"]))
    ms, mg = ref["s0"].v, ref["s2"].v
    d = ms - mg * mg
    live = ms > 0
    if not bool(((mg == 0) & (d == 0))[~live].all()):
        return float("-inf")
    return float((d[live] / ms[live]).min())
