"""References of the weighted FPN top-down fusion (FeatureFusion modes 'fast_attention' / 'fast_channel_attention',
reference model/layers/feature_fusion.py:41-56), in the style of pyramid_ref.py and act_ref.py.

The contract (include/rnet_hip.h, K7; rs = one rounding to the 16-bit storage type, one rounding per TF op):
    a_l = rs(max(w_l, 0))   a_u = rs(max(w_u, 0))   s = rs(rs(a_l + a_u) + rs(1e-4))
    lo = rs(rs(in[j] * a_l) / s)   up = rs(rs(up2(out[j+1]) * a_u) / s)   z = rs(lo + up)   out[j] = rs(act(z))
Backward: derivative of the unrounded function, one rounding where a tensor is stored; c_l = a_l / s, c_u = a_u / s:
    t_j = dout[j] + c_u^{j-1} sum2x2(g_{j-1})      g_j = rs(t_j act'(out[j]))      din[j] = rs(c_l^j g_j)
    din[L-1] = rs(t_{L-1})      Sl_j = sum g_j in[j]      Su_j = sum g_j up2(out[j+1])
    da_l = (Sl (s - a_l) - Su a_u) / s^2      da_u = (Su (s - a_u) - Sl a_l) / s^2      dw = da [w > 0]

Three kinds of reference live here:
  * the forward, op by op in explicit fp32 with `rs` after every op (`fuse`, `topdown_fwd`) — compared bit for bit; next
    to it torch's own arithmetic in the storage dtype (`fuse_torch`) and the one-rounding coefficient form
    (`fuse_coefficient_form`), which the contract is NOT;
  * the backward in float64 with the stated rounding points (`level_g`, `level_din`, `level_sums`, `weight_grads`,
    `topdown_bwd`); dtype None = no rounding, the exact formulas, for the comparison with autograd (`topdown_exact`);
  * the whole network: `FusedRefModel` / `FusedRefTrainer` override `fpn()` of oracle/model_ref.py with the contract at the
    same `_r` rounding points, and the trainer's `weight_decay()` adds the fusion weights (the reference decays every
    trainable variable of a non-conv layer whose name contains 'weight', executor.py:320-323).
"""
import torch
import torch.nn.functional as F

import act_ref as A
import pyramid_ref as R
from model_ref import RefModel, RefTrainer, _r

F32, F64 = torch.float32, torch.float64
# the five weight pairs of the sweeps: the initial value (s = 2 exactly), generic, a negative, both zero, one zero
WEIGHT_PAIRS = ((1.0, 1.0), (0.7, 1.9), (-0.3, 0.5), (0.0, 0.0), (1.3, 0.0))


def var_names(level):
    """(lower, upper) variable names of the fusion that joins P_{level-1} with the upsampled P_level"""
    layer = f"p{level - 1}-in-fusion-with-p{level}-in-upsampled"
    return tuple(f"fpn/{layer}/{layer}-{which}-level-weight" for which in ("lower", "upper"))


# ---- forward, fp32 + rs ------------------------------------------------------------------------------------------------
def rs(x, dtype):
    """fp32 -> storage -> fp32"""
    return x.to(dtype).to(F32)


class Coef:
    """a_l, a_u, s of one fusion as fp32 tensors holding storage values ([1] or [C]), from the f32 variables"""

    def __init__(self, w_l, w_u, dtype):
        w_l, w_u = torch.as_tensor(w_l, dtype=F32).reshape(-1), torch.as_tensor(w_u, dtype=F32).reshape(-1)
        self.w_l, self.w_u, self.dtype = w_l, w_u, dtype
        self.a_l, self.a_u = rs(w_l.clamp_min(0.0), dtype), rs(w_u.clamp_min(0.0), dtype)
        self.s = rs(rs(self.a_l + self.a_u, dtype) + rs(torch.tensor(1e-4, dtype=F32), dtype), dtype)

    def f64(self):
        """(a_l, a_u, s, c_l, c_u) in float64"""
        a_l, a_u, s = self.a_l.to(F64), self.a_u.to(F64), self.s.to(F64)
        return a_l, a_u, s, a_l / s, a_u / s


def fuse_z(lo, up, k):
    """z = rs(rs(rs(lo * a_l) / s) + rs(rs(up * a_u) / s)) as a storage tensor; lo, up storage tensors [..., C]"""
    dt = k.dtype
    a = rs(rs(lo.to(F32) * k.a_l, dt) / k.s, dt)
    b = rs(rs(up.to(F32) * k.a_u, dt) / k.s, dt)
    return (a + b).to(dt)


def fuse(lo, up, k, act):
    """out = rs(act(z)) for act = none | relu | relu6 (exact on storage values); swish is judged from z (act_ref)"""
    return R.act_fwd(fuse_z(lo, up, k).to(F32), act).to(k.dtype)


def fuse_torch(lo, up, w_l, w_u):
    """torch's own per-op arithmetic in the storage dtype: the f32 variables cast to it, every op's result a tensor of it"""
    dt = lo.dtype
    a_l, a_u = torch.relu(torch.as_tensor(w_l, dtype=F32).to(dt)), torch.relu(torch.as_tensor(w_u, dtype=F32).to(dt))
    s = a_l + a_u + torch.tensor(1e-4, dtype=dt)
    return lo * a_l / s + up * a_u / s


def fuse_coefficient_form(lo, up, k):
    """in * (a_l / s) + up * (a_u / s) with ONE rounding: NOT the contract"""
    return (lo.to(F32) * (k.a_l / k.s) + up.to(F32) * (k.a_u / k.s)).to(k.dtype)


def topdown_fwd(ins, ks, act):
    """out[L-1] = in[L-1]; out[j] = fuse(in[j], up2(out[j+1]), ks[j]); storage tensors, act none | relu | relu6"""
    outs = [None] * len(ins)
    outs[-1] = ins[-1]
    for j in range(len(ins) - 2, -1, -1):
        outs[j] = fuse(ins[j], R.up(outs[j + 1], 2), ks[j], act)
    return outs


# ---- backward, float64 with the stated rounding points -----------------------------------------------------------------
def level_g(dout, g_finer, cu_finer, out, act, dtype):
    """g = rs((dout + c_u sum2x2(g_finer)) act'(out)) as pyramid_ref.Ref (out None: no gate — the top level's din).
    fp32 operations of an element: three adds of the window, the product with c_u (itself a rounded fp32 quotient: one
    more), the add to dout, the gate: n = 7.  g_finer is taken as GIVEN (the tests pass the kernel's own stored copy)."""
    t, terms = dout, dout.abs()
    if g_finer is not None:
        t = t + cu_finer * R.sumpool(g_finer, 2)
        terms = terms + cu_finer.abs() * R.sumpool(g_finer.abs(), 2)
    m = torch.ones_like(dout) if out is None else R.act_mask(out, act)
    return R.Ref(R.round_storage(t * m, dtype), terms * m, 7)


def level_din(g, c_l, dtype):
    """din = rs(c_l g) from the STORED g: the product and the rounded quotient c_l, n = 2"""
    return R.Ref(R.round_storage(c_l * g, dtype), (c_l * g).abs(), 2)


def level_sums(g, in_lower, out_upper):
    """(Sl, Su, sum|g in|, sum|g up|) per channel over n, y, x in float64, from the STORED g"""
    u = R.up(out_upper, 2)
    return ((g * in_lower).sum((0, 1, 2)), (g * u).sum((0, 1, 2)), (g * in_lower).abs().sum((0, 1, 2)),
            (g * u).abs().sum((0, 1, 2)))


def weight_grads(Sl, Su, a_l, a_u, s, w_l, w_u):
    """(dw_l, dw_u): per channel, or for one-element weights (fast_attention) from the sums over the channels"""
    if a_l.numel() == 1:
        Sl, Su = Sl.sum().reshape(1), Su.sum().reshape(1)
    da_l = (Sl * (s - a_l) - Su * a_u) / s ** 2
    da_u = (Su * (s - a_u) - Sl * a_l) / s ** 2
    return da_l * (w_l > 0).to(F64), da_u * (w_u > 0).to(F64)


def exact_coef(w_l, w_u):
    """(a_l, a_u, s, c_l, c_u) of the unrounded function in float64"""
    a_l, a_u = w_l.to(F64).clamp_min(0.0), w_u.to(F64).clamp_min(0.0)
    s = a_l + a_u + 1e-4
    return a_l, a_u, s, a_l / s, a_u / s


def topdown_exact(ins, ws, act):
    """the unrounded forward in float64 (differentiable): out[j] = act((in[j] a_l + up2(out[j+1]) a_u) / s)"""
    outs = [None] * len(ins)
    outs[-1] = ins[-1]
    for j in range(len(ins) - 2, -1, -1):
        a_l, a_u = torch.relu(ws[j][0]), torch.relu(ws[j][1])
        s = a_l + a_u + 1e-4
        outs[j] = R.act_fwd(ins[j] * a_l / s + R.up(outs[j + 1], 2) * a_u / s, act)
    return outs


def topdown_bwd(douts, ins, outs, coefs, ws, act, dtype):
    """The whole backward, finest level first: ([din], [(dw_l, dw_u)], [g]) in float64; coefs[j] = (a_l, a_u, s, c_l, c_u),
    ws[j] = (w_l, w_u); dtype None: no rounding anywhere."""
    L = len(ins)
    dins, dws, gs = [], [], []
    g_prev = cu_prev = None
    for j in range(L):
        if j == L - 1:
            dins.append(level_g(douts[j], g_prev, cu_prev, None, None, dtype).value)
            break
        a_l, a_u, s, c_l, c_u = coefs[j]
        g = level_g(douts[j], g_prev, cu_prev, outs[j], act, dtype).value
        dins.append(level_din(g, c_l, dtype).value)
        Sl, Su, _, _ = level_sums(g, ins[j], outs[j + 1])
        dws.append(weight_grads(Sl, Su, a_l, a_u, s, ws[j][0], ws[j][1]))
        gs.append(g)
        g_prev, cu_prev = g, c_u
    return dins, dws, gs


# ---- the whole network ---------------------------------------------------------------------------------------------------
class _FusedFpn:
    """fpn() of oracle/model_ref.py (fpn_base.py:54-71, fpn.py:81-107) with the weighted FeatureFusion in the top-down
    path; NCHW inside, like the rest of RefModel"""

    def fpn(self, feats):
        ff = self.p.architecture.feature_fusion
        if ff.fusion_mode == "sum":
            return super().fpn(feats)
        lo, hi, bmax = ff.min_level, ff.max_level, ff.backbone_max_level
        act = self.p.architecture.activation.type
        t = self.bn_tag
        r = lambda x: _r(x, self.bf)
        out = dict(feats)
        for level in range(bmax + 1, hi + 1):
            x = out[str(level - 1)]
            if level == bmax + 1:
                x = r(self._bn(self._cs(x, "fpn/backbone_max_level_conv_1x1"), f"fpn/backbone_max_level_{t}"))
            out[str(level)] = F.max_pool2d(x, 2)
        for level in range(lo, bmax + 1):
            x = self._cs(out[str(level)], f"fpn/p{level}-in-channel-normalize-conv-1x1")
            out[str(level)] = r(self._bn(x, f"fpn/p{level}-in-channel-normalize-{t}"))
        for level in range(hi, lo, -1):
            up = F.interpolate(out[str(level)], scale_factor=2, mode="nearest")
            nl, nu = var_names(level)
            w_l, w_u = self.v[nl].reshape(1, -1, 1, 1), self.v[nu].reshape(1, -1, 1, 1)
            a_l, a_u = r(F.relu(w_l)), r(F.relu(w_u))
            s = r(r(a_l + a_u) + r(torch.tensor(1e-4, dtype=w_l.dtype)))
            z = r(r(r(out[str(level - 1)] * a_l) / s) + r(r(up * a_u) / s))
            out[str(level - 1)] = r(self._act(z, act))
        for level in range(lo, hi + 1):
            x = self._cs(out[str(level)], f"fpn/p{level}-out-conv-3x3")
            out[str(level)] = r(self._bn(x, f"fpn/p{level}-out-{t}"))
        return {str(l): out[str(l)] for l in range(lo, hi + 1)}


class FusedRefModel(_FusedFpn, RefModel):
    pass


class FusedRefTrainer(_FusedFpn, RefTrainer):
    def weight_decay(self):
        alpha = self.p.training.weight_decay_alpha
        tot = super().weight_decay()
        for k, t in self.leaf.items():
            if k.endswith("-level-weight"):
                tot = tot + alpha * 0.5 * (t * t).sum()
        return tot


def same_values(got, want):
    """act_ref.same_values with non-finite positions compared as such: the same infinities at the same places, a NaN only
    where the reference has one (inf - inf of the contract's own formula); elsewhere bit for bit, the two zeros equal"""
    gf, wf = got.float(), want.float()
    fin = torch.isfinite(wf)
    if not bool((torch.isfinite(gf) == fin).all()):
        return False
    nonfin_ok = bool(((gf == wf) | (torch.isnan(gf) & torch.isnan(wf)))[~fin].all())
    zero = torch.zeros_like(got)
    return nonfin_ok and A.same_values(torch.where(fin, got, zero), torch.where(fin, want, zero))
