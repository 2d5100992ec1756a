"""Float64 references of the activations (none | relu | relu6 | swish) and of their gradient gates, the tensor that holds
every value a 16-bit activation input can take, and the rule that compares a kernel's stored result with the reference.
In the style of pyramid_ref.py, whose rounding helpers (`round_storage`, `ulp_s`) are used here.

An activation has ONE input, so one small tensor covers its whole domain: `sweep(dtype)` is every bit pattern of the
storage type (65 280 finite bfloat16 values, 63 488 finite half values; the non-finite patterns are replaced by 0).

The acceptance rule (derived, not tuned)
----------------------------------------
A kernel stores got = rs(v32): v32 an fp32 evaluation of the activation (or of its derivative), rs one rounding to the
16-bit storage type.  The reference `ref` is the float64 value, NOT rounded.  Then
        |got - ref| <= ulp_s(ref) / 2 + slack                                                  (`bound`)
  * ulp_s(ref) = eps max(|ref|, smallest normal), eps = 2^-7 (bfloat16) or 2^-10 (half), is between one and two times the
    spacing of the storage type at ref, so ulp_s / 2 covers the one rounding rs() of a value that sits AT ref.
  * slack covers |v32 - ref|, the fp32 evaluation:
      swish value  x sigmoid(x):  slack = 2^-16 |ref| + 1e-30.  The product x log2(e) inside exp carries an absolute error
        of |x| 2^-24 into the exponent, a relative error of |x| 2^-24 <= 2^-17.5 of e^-x for |x| < 88.7 (beyond, e^-x
        overflows or the sigmoid is 1 to fp32); v_exp_f32, v_rcp_f32 and three roundings add a few 2^-24.  The 1e-30
        floor: below x = -88.7 the fp32 sum 1 + e^-x is infinite and the kernels return -0 where the value is about
        -2e-37 (bfloat16 reaches that far; -2e-37 is a normal bfloat16 value, so only the floor accepts the -0).
      swish derivative  s + x s (1 - s):  slack = 2^-20, ABSOLUTE: the derivative crosses zero near x = -1.2785, where
        no relative bound can hold; its value is in [-0.0998, 1.0998] and each of its five fp32 operations is off by at
        most 2^-24 of an operand of that size, the sigmoid by |x| 2^-24 s (1 - s)-weighted as above.
      relu, relu6, none and their 0 / 1 gates: slack = 0 — and since their results are storage values themselves, they
        are compared bit for bit (`same_values`; the two zeros compare equal: fmaxf(-0, 0) may return either).
  * below the smallest normal storage value the rounded reference OR a zero is accepted: whether a kernel keeps
    subnormals is not what these tests are about.
The rule has teeth (test_act_ref_cpu.py): a gate of 1 for swish, a gate taken in front of the residual add, a sigmoid
that is off by a relative 2^-12 and a swish taken on the unrounded residual sum are all rejected, while an fp32
transcription of the formulas is accepted on every input of both storage types.
"""
import torch

import pyramid_ref as R

F64 = R.F64
ACTS = ("none", "relu", "relu6", "swish")
C = 64                                   # channels of the sweep tensor: [P, 64]
DERIV_SLACK = 2.0 ** -20


def sweep(dtype):
    """[P, 64] tensor of `dtype` holding every finite value of the type (element i = bit pattern i, the non-finite
    patterns replaced by +0): P = 1024 rows."""
    bits = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16)
    bits = torch.cat([bits[1 << 15:], bits[:1 << 15]])           # 0x0000 .. 0xffff in order
    v = bits.view(dtype)
    v = torch.where(torch.isfinite(v.float()), v, torch.zeros_like(v))
    return v.reshape(-1, C).contiguous()


def n_finite(dtype):
    return int((sweep(dtype).view(torch.int16) != 0).sum()) + 1   # every non-zero pattern left, and +0


def sigmoid(v):
    return torch.sigmoid(v.to(F64))


def act_fwd(v, act):
    """float64 activation value"""
    if act == "swish":
        return v * sigmoid(v)
    return R.act_fwd(v, act)


def act_deriv(u, act):
    """float64 derivative at u: swish s + u s (1 - s); relu / relu6 / none: the 0 / 1 gate of pyramid_ref.act_mask"""
    if act == "swish":
        s = sigmoid(u)
        return s + u * s * (1.0 - s)
    return R.act_mask(u, act)


def value_slack(ref, act):
    return 2.0 ** -16 * ref.abs() + 1e-30 if act == "swish" else torch.zeros_like(ref)


def deriv_slack(ref, act):
    return torch.full_like(ref, DERIV_SLACK if act == "swish" else 0.0)


def bound(ref, dtype, slack):
    return 0.5 * R.ulp_s(ref, dtype) + slack


def check(got, ref, dtype, slack):
    """(every element accepted, largest |got - ref| / bound among the elements judged by the bound, number of elements
    outside, flat index of the worst element).  Below the smallest normal storage value a zero is accepted as well.
    A NaN or a shape mismatch is a miss."""
    if got.shape != ref.shape:
        return False, float("inf"), got.numel(), 0
    g = got.to(F64)
    ratio = (g - ref).abs() / bound(ref, dtype, slack)
    flushed = (ref.abs() < R._FMT[dtype][3]) & (g == 0)
    ratio = torch.where(flushed, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    outside = int((ratio > 1.0).sum())
    worst = int(ratio.reshape(-1).argmax())
    return outside == 0, float(ratio.reshape(-1)[worst]), outside, worst


def accept(got, ref, dtype, slack):
    return check(got, ref, dtype, slack)[0]


def same_values(got, want):
    """bit for bit, except that the two zeros are the same value (and no NaN anywhere)"""
    g, w = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    zero = (got.float() == 0) & (want.float() == 0)
    return bool(((g == w) | zero).all()) and not bool(torch.isnan(got.float()).any())


# ---- the fp32 transcription of the kernels' formulas (numpy: exp in fp32, a true division) ---------------------------
def fp32_sigmoid(x32, rel=0.0):
    import numpy as np
    with np.errstate(over="ignore"):
        s = np.float32(1.0) / (np.float32(1.0) + np.exp(-x32))
    return (s * np.float32(1.0 + rel)).astype(np.float32)


def fp32_swish(x, dtype, rel=0.0):
    """x: tensor of `dtype` -> swish evaluated in fp32, stored as `dtype`"""
    x32 = x.float().numpy()
    return torch.from_numpy(x32 * fp32_sigmoid(x32, rel)).to(dtype)


def fp32_swish_deriv(x, dtype, rel=0.0):
    import numpy as np
    x32 = x.float().numpy()
    s = fp32_sigmoid(x32, rel)
    return torch.from_numpy((s + x32 * s * (np.float32(1.0) - s)).astype(np.float32)).to(dtype)
