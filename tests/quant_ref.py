"""Plain numpy restatement of the INT8 serving arithmetic (include/rnet_hip.h "INT8 serving"): the symmetric
quantiser, the 3x3 integer convolution (int64 accumulation), the three-step float32 epilogue and a loop-form float64
KL (entropy) threshold search.  Shares no code with the product."""
import math

import numpy as np

F32 = np.float32
BINS = 2048
LEVELS = 128


def quantize(x, inv_scale):
    """q = clamp(rint(float32(x) * inv_scale), -127, 127), the product rounded to float32 first"""
    t = np.asarray(x, dtype=F32) * F32(inv_scale)
    return np.clip(np.rint(t), -127, 127).astype(np.int8)


def quantize_weights(w_ohwi):
    """per-output-channel symmetric int8 of f32 weights [Cout, 3, 3, Cin] -> (int8 weights, float32 scales)"""
    w = np.asarray(w_ohwi, dtype=F32)
    amax = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
    scale = np.where(amax > 0, amax / F32(127), F32(1)).astype(F32)
    q = np.clip(np.rint(w / scale[:, None, None, None]), -127, 127).astype(np.int8)
    return q, scale


def conv3x3_int(x, w):
    """x int8 [N,H,W,Cin], w int8 [Cout,3,3,Cin] -> int64 [N,H,W,Cout]; stride 1, zero padding 1.  The nine taps are
    accumulated in int64; one tap's sum over Cin goes through a floating-point matrix product, which is exact in any
    summation order: every product and partial sum is an integer below Cin * 127^2, which is below 2^24 (float32) for
    Cin <= 1024 and below 2^53 (float64) otherwise."""
    x = np.asarray(x)
    w = np.asarray(w)
    N, H, W, cin = x.shape
    assert cin * 127 * 127 < 2 ** 53
    ft = np.float32 if cin * 127 * 127 < 2 ** 24 else np.float64
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))).astype(ft)
    wf = w.astype(ft)
    acc = np.zeros((N, H, W, w.shape[0]), dtype=np.int64)
    for r in range(3):
        for s in range(3):
            tap = xp[:, r:r + H, s:s + W, :].reshape(-1, cin) @ wf[:, r, s, :].T
            acc += tap.astype(np.int64).reshape(N, H, W, -1)
    return acc


def activation(t, act):
    if act in (None, "none"):
        return t
    if act == "relu":
        return np.maximum(t, F32(0))
    if act == "relu6":
        return np.minimum(np.maximum(t, F32(0)), F32(6))
    raise ValueError(act)


def epilogue(acc, mul, add, act, out_inv_scale=None):
    """t = float32(acc) * mul; t = t + add; t = act(t); int8: clamp(rint(t * out_inv_scale)); every step rounded to
    float32.  out_inv_scale None: the float32 output."""
    assert np.abs(acc).max() < 2 ** 31
    t = acc.astype(np.int32).astype(F32) * np.asarray(mul, dtype=F32)
    t = t + np.asarray(add, dtype=F32)
    t = activation(t, act).astype(F32)
    if out_inv_scale is None:
        return t
    return np.clip(np.rint(t * F32(out_inv_scale)), -127, 127).astype(np.int8)


def conv3x3_i8(x, w, mul, add, act, out_inv_scale=None):
    return epilogue(conv3x3_int(x, w), mul, add, act, out_inv_scale)


def histogram(x, rng, counts=None):
    """2048 bins of |x| over [0, rng]: bin = min(int(|x| * (2048 / rng)), 2047), quotient and product in float32"""
    per_unit = F32(BINS) / F32(rng)
    f = np.minimum(np.abs(np.asarray(x, dtype=F32)).reshape(-1) * per_unit, F32(BINS - 1))
    h = np.bincount(f.astype(np.int64), minlength=BINS).astype(np.int64)
    return h if counts is None else counts + h


def _kl(p, q):
    """sum p log(p / q) over p > 0, both normalised; inf where q is 0 under a positive p"""
    ps, qs = float(sum(p)), float(sum(q))
    total = 0.0
    for a, b in zip(p, q):
        if a > 0:
            if b <= 0:
                return float("inf")
            total += (a / ps) * math.log((a / ps) / (b / qs))
    return total


def kl_threshold_bin(hist):
    """The published TensorRT-style entropy calibration, loop form, float64.  For every candidate i in 128 .. 2048: the
    reference distribution is hist[:i] with the clipped tail hist[i:] folded into its last bin; the candidate is hist[:i]
    merged into 128 groups (group j = bins [j*i // 128, (j+1)*i // 128)) and expanded back uniformly over the NON-ZERO
    bins of each group (zeros stay zero).  Returns the first i of minimal KL divergence (the threshold is i bin widths)."""
    hist = [float(v) for v in hist]
    best, best_i = None, None
    for i in range(LEVELS, BINS + 1):
        ref = hist[:i]
        ref[i - 1] += sum(hist[i:])
        if sum(ref) <= 0:
            continue
        cand = [0.0] * i
        for j in range(LEVELS):
            lo, hi = (j * i) // LEVELS, ((j + 1) * i) // LEVELS
            live = [k for k in range(lo, hi) if hist[k] > 0]
            if live:
                share = sum(hist[lo:hi]) / len(live)
                for k in live:
                    cand[k] = share
        if sum(cand) <= 0:
            continue
        d = _kl(ref, cand)
        if best is None or d < best:
            best, best_i = d, i
    return BINS if best_i is None else best_i


def entropy_scale(hist, amax):
    return np.float64(kl_threshold_bin(hist)) * (np.float64(amax) / BINS) / 127.0
