"""Float64 reference of training-mode BatchNorm whose batch is spread over R replicas (SyncBatchNormalization), the inputs
the SyncBN tests share, and the acceptance rules they share.  Plain torch on the CPU; nothing of the library is imported.

A replica is a shard of rows: shard r holds y_r [P, C] (values of the 16-bit storage type).  The statistics are those of
the concatenation, n = R*P rows:
    mean = sum y / n,  var = sum y^2 / n - mean^2 (never below 0),  invstd = 1 / sqrt(var + eps),
    scale = gamma invstd,  shift = beta - mean scale,
    moving_mean' = moving_mean m + mean (1 - m),  moving_var' = moving_var m + var c (1 - m),
    c = n / (n - 1) iff bessel and n > 1, else 1.
Forward of a shard, rs = one rounding to the storage type, u = y scale + shift (rn_bn_apply, include/rnet_hip.h):
    no residual:  z = rs(act(u)), swish: z = rs(swish(rs(u)));   residual: v = rs(rs(u) + residual), z = rs(act(v)).
Backward: g = dz act'(.) — relu / relu6: 1 where the STORED z is > 0 (and < 6); swish: s + v s (1 - s) at v behind a
residual add and at the unrounded u without one; xhat = (y - mean) invstd.  Per shard the LOCAL sums (sum g, sum g xhat)
are what dbeta / dgamma and the shard's bsums hold before the all-reduce; the global sums are their sums over shards;
    dy = scale (g - sum_g / n - xhat sum_gxhat / n)   with the GLOBAL sums and n = R*P;   dres = rs(g [+ dres]).
`n_override` replaces n everywhere it is read (the discrimination check of test_syncbn_ref_cpu.py: a kernel that ignores
count_scale divides the all-reduced sums by the local P).

Inputs (`make_inputs`): shard r draws y from N(2.3 + 2 r, (1 + 0.25 r)^2); dz is random with about 20 % zero rows
(segments of 8 rows or more).  Segments of 16 channels or more carry four special channels: 0 constant over all shards
(var = 0), 1 constant within a shard but not between shards, 2 = 64 + N(0, 0.5^2) (E[y^2] - mean^2 cancels), 3 all zero
with a non-zero dz.  Why these means and not N(0.3 + 0.7 r, .): test_syncbn_ref_cpu.py asks that a kernel without
count_scale and a kernel with local statistics miss every bound by 10x on EVERY ordinary channel.  A kernel that divides
the all-reduced sums by P has var' = R E[y^2] - R^2 mean^2, which EQUALS var where var = R mean^2: with means of
0.65 .. 1 and variances of 1.4 .. 1.9 (R = 2, 3) a 25-row sample lands there on several channels of 256, and on those the
wrong kernel is right.  With mean 2.3 or more R mean^2 is far above any sample variance (var' < 0, clamped).  Likewise
a between-shard variance of 0.7^2 / 4 is a tenth of the within-shard one and smaller than the sampling noise of a
36-row variance, so some channel's local variances equal the global one to a few per cent — less than ten bfloat16
steps of dy; a spread of 2 per shard makes the global variance 1.6x the local ones.

Acceptance rules shared by the GPU test and the CPU discrimination check: FWD_TOL / MOVING_TOL (rtol, atol) for the
ordinary channels, `step_top` (one storage step in the top binade of the reference, per channel) and the mismatch-share CAPS
of tests/test_gpu_bench_shapes_more.py::_check_bn_problem."""
import torch

import pyramid_ref as R

F64 = torch.float64
SEGMENTS = [(126, 64), (25, 256), (48, 8), (36, 144), (1, 16)]      # rows per shard x channels: one problem
BIG_SEGMENT = (16416, 64)                                           # 513 row chunks: the split stage-2 reduction
REPLICAS = [2, 3, 8]
N_SPECIAL = 4
OFFSET, SPREAD = 2.3, 2.0            # mean of shard r = OFFSET + SPREAD r (module docstring)
MIN_POPULATION = 1000                # elements a segment needs to be held to a mismatch-share cap on its own
FWD_ROWS = ("mean", "invstd", "scale", "shift")
FWD_TOL = {"mean": (1e-5, 1e-5), "invstd": (2e-5, 0.0), "scale": (2e-5, 0.0), "shift": (1e-4, 2e-5)}
MOVING_TOL = (1e-5, 1e-5)
CAPS = {"z": 0.02, "dy": 0.03, "dres": 0.01}
# (id, act, residual input (with the gate bit mask behind a relu), bessel, dres_accumulate)
FORMS = [("relu-res-mask-acc", "relu", True, 1, 1), ("relu-res-mask", "relu", True, 0, 0), ("relu", "relu", False, 0, 0),
         ("none", "none", False, 1, 0), ("swish", "swish", False, 0, 0)]


def f32(x):
    """the float32 value of a Python float, as a Python float: eps and momentum as the library reads them"""
    return float(torch.tensor(x, dtype=torch.float32))


# momentum 0.5 and not the engine's 0.99: old and new statistics weigh the same, so an error in either shows at half its
# size against the rtol 1e-5 bound instead of a hundredth of it
EPS, MOMENTUM = f32(1e-3), f32(0.5)


def rs(v, dtype):
    return R.round_storage(v, dtype)


def special(C):
    """number of special channels (the first ones) of a segment with C channels"""
    return N_SPECIAL if C >= 16 else 0


def make_inputs(shapes, replicas, dtype, seed):
    """one dict per segment: P, C, per-shard lists ys / dzs / res / dres0 (storage type) and gamma, beta, mm, mv (float32).
    Built from one generator in a fixed order; callers never modify the tensors."""
    g = torch.Generator().manual_seed(seed)
    segs = []
    for P, C in shapes:
        s = {"P": P, "C": C, "ys": [], "dzs": [], "res": [], "dres0": []}
        for r in range(replicas):
            y = torch.randn((P, C), generator=g) * (1.0 + 0.25 * r) + (OFFSET + SPREAD * r)
            if special(C):
                y[:, 0] = 0.75
                y[:, 1] = 0.5 + 0.25 * r
                y[:, 2] = 64.0 + torch.randn((P,), generator=g) * 0.5
                y[:, 3] = 0.0
            keep = (torch.rand((P, 1), generator=g) < 0.8).float() if P >= 8 else torch.ones((P, 1))
            s["ys"].append(y.to(dtype))
            s["dzs"].append((torch.randn((P, C), generator=g) * keep).to(dtype))
            s["res"].append(torch.randn((P, C), generator=g).to(dtype))
            s["dres0"].append(torch.randn((P, C), generator=g).to(dtype))
        s["gamma"] = torch.rand((C,), generator=g) + 0.5
        s["beta"] = torch.randn((C,), generator=g) * 0.3
        s["mm"] = torch.randn((C,), generator=g)
        s["mv"] = torch.rand((C,), generator=g) + 0.5
        segs.append(s)
    return segs


# ---- the formulas -------------------------------------------------------------------------------------------------------
def act_fwd(v, act):
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "relu6":
        return v.clamp(0.0, 6.0)
    if act == "swish":
        return v * torch.sigmoid(v)
    assert act in (None, "none")
    return v


def swish_deriv(v):
    s = torch.sigmoid(v)
    return s + v * s * (1.0 - s)


def stats(ys, gamma, beta, eps, n_override=None):
    """global statistics of the concatenated shards -> dict n, mean, var, ey2 (= E[y^2]), invstd, scale, shift (float64)"""
    cat = torch.cat([y.to(F64) for y in ys])
    n = float(cat.shape[0] if n_override is None else n_override)
    mean = cat.sum(0) / n
    ey2 = (cat * cat).sum(0) / n
    var = (ey2 - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(F64) * invstd
    return {"n": n, "mean": mean, "var": var, "ey2": ey2, "invstd": invstd, "scale": scale,
            "shift": beta.to(F64) - mean * scale}


def moving(mm, mv, mean, var, n, momentum, bessel):
    corr = n / (n - 1.0) if bessel and n > 1 else 1.0
    return mm.to(F64) * momentum + mean * (1.0 - momentum), mv.to(F64) * momentum + var * corr * (1.0 - momentum)


def forward(y, scale, shift, residual, act, dtype):
    """(u, v, z): u = y scale + shift unrounded, v the value in front of the activation, z the stored output (float64)"""
    u = y.to(F64) * scale + shift
    if residual is not None:
        v = rs(rs(u, dtype) + residual.to(F64), dtype)
    elif act == "swish":
        v = rs(u, dtype)
    else:
        v = u
    return u, v, rs(act_fwd(v, act), dtype)


def gradient(dz, u, v, z, act, has_residual):
    """g = dz act'(.), the gate of relu / relu6 taken on the stored z"""
    dz = dz.to(F64)
    if act == "relu":
        return dz * (z > 0).to(F64)
    if act == "relu6":
        return dz * ((z > 0) & (z < 6)).to(F64)
    if act == "swish":
        return dz * swish_deriv(v if has_residual else u)
    return dz


def xhat_of(y, mean, invstd):
    return (y.to(F64) - mean) * invstd


def dy_of(g, xhat, scale, sum_g, sum_gx, n):
    return scale * (g - sum_g / n - xhat * sum_gx / n)


def reference(ys, gamma, beta, eps, momentum, bessel, dtype, residuals=None, dzs=None, act="none", mm=None, mv=None,
              dres0=None, accumulate=False, n_override=None):
    """everything the passes write, in float64: the statistics dict of `stats` plus mm / mv (new moving statistics) and, per
    shard, z, g, xhat, local_sums [(sum g, sum g xhat)], and dy, dres from the global sums"""
    out = stats(ys, gamma, beta, eps, n_override)
    n = out["n"]
    if mm is not None:
        out["mm"], out["mv"] = moving(mm, mv, out["mean"], out["var"], n, momentum, bessel)
    out["z"], out["g"], out["xhat"], out["local_sums"] = [], [], [], []
    for r, y in enumerate(ys):
        res = None if residuals is None else residuals[r]
        u, v, z = forward(y, out["scale"], out["shift"], res, act, dtype)
        out["z"].append(z)
        if dzs is None:
            continue
        g = gradient(dzs[r], u, v, z, act, res is not None)
        xh = xhat_of(y, out["mean"], out["invstd"])
        out["g"].append(g)
        out["xhat"].append(xh)
        out["local_sums"].append((g.sum(0), (g * xh).sum(0)))
    if dzs is not None:
        out["sum_g"] = sum(s[0] for s in out["local_sums"])
        out["sum_gx"] = sum(s[1] for s in out["local_sums"])
        out["dy"] = [dy_of(g, xh, out["scale"], out["sum_g"], out["sum_gx"], n) for g, xh in zip(out["g"], out["xhat"])]
        out["dres"] = [rs(g + (dres0[r].to(F64) if accumulate else 0.0), dtype) for r, g in enumerate(out["g"])]
    return out


def from_table(y, dz, res, dres0, tab, bs, n, act, accumulate, dtype, z_stored=None):
    """What a kernel must store given ITS OWN float32 fwd table `tab` [4, C] and all-reduced sums `bs` [2, C] (whose
    accuracy is asserted separately): z, dy, dres in float64 holding storage values, g, xhat, and the element bounds.
    The relu gates are taken on `z_stored` (the kernel's z) when given."""
    t, b = tab.to(F64), bs.to(F64)
    u, v, z = forward(y, t[2], t[3], res, act, dtype)
    g = gradient(dz, u, v, z if z_stored is None else z_stored.to(F64), act, res is not None)
    xh = xhat_of(y, t[0], t[1])
    # uncertainty of g inherited by a swish gate: the fp32 evaluation of swish' (SWISH_GATE_SLACK) and of its argument
    # u = y scale + shift (two roundings, each 2^-24 of its operand: on a channel whose mean is many standard deviations
    # from 0 the two terms cancel), times |swish''| <= 1/2
    slack = torch.zeros_like(u)
    if act == "swish":
        slack = dz.to(F64).abs() * (SWISH_GATE_SLACK + 0.5 * 2.0 ** -23 * ((y.to(F64) * t[2]).abs() + t[3].abs()))
    out = {"z": z, "g": g, "xhat": xh, "gslack": slack, "dy": rs(dy_of(g, xh, t[2], b[0], b[1], float(n)), dtype),
           "dres": rs(g + (dres0.to(F64) if accumulate else 0.0), dtype)}
    # z behind an INNER rounding (rs(u) in front of a residual add or of swish): where the fp32 u and the float64 u fall
    # on different sides of a rounding boundary the inner value moves by one spacing at u, and z follows it with the
    # slope of what comes after (1 for the add, at most 1.0998 for swish) before its own rounding
    inner = None
    if res is not None or act == "swish":
        inner = spacing(rs(u, dtype), dtype) * (1.0998 if act == "swish" else 1.0)
    out["bound"] = {"z": element_bound(z, dtype, gate_slack=inner),
                    "dres": element_bound(out["dres"], dtype, gate_slack=slack),
                    "dy": element_bound(out["dy"], dtype, dy_terms(g, xh, t[2], b[0], b[1], float(n)), 8,
                                        t[2].abs() * slack)}
    return out


# ---- acceptance rules ---------------------------------------------------------------------------------------------------
def tol_ratio(got, want, tol):
    """|got - want| / (atol + rtol |want|) per element; tol = (rtol, atol)"""
    return (got.to(F64) - want).abs() / (tol[1] + tol[0] * want.abs()).clamp_min(1e-300)


def step_top(want, dtype):
    """per channel (column of want [P, C]): one step of the storage type in the top binade of that channel,
    2^(e - p + 1) for max |want[:, c]| in [2^e, 2^(e+1)); 0 for an all-zero channel.  Per channel and not per tensor: the
    special channels (invstd = 1 / sqrt(eps)) carry gradients a hundred times those of the others."""
    top = want.abs().max(0).values
    _, e = torch.frexp(top)                                    # top in [2^(e-1), 2^e)
    step = torch.exp2((e - R._FMT[dtype][0]).to(F64))
    return torch.where(top == 0, torch.zeros_like(step), step)


def spacing(x, dtype):
    """distance between neighbouring storage values at |x| (of the smallest normal below it), elementwise"""
    _, e = torch.frexp(x.abs().clamp_min(R._FMT[dtype][3]))
    return torch.exp2((e - R._FMT[dtype][0]).to(F64))


SWISH_GATE_SLACK = 2.0 ** -20          # absolute error of an fp32 swish'(v) (act_ref.DERIV_SLACK, derived there)


def dy_terms(g, xhat, scale, sum_g, sum_gx, n):
    """sum of the absolute values of the terms of dy: what the roundings of its fp32 evaluation are relative to"""
    return scale.abs() * (g.abs() + (sum_g / n).abs() + (xhat * sum_gx / n).abs())


def element_bound(want, dtype, terms=None, ops=0, gate_slack=None):
    """|got - want| allowed per element: one storage step in the top binade of the channel, plus the fp32 evaluation
    error `ops` 2^-23 `terms` (pyramid_ref.Ref.bound), plus an inherited uncertainty `gate_slack` (a swish gate; an inner
    rounding in front of z, see from_table).  The two extra
    terms are a thousandth of the step on ordinary data; they matter where dy is a difference of nearly equal terms — a
    batch of n = 2 rows has dy = O(eps / var) of its terms, and a float32 evaluation of it is already more than one
    half-precision step away from the float64 one (test_syncbn_ref_cpu.py shows that on the 1 x 16 segment)."""
    b = step_top(want, dtype).expand_as(want).clone()
    if terms is not None:
        b += ops * 2.0 ** -23 * terms
    if gate_slack is not None:
        b += gate_slack
    return b


def mismatches(got, want):
    """(elements that differ at all, elements)"""
    return int((got.to(F64) != want).sum()), got.numel()


def worst_share(counts):
    """counts: (mismatches, elements) per segment of ONE problem (one shard).  The largest share among the segments of
    MIN_POPULATION elements or more and the problem as a whole: a 1 x 16 segment holds 16 elements, so a single rounding
    that falls the other way is 6 % of it — a share cap says nothing about a population smaller than 1 / cap."""
    shares = [m / n for m, n in counts if n >= MIN_POPULATION]
    shares.append(sum(m for m, _ in counts) / sum(n for _, n in counts))
    return max(shares)
