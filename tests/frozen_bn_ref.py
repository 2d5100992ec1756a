"""Numpy restatement of a FROZEN BatchNorm under a trainable conv (the `bn` / `*-bn` keys of training.freeze_variables):
the layer runs in inference mode inside the training step,
        z = act((y scale + shift) [m_n] + residual),     scale = gamma / sqrt(moving_var + eps),  shift = beta - moving_mean scale
        g = dz act'(.),    dy = scale (g m_n),    dres (+)= g
with no mean / xhat term and no gradient for gamma / beta.  In the style of act_ref.py / pyramid_ref.py.

Two precisions of the same formulas:
  * fp = numpy.float64, storage = None: the exact function, what central finite differences are taken of;
  * fp = numpy.float32, storage = torch.bfloat16 | torch.float16: the kernels' arithmetic — every product and sum rounded to
    fp32 on its own (the library is built without contraction), and one rounding to the 16-bit storage type exactly where
    rn_bn_apply / rn_bn_frozen_bwd store or round a tensor:
      forward   u = y scale + shift; rounded to storage when a residual add, drop_connect or swish follows; then rs(u m_n);
                then + residual, rounded again in front of swish; z = rs(act(.))
      backward  relu / relu6 gate on the STORED z (which decides the same as u = y scale + shift without a residual input);
                swish' at the value the forward pass fed to swish behind a residual add and at the fp32 u without one
                (include/rnet_hip.h); dy = rs(scale (g m_n)), dres = rs(g [+ dres]).
    For act = none | relu | relu6 the gate is 0 / 1 and dy is ONE fp32 product of exactly representable inputs (two with
    drop_connect) and one rounding: the fp32 restatement gives the kernel's bits.
"""
import numpy as np
import torch

ACTS = ("none", "relu", "relu6", "swish")


def rs(x, storage):
    """one rounding to the storage type (ties to even); float64 input is rounded directly, not through float32"""
    if storage is None:
        return x
    if x.dtype == np.float64:
        import pyramid_ref as R
        return R.round_storage(torch.from_numpy(np.ascontiguousarray(x)), storage).numpy()
    return torch.from_numpy(np.ascontiguousarray(x)).to(storage).to(torch.float32).numpy()


def fold(gamma, beta, moving_mean, moving_var, eps, fp=np.float32):
    """(scale, shift) as model/forward.py:fold_bn computes them"""
    g, b, mm, mv = (np.asarray(t, dtype=fp) for t in (gamma, beta, moving_mean, moving_var))
    scale = g / np.sqrt(mv + fp(eps))
    return scale.astype(fp), (b - mm * scale).astype(fp)


def _sigmoid(v, fp):
    with np.errstate(over="ignore"):
        return (fp(1.0) / (fp(1.0) + np.exp(-v))).astype(fp)


def act_value(v, act, fp):
    if act == "relu":
        return np.maximum(v, fp(0.0))
    if act == "relu6":
        return np.minimum(np.maximum(v, fp(0.0)), fp(6.0))
    if act == "swish":
        return (v * _sigmoid(v, fp)).astype(fp)
    return v


def act_deriv(v, act, fp):
    """d act / dv at v; relu / relu6: 1 strictly inside (0, inf) / (0, 6)"""
    if act == "relu":
        return (v > 0).astype(fp)
    if act == "relu6":
        return ((v > 0) & (v < 6)).astype(fp)
    if act == "swish":
        s = _sigmoid(v, fp)
        return (s + v * s * (fp(1.0) - s)).astype(fp)
    return np.ones_like(v)


def _per_row(sample_scale, rows_per_sample, P, fp):
    if sample_scale is None:
        return None
    return np.repeat(np.asarray(sample_scale, dtype=fp), rows_per_sample)[:P].reshape(P, 1)


def forward(y, scale, shift, act, residual=None, sample_scale=None, rows_per_sample=1, storage=None, fp=np.float64):
    """y, residual [P, C]; scale, shift [C]; sample_scale [P / rows_per_sample] -> dict(z, pre, gate_at): the stored output,
    the value in front of the activation and the value swish' is taken at (the relu / relu6 gates read the stored z)"""
    y = np.asarray(y, dtype=fp)
    m = _per_row(sample_scale, rows_per_sample, y.shape[0], fp)
    u = ((y * np.asarray(scale, dtype=fp)).astype(fp) + np.asarray(shift, dtype=fp)).astype(fp)
    o = u
    if residual is not None or m is not None or act == "swish":     # the BatchNorm output is a 16-bit tensor there
        o = rs(o, storage)
    if m is not None:
        o = rs((o * m).astype(fp), storage)                         # ... and so is the drop_connect output
    if residual is not None:
        o = (o + np.asarray(residual, dtype=fp)).astype(fp)
        if act == "swish":
            o = rs(o, storage)                                      # ... and the Add output in front of tf.nn.swish
    # swish without a residual input: the forward pass feeds rs(u) to swish, the backward passes take swish' at the fp32 u
    # (swish with drop_connect: the kernels refuse the backward; the reference keeps the true derivative, at o)
    gate_at = u if (act == "swish" and residual is None and m is None) else o
    return {"z": rs(act_value(o, act, fp).astype(fp), storage), "pre": o, "gate_at": gate_at}


def backward(dz, scale, act, fwd, sample_scale=None, rows_per_sample=1, dres0=None, storage=None, fp=np.float64):
    """fwd: forward()'s result on the same inputs -> dict(dy, dres, g).  dres0: the value dres holds before
    (dres_accumulate), None for a first write."""
    dz = np.asarray(dz, dtype=fp)
    m = _per_row(sample_scale, rows_per_sample, dz.shape[0], fp)
    gate = act_deriv(np.asarray(fwd["z"] if act in ("relu", "relu6") else fwd["gate_at"], dtype=fp), act, fp)
    g = (dz * gate).astype(fp)
    gm = g if m is None else (g * m).astype(fp)
    dy = rs((np.asarray(scale, dtype=fp) * gm).astype(fp), storage)
    dres = g if dres0 is None else (g + np.asarray(dres0, dtype=fp)).astype(fp)
    return {"dy": dy, "dres": rs(dres, storage), "g": g}


def gate_bits(z, act):
    """rn_bn_segment.act_mask as rn_bn_apply writes it for the stored z [P, C]: bit (c & 7) of byte (p C + c) / 8"""
    on = act_deriv(np.asarray(z, dtype=np.float32), act, np.float32).astype(np.uint8).reshape(-1, 8)
    return (on << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8)


def bn_variable_scopes(graph):
    """{scope: set of BatchNorm variable names} from the graph's own BatchNorm table (not from a name pattern):
    scope = 'fpn' | 'head' | 'backbone' by the layer's top-level name, the split the reference's freeze keys make"""
    out = {"backbone": set(), "fpn": set(), "head": set()}
    for bn in graph.bns:
        scope = "fpn" if bn.startswith("fpn") else "head" if bn.startswith(("box-head", "class-head")) else "backbone"
        for sfx in ("/gamma", "/beta", "/moving_mean", "/moving_variance"):
            if bn + sfx in graph.var_specs:
                out[scope].add(bn + sfx)
    return out
