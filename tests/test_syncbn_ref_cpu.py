"""The SyncBN reference (syncbn_ref.py) is right, and the inputs of tests/test_gpu_syncbn_kernels.py discriminate.

  * the reference's dy, dgamma, dbeta equal float64 autograd of a plain BatchNorm over the concatenated batch;
  * a kernel that ignores count_scale (the all-reduced sums divided by the local P) and a kernel that normalises every
    shard by its own statistics miss every acceptance bound of the fwd table, of moving_var and of dy by at least 10x on
    every ordinary channel of the shared inputs;
  * an fp32 transcription of the kernels' formulas, fed the float64 fwd table rounded to float32, differs from the
    float64 evaluation of the same table on less than HALF of each mismatch-share cap — so the caps leave room for the
    kernels' own fp32 arithmetic and for nothing else."""
import numpy as np
import pytest
import torch

import act_ref as A
import syncbn_ref as S

F64 = S.F64
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


# ---- the reference against autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("replicas", [1, 2, 3])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_reference_equals_autograd_of_batchnorm_over_the_concatenation(act, replicas):
    segs = S.make_inputs([(37, 24)], replicas, torch.bfloat16, 5 + replicas)
    s = segs[0]
    ref = S.reference(s["ys"], s["gamma"], s["beta"], S.EPS, S.MOMENTUM, 1, None, dzs=s["dzs"], act=act)
    y = torch.cat([t.to(F64) for t in s["ys"]]).requires_grad_(True)
    gam, bet = s["gamma"].to(F64).requires_grad_(True), s["beta"].to(F64).requires_grad_(True)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    v = (y - mean) / torch.sqrt(var + S.EPS) * gam + bet
    z = torch.relu(v) if act == "relu" else v
    (z * torch.cat([t.to(F64) for t in s["dzs"]])).sum().backward()
    for name, got, want in (("dy", torch.cat(ref["dy"]), y.grad), ("dgamma", ref["sum_gx"], gam.grad),
                            ("dbeta", ref["sum_g"], bet.grad), ("z", torch.cat(ref["z"]), z.detach())):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"{name} act={act} R={replicas}: max error / max value = {err:.3e}")
        assert err <= 1e-12, (name, err)
    # local sums add up to the global ones, and each is the sum over that shard's rows only
    for r in range(replicas):
        assert torch.equal(ref["local_sums"][r][0], ref["g"][r].sum(0))


def test_moving_variance_correction_and_its_guard():
    y = [torch.tensor([[1.0, 3.0]]), torch.tensor([[2.0, 7.0]])]
    one = torch.ones((2,))
    ref = S.reference(y, one, one, 1e-3, 0.5, 1, None, mm=one * 0, mv=one * 0)
    assert torch.allclose(ref["mv"], torch.tensor([0.25, 4.0], dtype=F64) * 2 * 0.5)        # n = 2: factor 2
    ref = S.reference(y[:1], one, one, 1e-3, 0.5, 1, None, mm=one * 0, mv=one * 0)
    assert torch.equal(ref["mv"], torch.zeros((2,), dtype=F64))                               # n = 1: the guard, no 0 / 0


# ---- discrimination -------------------------------------------------------------------------------------------------------
def _inputs(dtype, replicas):
    return S.make_inputs(S.SEGMENTS, replicas, dtype, 100 + replicas)


def _ref(s, dtype, act, use_res, bessel, acc, **kw):
    return S.reference(s["ys"], s["gamma"], s["beta"], S.EPS, S.MOMENTUM, bessel, dtype,
                       residuals=s["res"] if use_res else None, dzs=s["dzs"], act=act, mm=s["mm"], mv=s["mv"],
                       dres0=s["dres0"], accumulate=bool(acc), **kw)


@pytest.mark.parametrize("form", S.FORMS, ids=[f[0] for f in S.FORMS])
@pytest.mark.parametrize("replicas", S.REPLICAS)
@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_a_kernel_without_count_scale_or_with_local_statistics_cannot_pass(build, replicas, form):
    """Both wrong kernels against the float64 reference, per ordinary channel: every fwd row, moving_var and dy at least
    10x outside the bound the GPU test applies.  The locally normalised kernel is judged per channel on the shard where it
    is furthest off (the GPU test checks every shard; one shard's sample variance can equal the global one by chance), and
    a channel whose every relu gate is shut has dy = 0 in any kernel and says nothing.  dy is judged the way that test
    judges it — the largest error of the channel over one storage step in the top binade of the channel's dy — with one
    exception that is arithmetic, not
    input choice: with one row per shard a locally normalised shard has xhat = 0 and g - sum g / 1 = 0, so its dy is
    exactly 0, while the true dy of a two- or three-row batch is itself only O(eps / var) of its terms; there the share
    of elements that differ (all of them) is what is 10x over its cap."""
    dtype = DTYPES[build]
    _, act, use_res, bessel, acc = form
    worst = {}
    for s in _inputs(dtype, replicas):
        P, C, k0 = s["P"], s["C"], S.special(s["C"])
        right = _ref(s, dtype, act, use_res, bessel, acc)
        wrong_n = _ref(s, dtype, act, use_res, bessel, acc, n_override=P)
        local = [_ref({k: ([v[r]] if isinstance(v, list) else v) for k, v in s.items()}, dtype, act, use_res, bessel, acc)
                 for r in range(replicas)]
        step = S.step_top(S.rs(torch.cat(right["dy"]), dtype), dtype)
        # per ordinary channel: violation / bound of the wrong-n kernel, and of the local kernel on the shard where it is
        # largest (the GPU test checks every shard, so one shard outside is a failure; a single shard's local variance
        # can come close to the global one by chance, all of them cannot)
        viol = {"wrong-n": {}, "local": {}}
        for row in S.FWD_ROWS + ("mv",):
            tol = S.MOVING_TOL if row == "mv" else S.FWD_TOL[row]
            viol["wrong-n"][row] = S.tol_ratio(wrong_n[row], right[row], tol)
            viol["local"][row] = torch.stack([S.tol_ratio(w[row], right[row], tol) for w in local]).max(0).values
        viol["wrong-n"]["dy"] = (torch.cat(wrong_n["dy"]) - torch.cat(right["dy"])).abs().max(0).values / step
        live = torch.cat(right["g"]).abs().max(0).values > 0       # a channel whose every gate is shut has dy = 0 in any kernel
        if P == 1:
            # (see the docstring) the share of differing elements over its cap instead of the error over the step
            differ = torch.stack([S.rs(w["dy"][0], dtype) != S.rs(right["dy"][r], dtype) for r, w in enumerate(local)])
            assert all(bool((w["dy"][0] == 0).all()) for w in local)
            viol["local"]["dy"] = differ.to(F64).mean((0, 1)) / S.CAPS["dy"]
        else:
            viol["local"]["dy"] = torch.stack([(w["dy"][0] - right["dy"][r]).abs().max(0).values
                                               for r, w in enumerate(local)]).max(0).values / step
        for name, rows in viol.items():
            for row, ratio in rows.items():
                kept = ratio[k0:][live[k0:]] if row == "dy" else ratio[k0:]
                least = float(kept.min()) if kept.numel() else 1e300
                worst[f"{name} {row}"] = min(worst.get(f"{name} {row}", 1e300), least)
                assert least >= 10.0, (name, row, (P, C), least)
    print(f"{build} R={replicas} {form[0]}: smallest violation / bound over both wrong kernels, all ordinary channels: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- the float32 model against the mismatch-share caps ----------------------------------------------------------------------
def _fp32_model(s, r, tab, bs, n, act, use_res, acc, dtype):
    """the kernels' formulas in float32 (numpy: separate multiply and add, a true division in the sigmoid), the storage
    roundings where rn_bn_apply / rn_bn_bwd_apply have them.  tab: float32 fwd table [4, C]; bs: float32 global sums."""
    f = np.float32
    y, dz = s["ys"][r].float().numpy(), s["dzs"][r].float().numpy()
    mean, istd, sc, sh = (tab[i].numpy() for i in range(4))
    rb = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype).float().numpy()      # noqa: E731
    u = y * sc + sh
    o = u
    if use_res or act == "swish":
        o = rb(o)
    if use_res:
        o = o + s["res"][r].float().numpy()
        if act == "swish":
            o = rb(o)
    v = o
    if act == "relu":
        o = np.maximum(o, f(0))
    elif act == "swish":
        o = o * A.fp32_sigmoid(o)
    z = rb(o)
    if act == "relu":
        g = np.where(z > 0, dz, f(0))
    elif act == "swish":
        x = v if use_res else u
        sg = A.fp32_sigmoid(x)
        g = dz * (sg + x * sg * (f(1) - sg))
    else:
        g = dz
    inv_n = f(1.0 / n)
    k1, k2 = bs[0].numpy() * inv_n, bs[1].numpy() * inv_n
    xh = (y - mean) * istd
    dy = rb(sc * (g - k1 - xh * k2))
    dres = rb(g + (s["dres0"][r].float().numpy() if acc else f(0)))
    return {k: torch.from_numpy(a).to(F64) for k, a in (("z", z), ("dy", dy), ("dres", dres))}


@pytest.mark.parametrize("form", S.FORMS, ids=[f[0] for f in S.FORMS])
@pytest.mark.parametrize("replicas", S.REPLICAS)
@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_float32_arithmetic_alone_stays_under_half_of_each_mismatch_cap(build, replicas, form):
    dtype = DTYPES[build]
    _, act, use_res, bessel, acc = form
    counts = {}
    for s in _inputs(dtype, replicas):
        right = _ref(s, dtype, act, use_res, bessel, acc)
        tab = torch.stack([right[k] for k in S.FWD_ROWS]).float()
        bs = torch.stack([right["sum_g"], right["sum_gx"]]).float()
        n = replicas * s["P"]
        for r in range(replicas):
            model = _fp32_model(s, r, tab, bs, n, act, use_res, acc, dtype)
            want = S.from_table(s["ys"][r], s["dzs"][r], s["res"][r] if use_res else None, s["dres0"][r], tab, bs, n, act,
                                acc, dtype, z_stored=model["z"])
            for k in S.CAPS:
                if k == "dres" and not use_res:
                    continue
                # (the element-wise rule of the GPU test holds for the model too)
                assert bool(((model[k] - want[k]).abs() <= want["bound"][k]).all()), (k, (s["P"], s["C"]), r)
                counts.setdefault((k, r), []).append(S.mismatches(model[k], want[k]))
    worst = {k: 0.0 for k in S.CAPS}
    for (k, r), c in counts.items():
        sh = S.worst_share(c)
        worst[k] = max(worst[k], sh / S.CAPS[k])
        assert sh < 0.5 * S.CAPS[k], (k, r, sh, c)
    print(f"{build} R={replicas} {form[0]}: largest share / cap of the float32 model: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("replicas", S.REPLICAS)
@pytest.mark.parametrize("build", ["bf16", "f16"])
def test_float32_sums_alone_stay_under_half_of_the_table_bounds(build, replicas):
    """`sums` is a float32 tensor and the all-reduce adds R of them in float32: a kernel whose own sums were exact would
    still hand rn_bn_finalize these values.  On the ordinary channels of the chosen inputs (a two-row batch included:
    var = (y0 - y1)^2 / 4 out of E[y^2] - mean^2) that alone must use less than half of every fwd-table bound."""
    dtype = DTYPES[build]
    worst = {}
    for s in _inputs(dtype, replicas):
        k0 = S.special(s["C"])
        right = S.stats(s["ys"], s["gamma"], s["beta"], S.EPS)
        total = None
        for y in s["ys"]:
            part = torch.stack([y.to(F64).sum(0), (y.to(F64) ** 2).sum(0)]).float()
            total = part if total is None else total + part
        n = right["n"]
        mean = total[0].to(F64) / n
        var = (total[1].to(F64) / n - mean * mean).clamp_min(0.0)
        invstd = (1.0 / torch.sqrt(var + S.EPS)).float()
        scale = s["gamma"] * invstd
        got = {"mean": mean.float(), "invstd": invstd, "scale": scale, "shift": s["beta"] - mean.float() * scale}
        for row in S.FWD_ROWS:
            ratio = float(S.tol_ratio(got[row], right[row], S.FWD_TOL[row])[k0:].max())
            worst[row] = max(worst.get(row, 0.0), ratio)
            assert ratio < 0.5, (row, (s["P"], s["C"]), ratio)
    print(f"{build} R={replicas}: largest error / bound of exact sums passed through float32: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
