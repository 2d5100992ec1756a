"""The BatchNorm passes in their SyncBatchNormalization form — rn_bn_stats, all-reduce of `sums`, rn_bn_finalize,
rn_bn_apply, rn_bn_bwd_reduce, all-reduce of `bsums`, rn_bn_bwd_apply with bessel = 0 / 1 and count_scale = replicas —
against float64 (syncbn_ref.py) on ONE device: a replica is a shard of rows with its own rn_bn_problem and buffers, an
all-reduce is the float32 sum of the shards' tensors in rank order, copied back into every shard.

Acceptance (the kernel-level rule of test_gpu_bench_shapes_more.py::_check_bn_problem, so that both configurations
are held to one standard):
  fwd table, ordinary channels   mean rtol 1e-5 / atol 1e-5, invstd and scale rtol 2e-5, shift rtol 1e-4 / atol 2e-5
                                 against the float64 statistics of the CONCATENATION
  moving statistics              rtol 1e-5 / atol 1e-5 against old m + new (1 - m), the n / (n - 1) factor at n = R P
  z, dy, dres                    recomputed in float64 from the kernel's own float32 table and all-reduced bsums: every
                                 element within one storage step of the top binade of its channel (plus the fp32
                                 evaluation error of dy where its terms cancel: syncbn_ref.element_bound), the share of
                                 elements that differ at all under 0.02 / 0.03 / 0.01 (syncbn_ref.worst_share), relu
                                 gates and mask bits bit for bit
  sums                           every shard's bsums BEFORE the all-reduce and its dgamma / dbeta = that shard's LOCAL
                                 float64 sums (rtol 1e-4, atol 2e-5 max + 1e-6, plus for swish the uncertainty its
                                 gate inherits from the fp32 u: syncbn_ref.from_table); dgamma / dbeta keep those
                                 bits afterwards

The special channels (syncbn_ref.make_inputs: var = 0, var = 0 locally only, mean 64, all zero) have a DERIVED bound.
Stage 1 of rn_bn_stats adds y and y^2 in float32 along a chain of at most m = ceil(rows_per_chunk / RL) + RL terms (RL row
lanes of a slab: a lane's rows, then the RL lane sums in order; y^2 of a 16-bit value is exact in float32); everything
after that is double, and the result is stored as float32.  m - 1 additions and one conversion are off by at most
2^-24 of the sum of their (non-negative) terms each, so
    |E[y^2]' - E[y^2]| <= (m + 2) 2^-24 E[y^2],      |mean' - mean| <= (m + 2) 2^-24 sqrt(E[y^2])
(the 2 spare units cover the float32 adds of the all-reduce for R <= 3 in the worst case and for every R in practice:
the printed ratios show it).  With var = E[y^2] - mean^2 the kernel's var is off by at most dvar = (m + 2) 2^-24 E[y^2]
(the mean term is second order next to it where it matters), hence
    invstd   relative dvar / (2 (var + eps)) + 2^-24      (the table is float32: one rounding of the stored value —
                                                           without it the bound of the all-zero channel would be 0)
    scale    one more 2^-24 (the product gamma invstd)
    mean     (m + 2) 2^-24 sqrt(E[y^2]) + 2^-24 |mean|
    shift    |mean| dscale + |scale| dmean + 3 2^-24 (|beta| + |mean scale|)
    moving   the ordinary bound plus (1 - momentum) times dvar c / dmean.
var is never negative in effect: invstd <= float32(1 / sqrt(eps)) exactly on channels 0 and 3.  m is computed here from
the formulas of bn_chunks_of / bn_slab_plan (csrc/rn_train.hip).

Every test prints its worst error / bound per family, and where, before it asserts.  The figures of the kernels as
of this file's first version, on an MI355X, largest over both builds (a later change to the reductions reads its room
from them):
  shards (R = 2, 3, 8, five forms)   fwd 0.05, fwd special 0.40, moving 0.14, moving special 0.09, local sums 0.11,
                                     z 1.00, dy 1.00, dres 0.00 (1.00 = one storage step), share z 0.12, dy 0.06, dres 0.00
  one replica, bessel = 1            fwd 0.07, fwd special 0.44, moving 0.05, z 1.00, dy 0.06, share z 0.05
  513 chunks, R = 2                  fwd 0.04, fwd special 0.15, moving 0.06, moving special 0.08, z 0.50, dy 1.00
  identical shards                   exact; fwd 0.07, fwd special 0.44, moving 0.05 against float64
  shards vs concatenation            fwd 0.04, between forms fwd 0.03, moving 0.08, share of dy 0.43
  conv-epilogue partials             fwd 0.01, moving 0.01, z 0.25
  data-gradient partials             fwd 0.04, moving 0.06, local sums 0.00, z 0.50, dy 0.00
  dy column sums                     column sums 0.02, dy 0.02"""
import ctypes
import math

import pytest
import torch

import syncbn_ref as S

pytestmark = pytest.mark.gpu

H16 = torch.bfloat16
_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BUILDS = ["bf16", "f16"]
F64 = S.F64
U24 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _storage_type(request):
    global H16
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    H16 = _DT[params.get("build", "bf16")]
    yield
    H16 = torch.bfloat16


def _lib():
    from retinanet import _C
    return _C.lib(H16 == torch.float16)


# ---- the reduction plan of csrc/rn_train.hip (bn_chunks_of, bn_slab_plan) ----------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _chunks(P, C):
    want = max(256, 2048 // _cdiv(C, 64))
    rpc = max(32, _cdiv(_cdiv(P, want), 32) * 32)
    return _cdiv(P, rpc), rpc


def _slab_groups(C8, chunks):
    old_n = _cdiv(C8, 8)
    if C8 >= 8 and C8 / (8.0 * old_n) >= 0.95:
        return 8
    score = lambda n: C8 * (256 // _cdiv(C8, n)) / (n * 256.0)        # noqa: E731
    ok = [n for n in range(1, old_n + 1) if not (_cdiv(C8, n) > 64 or (_cdiv(C8, n) < 8 and n > 1))]
    best = max([score(n) for n in ok] + [0.0])
    for n in ok:
        if score(n) >= best - 0.01 and (chunks * n >= 512 or C8 < 8):
            return _cdiv(C8, n)
    return min(C8, 8)


def _chain_terms(P, C):
    chunks, rpc = _chunks(P, C)
    rl = 256 // _slab_groups(C // 8, chunks)
    return _cdiv(rpc, rl) + rl


# ---- one rn_bn_problem per shard ------------------------------------------------------------------------------------------
class _Shard:
    def __init__(self, p, T, ws):
        self.p, self.T, self.ws = p, T, ws


def _shard(cuda, segs, r, act, use_res, bessel, acc, count_scale):
    """shard r of `segs` (syncbn_ref.make_inputs) with buffers of its own.  A relu behind a residual add gets the bit mask."""
    from retinanet import _C
    p = _C.BnProblem()
    p.num_segments, p.act, p.bessel, p.eps, p.momentum = len(segs), _C.ACT_IDS[act], bessel, S.EPS, S.MOMENTUM
    p.count_scale = count_scale
    T = []
    for i, s in enumerate(segs):
        P, C = s["P"], s["C"]
        t = {"y": s["ys"][r].to(cuda).contiguous(), "dz": s["dzs"][r].to(cuda).contiguous(),
             "res": s["res"][r].to(cuda).contiguous() if use_res else None,
             "dres": s["dres0"][r].to(cuda).clone() if use_res else None, "dres0": s["dres0"][r]}
        t["z"], t["dy"] = torch.full_like(t["y"], 7.0), torch.full_like(t["y"], 7.0)
        t["mask"] = torch.full((P * C // 8,), 0xA5, dtype=torch.uint8, device=cuda) if use_res and act == "relu" else None
        for k, rows in (("sums", 2), ("bsums", 2), ("fwd", 4)):
            t[k] = torch.zeros((rows, C), dtype=torch.float32, device=cuda)
        t["dgamma"], t["dbeta"] = torch.zeros((C,), device=cuda), torch.zeros((C,), device=cuda)
        for k in ("gamma", "beta", "mm", "mv"):
            t[k] = s[k].to(cuda).float().clone()
        t["mm0"], t["mv0"] = s["mm"], s["mv"]
        d = p.seg[i]
        d.y, d.z, d.dz, d.dy = t["y"].data_ptr(), t["z"].data_ptr(), t["dz"].data_ptr(), t["dy"].data_ptr()
        d.residual = None if t["res"] is None else t["res"].data_ptr()
        d.dres = None if t["dres"] is None else t["dres"].data_ptr()
        d.act_mask = None if t["mask"] is None else t["mask"].data_ptr()
        d.sums, d.bsums, d.fwd = t["sums"].data_ptr(), t["bsums"].data_ptr(), t["fwd"].data_ptr()
        d.gamma, d.beta, d.moving_mean, d.moving_var = (t["gamma"].data_ptr(), t["beta"].data_ptr(), t["mm"].data_ptr(),
                                                        t["mv"].data_ptr())
        d.dgamma, d.dbeta = t["dgamma"].data_ptr(), t["dbeta"].data_ptr()
        d.P, d.C, d.dres_accumulate = P, C, int(bool(acc))
        T.append(t)
    return _Shard(p, T, _workspace(p, cuda))


def _workspace(p, cuda):
    # zeros: the ticket counters of the split stage-2 reduction start at zero
    return torch.zeros((max(int(_lib().rn_bn_workspace_bytes(ctypes.byref(p))), 256),), dtype=torch.uint8, device=cuda)


def _allreduce(tensors, tree=False):
    """the sum of the shards' float32 tensors, copied back into every shard.  Rank order (one running sum); tree = pairwise,
    for the exact identities: R identical addends then add up without a rounding."""
    if tree:
        level = [t.clone() for t in tensors]
        while len(level) > 1:
            assert len(level) % 2 == 0
            level = [level[i] + level[i + 1] for i in range(0, len(level), 2)]
        total = level[0]
    else:
        total = tensors[0].clone()
        for t in tensors[1:]:
            total += t
    for t in tensors:
        t.copy_(total)


def _call(fn, sh, name, with_ws):
    from retinanet import _C
    st = _C.current_stream()
    lib = _lib()
    args = (ctypes.byref(sh.p), _C.ptr(sh.ws), sh.ws.numel(), st) if with_ws else (ctypes.byref(sh.p), st)
    _C.check(getattr(lib, fn)(*args), name)


def _forward(shards, tree=False, stats=True):
    if stats:
        for sh in shards:
            _call("rn_bn_stats", sh, "rn_bn_stats", True)
    for i in range(len(shards[0].T)):
        _allreduce([sh.T[i]["sums"] for sh in shards], tree)
    for sh in shards:
        _call("rn_bn_finalize", sh, "rn_bn_finalize", False)
        _call("rn_bn_apply", sh, "rn_bn_apply", False)
    torch.cuda.synchronize()
    for sh in shards:
        for t in sh.T:
            t["z_kept"] = t["z"].clone()
            if t["mask"] is not None:
                t["z"].fill_(float("nan"))       # with the bit mask the backward passes must not look at z


def _backward(shards, tree=False):
    for sh in shards:
        _call("rn_bn_bwd_reduce", sh, "rn_bn_bwd_reduce", True)
    torch.cuda.synchronize()
    for sh in shards:
        for t in sh.T:
            t["local"] = {k: t[k].clone() for k in ("bsums", "dgamma", "dbeta")}
    for i in range(len(shards[0].T)):
        _allreduce([sh.T[i]["bsums"] for sh in shards], tree)
    for sh in shards:
        _call("rn_bn_bwd_apply", sh, "rn_bn_bwd_apply", False)
    torch.cuda.synchronize()


# ---- the checks -------------------------------------------------------------------------------------------------------------
class _Report:
    """worst error / bound per family, where it occurred, and every miss"""

    def __init__(self, what):
        self.what, self.worst, self.missed = what, {}, []

    def add(self, family, ratio, where):
        ratio = torch.as_tensor(ratio, dtype=F64).reshape(-1)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        if ratio.numel() == 0:
            return
        k = int(ratio.argmax())
        v = float(ratio[k])
        if v > self.worst.get(family, (-1.0, None))[0]:
            self.worst[family] = (v, f"{where} index {k}")
        if v > 1.0:
            self.missed.append((family, where, "error / bound", v, "index", k))

    def finish(self):
        build = "f16" if H16 == torch.float16 else "bf16"
        print(f"{self.what} [{build}] worst error / bound: "
              + "; ".join(f"{k} {v:.4f} ({w})" for k, (v, w) in sorted(self.worst.items())))
        assert not self.missed, self.missed[:12]


def _special_bounds(ref, P, C, gamma, beta):
    """derived bounds of the fwd rows (module docstring), per channel; dvar and dmean with them"""
    m = _chain_terms(P, C)
    dvar = (m + 2) * U24 * ref["ey2"]
    dmean = (m + 2) * U24 * torch.sqrt(ref["ey2"]) + U24 * ref["mean"].abs()
    rel = dvar / (2.0 * (ref["var"] + S.EPS)) + U24
    dscale = (rel + U24) * ref["scale"].abs()
    dshift = (ref["mean"].abs() * dscale + ref["scale"].abs() * dmean
              + 3 * U24 * (beta.to(F64).abs() + (ref["mean"] * ref["scale"]).abs()))
    return {"mean": dmean, "invstd": rel * ref["invstd"], "scale": dscale, "shift": dshift, "dvar": dvar, "dmean": dmean}


def _check_forward_tables(rep, shards, segs_ref, replicas, bessel, same_table=True, no_special=False):
    """fwd table and moving statistics of every shard and segment against the float64 statistics of the concatenation.
    Returns the per-segment reference statistics.  no_special: every channel is an ordinary one (y is not make_inputs')."""
    refs = []
    for i, t0 in enumerate(shards[0].T):
        P, C = t0["y"].shape
        k0 = 0 if no_special else S.special(C)
        ys = segs_ref[i]
        ref = S.stats(ys, t0["gamma"].cpu(), t0["beta"].cpu(), S.EPS)
        assert ref["n"] == sum(y.shape[0] for y in ys)
        mm, mv = S.moving(t0["mm0"], t0["mv0"], ref["mean"], ref["var"], ref["n"], S.MOMENTUM, bessel)
        sb = _special_bounds(ref, P, C, t0["gamma"].cpu(), t0["beta"].cpu())
        corr = ref["n"] / (ref["n"] - 1.0) if bessel and ref["n"] > 1 else 1.0
        for r, sh in enumerate(shards):
            t = sh.T[i]
            where = f"segment {P}x{C} shard {r}"
            tab = t["fwd"].cpu().to(F64)
            if same_table and r:
                assert torch.equal(t["fwd"], t0["fwd"]), (where, "every replica finalizes the same sums")
            for j, row in enumerate(S.FWD_ROWS):
                rep.add(f"fwd {row}", S.tol_ratio(tab[j], ref[row], S.FWD_TOL[row])[k0:], where)
                rep.add(f"fwd {row} special", ((tab[j] - ref[row]).abs() / sb[row].clamp_min(1e-300))[:k0], where)
            if k0:
                cap = torch.tensor(1.0 / math.sqrt(S.EPS), dtype=F64).float()          # float32(1 / sqrt(eps))
                assert bool((t["fwd"][1, [0, 3]].cpu() <= cap).all()), (where, "var below 0", t["fwd"][1, :4].tolist())
            tol_m = S.MOVING_TOL[1] + S.MOVING_TOL[0] * mm.abs()
            tol_v = S.MOVING_TOL[1] + S.MOVING_TOL[0] * mv.abs()
            extra_m, extra_v = (1 - S.MOMENTUM) * sb["dmean"], (1 - S.MOMENTUM) * corr * sb["dvar"]
            em, ev = (t["mm"].cpu().to(F64) - mm).abs(), (t["mv"].cpu().to(F64) - mv).abs()
            rep.add("moving_mean", (em / tol_m)[k0:], where)
            rep.add("moving_var", (ev / tol_v)[k0:], where)
            rep.add("moving_mean special", (em / (tol_m + extra_m))[:k0], where)
            rep.add("moving_var special", (ev / (tol_v + extra_v))[:k0], where)
        refs.append(ref)
    return refs


def _mask_bits(mask, shape):
    return ((mask.cpu().view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).reshape(shape)


def _check_elements(rep, shards, replicas, act, acc, backward=True):
    """z, dy, dres of every shard from the kernel's own table and all-reduced sums; the local sums; the gates"""
    for r, sh in enumerate(shards):
        counts = {k: [] for k in S.CAPS}
        for t in sh.T:
            P, C = t["y"].shape
            where = f"segment {P}x{C} shard {r}"
            n = replicas * P
            z = t["z_kept"].cpu()
            res = None if t["res"] is None else t["res"].cpu()
            want = S.from_table(t["y"].cpu(), t["dz"].cpu(), res, t["dres0"], t["fwd"].cpu(), t["bsums"].cpu(), n, act,
                                acc, H16, z_stored=z)
            got = {"z": z.to(F64), "dy": t["dy"].cpu().to(F64)}
            if t["dres"] is not None:
                got["dres"] = t["dres"].cpu().to(F64)
            if t["mask"] is not None:
                assert torch.equal(_mask_bits(t["mask"], z.shape), (z.float() > 0).to(torch.uint8)), (where, "mask bits")
            for k in got if backward else ("z",):
                rep.add(k, (got[k] - want[k]).abs() / want["bound"][k].clamp_min(1e-300), where)
                counts[k].append(S.mismatches(got[k], want[k]))
            if not backward:
                continue
            # the shard's own sums: bsums before the all-reduce, dgamma / dbeta before and after it
            loc = t["local"]
            for j, (term, name, sl) in enumerate(((want["g"], "dbeta", want["gslack"]),
                                                  (want["g"] * want["xhat"], "dgamma", want["gslack"] * want["xhat"].abs()))):
                ref = term.sum(0)
                # (+ what a swish gate inherits from its fp32 argument, summed over the rows: syncbn_ref.from_table)
                tol = (1e-4, 2e-5 * float(ref.abs().max()) + 1e-6 + sl.sum(0))
                rep.add("local bsums", S.tol_ratio(loc["bsums"][j].cpu(), ref, tol), where)
                rep.add(f"local {name}", S.tol_ratio(loc[name].cpu(), ref, tol), where)
                assert torch.equal(loc[name].view(torch.int32), loc["bsums"][j].view(torch.int32)), (where, name)
                assert torch.equal(t[name].view(torch.int32), loc[name].view(torch.int32)), (where, name, "after the all-reduce")
        for k, c in counts.items():
            if c:
                rep.add(f"share {k}", S.worst_share(c) / S.CAPS[k], f"shard {r}")


def _run(cuda, segs, replicas, act, use_res, bessel, acc, what):
    shards = [_shard(cuda, segs, r, act, use_res, bessel, acc, float(replicas)) for r in range(replicas)]
    _forward(shards)
    _backward(shards)
    rep = _Report(what)
    _check_forward_tables(rep, shards, [s["ys"] for s in segs], replicas, bessel)
    _check_elements(rep, shards, replicas, act, acc)
    rep.finish()
    return shards


def _inputs(replicas, shapes=S.SEGMENTS):
    key = (H16, replicas, tuple(shapes))
    if key not in _inputs.cache:
        _inputs.cache[key] = S.make_inputs(shapes, replicas, H16, 100 + replicas)
    return _inputs.cache[key]


_inputs.cache = {}


# ---- replicas as shards ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", S.FORMS, ids=[f[0] for f in S.FORMS])
@pytest.mark.parametrize("replicas", S.REPLICAS)
@pytest.mark.parametrize("build", BUILDS)
def test_syncbn_passes_on_shards(cuda, build, replicas, form):
    """five segments in one problem per shard: 126 x 64 (four 32-row chunks, the last a 30-row tail), 25 x 256, 48 x 8 (one
    channel group, 256 row lanes), 36 x 144 (18 groups: grid-stride elementwise form, a partial last slab), 1 x 16 (one
    row per shard: n = R)"""
    name, act, use_res, bessel, acc = form
    assert [_chunks(P, C)[0] for P, C in S.SEGMENTS] == [4, 1, 2, 2, 1]
    _run(cuda, _inputs(replicas), replicas, act, use_res, bessel, acc, f"shards R={replicas} {name}")


@pytest.mark.parametrize("build", BUILDS)
def test_single_replica_single_row_takes_the_variance_guard(cuda, build):
    """R = 1, P = 1 (the 1 x 16 segment) with bessel = 1: n = 1, the n > 1 guard must write the uncorrected variance (0)
    instead of 0 / 0; the other segments get n / (n - 1) at n = P"""
    _run(cuda, _inputs(1), 1, "none", False, 1, 0, "one replica, bessel = 1")


@pytest.mark.parametrize("form", [S.FORMS[0], S.FORMS[3]], ids=[S.FORMS[0][0], S.FORMS[3][0]])
@pytest.mark.parametrize("build", BUILDS)
def test_syncbn_split_stage2_reduction_then_separate_finalize(cuda, build, form):
    """16416 x 64 per shard, R = 2: 513 row chunks, so stage 2 of both reductions runs in parts with the ticket hand-off and
    the forward one is followed by the SEPARATE rn_bn_finalize on the all-reduced sums"""
    name, act, use_res, bessel, acc = form
    assert _chunks(*S.BIG_SEGMENT)[0] == 513
    _run(cuda, _inputs(2, [S.BIG_SEGMENT]), 2, act, use_res, bessel, acc, f"513 chunks R=2 {name}")


# ---- exact identities -----------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _outputs(shard):
    keys = ["fwd", "mm", "mv", "z_kept", "dy", "dres", "bsums"]
    return [{k: t[k].clone() for k in keys if t[k] is not None} for t in shard.T]


def _replicate(segs, replicas):
    return [{k: (v * replicas if isinstance(v, list) else v) for k, v in s.items()} for s in segs]


@pytest.mark.parametrize("bessel", [0, 1])
@pytest.mark.parametrize("replicas", [2, 8])
@pytest.mark.parametrize("build", BUILDS)
def test_identical_shards_give_the_bits_of_one_shard(cuda, build, replicas, bessel):
    """R identical shards, count_scale = R, pairwise all-reduce: the float32 sums are R times those of one shard without a
    rounding and 1 / (R P) is 1 / P scaled by a power of two, so with bessel = 0 every output of every shard has the BITS
    of the single-shard run with count_scale = 1 — any site that reads P where it should read P count_scale breaks that.
    With bessel = 1 only moving_var may differ (n / (n - 1) at n = R P): it is held to the formula."""
    rep = _Report(f"identical shards R={replicas} bessel={bessel}")
    for name, act, use_res, _, acc in (S.FORMS[0], S.FORMS[4]):
        one = _inputs(1)
        single = _shard(cuda, one, 0, act, use_res, bessel, acc, 1.0)
        _forward([single])
        _backward([single])
        base = _outputs(single)
        segs = _replicate(one, replicas)
        shards = [_shard(cuda, segs, r, act, use_res, bessel, acc, float(replicas)) for r in range(replicas)]
        _forward(shards, tree=True)
        _backward(shards, tree=True)
        for r, sh in enumerate(shards):
            for i, (a, b) in enumerate(zip(base, _outputs(sh))):
                for k in a:
                    if k == "bsums" or (k == "mv" and bessel):
                        continue
                    assert torch.equal(_bits(a[k]), _bits(b[k])), (name, "shard", r, "segment", i, k)
                assert torch.equal(_bits(b["bsums"]), _bits(a["bsums"] * float(replicas))), (name, r, i, "bsums")
        _check_forward_tables(rep, shards, [s["ys"] for s in segs], replicas, bessel)
    rep.finish()


@pytest.mark.parametrize("build", BUILDS)
def test_count_scale_zero_or_negative_is_one(cuda, build):
    """bn_fill's default: count_scale <= 0 reads as 1 in all three sites (finalize, moving statistics, rn_bn_bwd_apply)"""
    name, act, use_res, bessel, acc = S.FORMS[0]
    outs = []
    for cs in (1.0, 0.0, -3.0):
        sh = _shard(cuda, _inputs(1), 0, act, use_res, bessel, acc, cs)
        _forward([sh])
        _backward([sh])
        outs.append(_outputs(sh))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            for k in a:
                assert torch.equal(_bits(a[k]), _bits(b[k])), k


# ---- shards against one problem over the concatenation ------------------------------------------------------------------------
@pytest.mark.parametrize("bessel", [0, 1])
@pytest.mark.parametrize("build", BUILDS)
def test_shards_agree_with_one_problem_over_the_concatenated_rows(cuda, build, bessel):
    """R = 3 shards with count_scale = 3 against ONE problem of 3 P rows with count_scale = 1: the same batch, another
    summation order.  Both fwd tables and moving statistics inside the bounds (against float64 and against each other);
    the share of dy elements that differ between the two forms under the 0.03 cap."""
    replicas = 3
    name, act, use_res, _, acc = S.FORMS[2]
    segs = _inputs(replicas)
    shards = [_shard(cuda, segs, r, act, use_res, bessel, acc, float(replicas)) for r in range(replicas)]
    _forward(shards)
    _backward(shards)
    cat = [{k: ([torch.cat(v)] if isinstance(v, list) else v) for k, v in s.items()} for s in segs]
    for s in cat:
        s["P"] = s["ys"][0].shape[0]
    whole = _shard(cuda, cat, 0, act, use_res, bessel, acc, 1.0)
    _forward([whole])
    _backward([whole])
    rep = _Report(f"shards vs concatenation bessel={bessel}")
    _check_forward_tables(rep, shards, [s["ys"] for s in segs], replicas, bessel)
    # (the concatenated problem has other chunks: its special channels are held to ITS chain length)
    _check_forward_tables(rep, [whole], [s["ys"] for s in segs], 1, bessel)
    counts = []
    for i, tw in enumerate(whole.T):
        P, C = segs[i]["P"], segs[i]["C"]
        k0 = S.special(C)
        ts = shards[0].T[i]
        for j, row in enumerate(S.FWD_ROWS):
            rep.add(f"between forms fwd {row}", S.tol_ratio(tw["fwd"][j].cpu(), ts["fwd"][j].cpu().to(F64), S.FWD_TOL[row])[k0:],
                    f"segment {P}x{C}")
        for k in ("mm", "mv"):
            rep.add(f"between forms {k}", S.tol_ratio(tw[k].cpu(), ts[k].cpu().to(F64), S.MOVING_TOL)[k0:], f"segment {P}x{C}")
        dy_shards = torch.cat([sh.T[i]["dy"] for sh in shards]).cpu().to(F64)
        counts.append(S.mismatches(tw["dy"].cpu(), dy_shards))
    rep.add("between forms share dy", S.worst_share(counts) / S.CAPS["dy"], "all segments")
    rep.finish()


# ---- stage 1 written by another launch ------------------------------------------------------------------------------------------
def _conv_1x1(cuda, g, r, N, H, W, C):
    """a 1x1 convolution of C -> C channels on N x H x W pixels with fresh tensors: (problem, x, packed weights, output)"""
    from retinanet import _C
    lib = _lib()
    x = (torch.randn((N, H, W, C), generator=g) * (1.0 + 0.25 * r) + 0.3 * r).to(H16).to(cuda)
    w = (torch.randn((1, 1, C, C), generator=g) / 8.0 + 0.02).to(cuda).contiguous()
    cinp = lib.rn_conv_cin_pad(C)
    wp = torch.empty((lib.rn_conv_cout_pad(C), 1, 1, cinp), dtype=H16, device=cuda)
    _C.check(lib.rn_pack_conv_weight(_C.ptr(w), 1, 1, C, C, cinp, _C.ptr(wp), _C.current_stream()), "pack")
    out = torch.zeros((N, H, W, C), dtype=H16, device=cuda)
    pc = _C.ConvProblem()
    pc.R = pc.S = pc.stride_h = pc.stride_w = 1
    pc.pad_top = pc.pad_left = 0
    pc.act, pc.out_dtype, pc.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, 1
    sg = pc.seg[0]
    sg.x, sg.w, sg.y = x.data_ptr(), wp.data_ptr(), out.data_ptr()
    sg.N, sg.H, sg.W, sg.Cin, sg.pix_stride, sg.Ho, sg.Wo, sg.Cout = N, H, W, C, C, H, W, C
    return pc, (x, w, wp), out


def _plain_segment(P, C, g, replicas):
    return S.make_inputs([(P, C)], replicas, H16, int(torch.randint(1, 1 << 20, (1,), generator=g)))[0]


@pytest.mark.parametrize("build", BUILDS)
def test_forward_partials_from_the_conv_epilogue_under_count_scale(cuda, build):
    """rn_conv_segment.bn_partial + rn_bn_segment.ext_chunks on every shard (a 1x1 conv of 64 -> 64 channels on 2 x 9 x 7
    pixels), rn_bn_stats per shard, all-reduce, rn_bn_finalize with count_scale = 2: the table and the moving statistics
    of the concatenated STORED conv outputs, same bounds"""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(41)
    N, H, W, C, replicas = 2, 9, 7, 64, 2
    seg = _plain_segment(N * H * W, C, g, replicas)
    shards, keep = [], []
    for r in range(replicas):
        sh = _shard(cuda, [seg], r, "none", False, 1, 0, float(replicas))
        pc, tensors, out = _conv_1x1(cuda, g, r, N, H, W, C)
        sh.p.seg[0].y = out.data_ptr()
        sh.p.seg[0].ext_chunks = lib.rn_conv_bn_row_blocks(ctypes.byref(pc), 0)
        assert sh.p.seg[0].ext_chunks >= 1
        sh.ws = _workspace(sh.p, cuda)
        pc.seg[0].bn_partial = sh.ws.data_ptr() + lib.rn_bn_partial_offset_bytes(ctypes.byref(sh.p), 0)
        _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(pc), _C.current_stream()), "conv")
        sh.T[0]["y"] = out.reshape(-1, C)
        shards.append(sh)
        keep.append((pc, tensors))
    _forward(shards)
    rep = _Report("conv-epilogue partials, count_scale = 2")
    ys = [sh.T[0]["y"].cpu() for sh in shards]
    assert float(torch.cat(ys).float().abs().max()) > 0.5
    _check_forward_tables(rep, shards, [ys], replicas, 1, no_special=True)       # conv outputs: the ordinary bounds throughout
    _check_elements(rep, shards, replicas, "none", 0, backward=False)
    rep.finish()


@pytest.mark.parametrize("build", BUILDS)
def test_backward_partials_from_the_data_gradient_under_count_scale(cuda, build):
    """rn_conv_segment.bn_bwd_y + rn_bn_segment.ext_chunks_bwd (relu, no residual) on every shard: the launch that writes
    dz writes stage 1 of rn_bn_bwd_reduce from the all-reduced table; bsums per shard are the LOCAL sums, their sum and
    count_scale = 2 give dy"""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(43)
    N, H, W, C, replicas = 2, 9, 7, 64, 2
    seg = _plain_segment(N * H * W, C, g, replicas)
    shards, keep = [], []
    for r in range(replicas):
        sh = _shard(cuda, [seg], r, "relu", False, 0, 0, float(replicas))
        pc, tensors, out = _conv_1x1(cuda, g, r, N, H, W, C)
        sh.p.seg[0].dz = out.data_ptr()
        sh.p.seg[0].ext_chunks_bwd = lib.rn_conv_bn_row_blocks(ctypes.byref(pc), 0)
        sh.ws = _workspace(sh.p, cuda)
        sh.T[0]["dz"] = out.reshape(-1, C)
        shards.append(sh)
        keep.append((pc, tensors))
    _forward(shards)
    for sh, (pc, _) in zip(shards, keep):
        sg = pc.seg[0]
        sg.bn_partial = sh.ws.data_ptr() + lib.rn_bn_bwd_partial_offset_bytes(ctypes.byref(sh.p), 0)
        sg.bn_bwd_y, sg.bn_bwd_fwd = sh.T[0]["y"].data_ptr(), sh.T[0]["fwd"].data_ptr()
        _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(pc), _C.current_stream()), "data gradient")
    _backward(shards)
    rep = _Report("data-gradient partials, count_scale = 2")
    assert all(float(sh.T[0]["dz"].float().abs().max()) > 0.5 for sh in shards)
    _check_forward_tables(rep, shards, [seg["ys"]], replicas, 0)
    _check_elements(rep, shards, replicas, "relu", 0)
    rep.finish()


@pytest.mark.parametrize("build", BUILDS)
def test_column_sums_of_dy_under_count_scale(cuda, build):
    """rn_bn_segment.dy_colsum_partial with count_scale = 2: dy has the bits of the call without the field, and the
    finished column sums (rn_bn_stats on the per-chunk partials) are the column sums of the STORED dy to 2e-6 of the
    column's absolute sum"""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(47)
    P, C, replicas = 300, 64, 2                 # 2400 16-byte units: two 2048-unit chunks, the second short
    seg = _plain_segment(P, C, g, replicas)
    rep = _Report("dy column sums, count_scale = 2")
    dys = {}
    for fused in (False, True):
        shards = [_shard(cuda, [seg], r, "relu", False, 0, 0, float(replicas)) for r in range(replicas)]
        finish = []
        if fused:
            for sh in shards:
                ch = lib.rn_bn_bwd_colsum_chunks(ctypes.byref(sh.p), 0)
                assert ch == 2
                p2 = _C.BnProblem()
                p2.num_segments, p2.act, p2.bessel, p2.eps, p2.momentum, p2.count_scale = 1, 0, 0, 0.0, 0.0, 1.0
                sums = torch.zeros((2, C), dtype=torch.float32, device=cuda)
                q = p2.seg[0]
                q.y, q.sums, q.P, q.C, q.ext_chunks = sh.T[0]["dy"].data_ptr(), sums.data_ptr(), P, C, ch
                ws2 = torch.zeros((lib.rn_bn_workspace_bytes(ctypes.byref(p2)),), dtype=torch.uint8, device=cuda)
                sh.p.seg[0].dy_colsum_partial = ws2.data_ptr() + lib.rn_bn_partial_offset_bytes(ctypes.byref(p2), 0)
                finish.append((p2, ws2, sums))
        _forward(shards)
        _backward(shards)
        for p2, ws2, _ in finish:
            _C.check(lib.rn_bn_stats(ctypes.byref(p2), _C.ptr(ws2), ws2.numel(), _C.current_stream()), "column sums")
        torch.cuda.synchronize()
        dys[fused] = [sh.T[0]["dy"].clone() for sh in shards]
        if fused:
            _check_elements(rep, shards, replicas, "relu", 0)
            for r, (sh, (_, _, sums)) in enumerate(zip(shards, finish)):
                dy = sh.T[0]["dy"].cpu().to(F64)
                rep.add("column sums", (sums[0].cpu().to(F64) - dy.sum(0)).abs() / (2e-6 * dy.abs().sum(0)).clamp_min(1e-300),
                        f"shard {r}")
    for a, b in zip(dys[False], dys[True]):
        assert torch.equal(_bits(a), _bits(b))
    rep.finish()
