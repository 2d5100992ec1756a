"""GPU: a frozen BatchNorm under a trainable conv (the `bn` / `backbone-bn` / `fpn-bn` / `head-bn` keys of
training.freeze_variables) — the kernel rn_bn_frozen_bwd against frozen_bn_ref.py, and the engine around it: the four keys
on ResNet-50, a float64 slice of one bottleneck tail, EfficientNet-B0 in mixed_float16, checkpoints, two ranks."""
import ctypes
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch

import act_ref as A
import frozen_bn_ref as F
import pyramid_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

H16 = torch.bfloat16
_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BUILDS = ["bf16", "f16"]
KEYS = ["bn", "backbone-bn", "fpn-bn", "head-bn"]


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


# ---- kernel ------------------------------------------------------------------------------------------------------------------
# (P, C, rows per sample) with N = 2 images: one 8-channel group; C/8 = 3 does not divide 256 (grid-stride form); the chunked
# form with one partial workgroup (50 * 8 = 400 of 2 048 units) and with three workgroups, the last partial (182 * 32 = 5 824)
SHAPES = {"8": (50, 8, 25), "24": (182, 24, 91), "64": (50, 64, 25), "256": (182, 256, 91)}
PROBLEMS = [("8",), ("24",), ("64",), ("256",), ("64", "256"), ("24", "8")]     # the last two: blockIdx.y indexing
GUARD = 64
_NAN_BITS = 0x7FC0BEEF


def _inputs(names, residual, seed, drop_connect=False):
    """Per segment: y and the residual on multiples of 1/4, scale on multiples of 1/2 without 0, shift on multiples of 1/8:
    u = y scale + shift and u + residual are multiples of 1/8 below 16, exact in fp32 and in both storage types, so the value
    in front of the activation is the same number in the kernel and in the reference and lands exactly on 0 and on 6.
    Built on the CPU, never modified."""
    key = (H16, names, residual, seed, drop_connect)
    if key not in _inputs.cache:
        g = torch.Generator().manual_seed(seed)
        segs = []
        for n in names:
            P, C, rows = SHAPES[n]
            sc = torch.randint(1, 5, (C,), generator=g).float() / 2 * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
            sh = torch.randint(-8, 9, (C,), generator=g).float() / 8
            segs.append({"y": R.grid((P, C), g, H16, lim=16), "scale": sc, "shift": sh, "dz": R.grads((P, C), g, H16),
                         "residual": R.grid((P, C), g, H16) if residual else None, "dres0": R.grads((P, C), g, H16),
                         "rows": rows, "sample_scale": torch.tensor([0.0, 1.25]) if drop_connect else None})
        _inputs.cache[key] = segs
    return _inputs.cache[key]


_inputs.cache = {}


def _problem(cuda, act, segs, accumulate=False, mask=False, canaries=False):
    """rn_bn_problem of a frozen BatchNorm over `segs`: everything the statistics, the reductions and the gamma / beta
    gradients touch is NULL — or, canaries=True, a buffer full of one NaN pattern that must come back unchanged.  The
    mean / invstd rows of the fwd table are NaN: nothing may use them."""
    from retinanet import _C
    p = _C.BnProblem()
    p.num_segments, p.act, p.bessel, p.eps, p.momentum, p.count_scale = len(segs), _C.ACT_IDS[act], 1, 1e-3, 0.99, 1.0
    T = []
    for i, s in enumerate(segs):
        P, C = s["y"].shape
        t = {"y": s["y"].to(cuda).contiguous(), "dz": s["dz"].to(cuda).contiguous(), "P": P, "C": C}
        t["fwd"] = torch.stack([torch.full((C,), float("nan")), torch.full((C,), float("nan")), s["scale"],
                                s["shift"]]).to(cuda).contiguous()
        t["z"] = torch.full_like(t["y"], 7.0)
        t["residual"] = None if s["residual"] is None else s["residual"].to(cuda).contiguous()
        t["dy"] = torch.full((P * C + GUARD,), 7.0, dtype=H16, device=cuda)
        t["dres"] = None
        if s["residual"] is not None:
            t["dres"] = torch.full((P * C + GUARD,), 7.0, dtype=H16, device=cuda)
            if accumulate:
                t["dres"][:P * C].copy_(s["dres0"].reshape(-1))
        t["mask"] = torch.full((P * C // 8,), 0xA5, dtype=torch.uint8, device=cuda) if mask else None
        t["m"] = None if s["sample_scale"] is None else s["sample_scale"].to(cuda)
        d = p.seg[i]
        d.y, d.z, d.dz, d.dy, d.fwd = (t["y"].data_ptr(), t["z"].data_ptr(), t["dz"].data_ptr(), t["dy"].data_ptr(),
                                       t["fwd"].data_ptr())
        d.residual, d.dres, d.act_mask = (None if t[k] is None else t[k].data_ptr() for k in ("residual", "dres", "mask"))
        d.P, d.C, d.dres_accumulate = P, C, int(accumulate)
        if t["m"] is not None:
            d.sample_scale, d.rows_per_sample = t["m"].data_ptr(), s["rows"]
        if canaries:
            t["canary"] = {k: torch.full((2 * C,), _NAN_BITS, dtype=torch.int32, device=cuda)
                           for k in ("sums", "bsums", "moving_mean", "moving_var", "dgamma", "dbeta")}
            for k, v in t["canary"].items():
                setattr(d, k, v.data_ptr())
        T.append(t)
    return p, T


def _forward(p):
    from retinanet import _C
    _C.check(_lib().rn_bn_apply(ctypes.byref(p), _C.current_stream()), "rn_bn_apply")
    torch.cuda.synchronize()


def _frozen_bwd(p):
    from retinanet import _C
    _C.check(_lib().rn_bn_frozen_bwd(ctypes.byref(p), _C.current_stream()), "rn_bn_frozen_bwd")
    torch.cuda.synchronize()


def _reference(s, act, accumulate, storage, fp):
    np_ = lambda t: None if t is None else t.to(torch.float64).numpy().astype(fp)
    m = None if s["sample_scale"] is None else s["sample_scale"].numpy()
    fwd = F.forward(np_(s["y"]), s["scale"].numpy(), s["shift"].numpy(), act, np_(s["residual"]), m, s["rows"],
                    storage=storage, fp=fp)
    bwd = F.backward(np_(s["dz"]), s["scale"].numpy(), act, fwd, m, s["rows"],
                     dres0=np_(s["dres0"]) if accumulate else None, storage=storage, fp=fp)
    return fwd, bwd


def _outputs(t):
    n = t["P"] * t["C"]
    dy = t["dy"][:n].reshape(t["P"], t["C"]).cpu()
    dres = None if t["dres"] is None else t["dres"][:n].reshape(t["P"], t["C"]).cpu()
    for k in ("dy", "dres"):      # nothing was written behind the tensors
        assert t[k] is None or bool((t[k][n:].float() == 7.0).all()), (k, "guard")
    return dy, dres


def _bits_equal(got, want32):
    return A.same_values(got, torch.from_numpy(np.ascontiguousarray(want32)).to(H16))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("residual", ["no", "first-write", "accumulate"])
@pytest.mark.parametrize("act", ["none", "relu", "relu6"])
@pytest.mark.parametrize("names", PROBLEMS, ids=["+".join(n) for n in PROBLEMS])
def test_frozen_bwd_bit_exact(cuda, build, names, act, residual):
    """dy = rs(scale g) and dres = rs(g [+ dres]) bit for bit against the fp32 numpy restatement: g is dz or 0, the product is
    ONE fp32 multiply of exactly representable inputs and one rounding.  Every gate source the header lists gives the same
    bits: the natural one (u = y scale + shift without a residual input, the stored z behind one — y is then NaN: the pass
    may not touch it) and the act_mask bits (y AND z NaN).  Everything a frozen layer does not own is a NaN canary."""
    has_res, acc = residual != "no", residual == "accumulate"
    segs = _inputs(names, has_res, seed=11)
    want = [_reference(s, act, acc, H16, np.float32) for s in segs]
    if act != "none" and sum(s["y"].numel() for s in segs) >= 3000:      # the kinks are hit exactly, and from both sides
        pre = np.concatenate([f["pre"].reshape(-1) for f, _ in want])
        assert (pre == 0).any() and (pre < 0).any() and (pre > 0).any()
        assert act != "relu6" or ((pre == 6).any() and (pre > 6).any())
    for masked in (False, True) if act != "none" else (False,):
        p, T = _problem(cuda, act, segs, accumulate=acc, mask=masked, canaries=True)
        _forward(p)
        for t, (fwd, _) in zip(T, want):
            assert _bits_equal(t["z"].cpu(), fwd["z"]), "z"
            if masked:
                assert np.array_equal(t["mask"].cpu().numpy(), F.gate_bits(fwd["z"], act)), "gate bits"
            if masked or act == "none" or has_res:
                t["y"].fill_(float("nan"))          # not a gate source here
            if masked or act == "none" or not has_res:
                t["z"].fill_(float("nan"))
        _frozen_bwd(p)
        for i, (t, (_, bwd)) in enumerate(zip(T, want)):
            dy, dres = _outputs(t)
            what = (names, act, residual, "mask" if masked else "natural gate", "segment", i)
            assert _bits_equal(dy, bwd["dy"]), (what, "dy", int((dy.float().numpy() != bwd["dy"]).sum()))
            if has_res:
                assert _bits_equal(dres, bwd["dres"]), (what, "dres", int((dres.float().numpy() != bwd["dres"]).sum()))
            for k, v in t["canary"].items():
                assert bool((v == _NAN_BITS).all()), (what, k, "was written")
            assert bool(torch.isnan(t["fwd"][:2]).all())


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("act", ["relu", "relu6"])
def test_frozen_bwd_segments_disagree_on_the_residual(cuda, build, act):
    """one problem, a segment behind a residual add (gate: the stored z) and one without (gate: u): the generic form,
    bit for bit like the uniform ones"""
    with_res, without = _inputs(("64",), True, seed=15)[0], _inputs(("24",), False, seed=16)[0]
    segs = [with_res, without]
    p, T = _problem(cuda, act, segs)
    _forward(p)
    T[0]["y"].fill_(float("nan"))
    T[1]["z"].fill_(float("nan"))
    _frozen_bwd(p)
    for s, t in zip(segs, T):
        _, bwd = _reference(s, act, False, H16, np.float32)
        dy, dres = _outputs(t)
        assert _bits_equal(dy, bwd["dy"]) and (dres is None or _bits_equal(dres, bwd["dres"]))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("names", PROBLEMS, ids=["+".join(n) for n in PROBLEMS])
def test_frozen_bwd_swish(cuda, build, names, residual):
    """swish' at the value rn_bn_apply fed to swish (the same number in kernel and reference on these inputs), against
    float64 with the allowance the live passes' swish gate has in test_gpu_activation_math.py
    (test_bn_backward_sums_and_gradients: pyramid_ref.Ref with act_ref.DERIV_SLACK scaled by the gate's other factors,
    |scale dz| for dy and |dz| for dres); fp32 operations per element: 2 for dy (gate, scale), 2 for dres (gate, add)."""
    segs = _inputs(names, residual, seed=12)
    p, T = _problem(cuda, "swish", segs, accumulate=residual)
    _forward(p)
    for t in T:
        t["z"].fill_(float("nan"))                  # swish' is no function of z
    _frozen_bwd(p)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    missed = []
    for i, (s, t) in enumerate(zip(segs, T)):
        fwd, bwd = _reference(s, "swish", residual, None, np.float64)
        assert np.array_equal(fwd["pre"].astype(np.float32).astype(np.float64), fwd["pre"]), "exact in front of swish"
        dy, dres = _outputs(t)
        dz, sc = f64(s["dz"].double().numpy()), f64(s["scale"].double().numpy())
        want = f64(bwd["dy"])
        ref = R.Ref(R.round_storage(want, H16), want.abs(), 2, (sc * dz).abs() * A.DERIV_SLACK)
        ok, ratio, outside = R.check(dy, ref, H16)
        print(f"swish dy {names} segment {i} residual={residual}: worst |got - ref| / bound = {ratio:.4f}")
        if not ok:
            missed.append(("dy", i, ratio, outside))
        if residual:
            g, old = f64(bwd["g"]), f64(s["dres0"].double().numpy())
            ref = R.Ref(R.round_storage(g + old, H16), g.abs() + old.abs(), 2, dz.abs() * A.DERIV_SLACK)
            ok, ratio, outside = R.check(dres, ref, H16)
            print(f"swish dres {names} segment {i}: worst |got - ref| / bound = {ratio:.4f}")
            if not ok:
                missed.append(("dres", i, ratio, outside))
    assert not missed, missed


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("names", PROBLEMS, ids=["+".join(n) for n in PROBLEMS])
def test_frozen_bwd_drop_connect(cuda, build, names, accumulate):
    """sample_scale = (0, 1.25), act = none, a residual input: dy = rs(scale (dz m_n)) bit for bit (two fp32 products) — the
    zeroed image's rows are 0 — and dres = rs(dz [+ dres]) does not see the factor.  All pointers a frozen layer does not own
    are NULL here."""
    segs = _inputs(names, True, seed=13, drop_connect=True)
    p, T = _problem(cuda, "none", segs, accumulate=accumulate)
    for t in T:
        t["y"].fill_(float("nan"))
    _frozen_bwd(p)
    for s, t in zip(segs, T):
        _, bwd = _reference(s, "none", accumulate, H16, np.float32)
        dy, dres = _outputs(t)
        assert _bits_equal(dy, bwd["dy"]) and _bits_equal(dres, bwd["dres"])
        assert bool((dy[:s["rows"]].float() == 0).all()) and bool((dy[s["rows"]:].float() != 0).any())
        zero_m = dict(s, sample_scale=None)
        assert _bits_equal(dres, _reference(zero_m, "none", accumulate, H16, np.float32)[1]["dres"])


@pytest.mark.parametrize("build", BUILDS)
def test_frozen_bwd_refusals(cuda, build):
    """RN_EINVAL before any launch, dy untouched: C % 8 != 0, swish with sample_scale, a missing dz, a set dy_colsum_partial"""
    from retinanet import _C
    lib, st = _lib(), _C.current_stream()
    g = torch.Generator().manual_seed(14)

    def seg(C=16):
        return {"y": R.grid((50, C), g, H16), "scale": torch.ones(C), "shift": torch.zeros(C), "dz": R.grads((50, C), g, H16),
                "residual": None, "dres0": None, "rows": 25, "sample_scale": None}

    def refused(p, T):
        rc = lib.rn_bn_frozen_bwd(ctypes.byref(p), st)
        torch.cuda.synchronize()
        return rc == _C.RN_EINVAL and all(bool((t["dy"].float() == 7.0).all()) for t in T)

    p, T = _problem(cuda, "none", [seg()])
    assert lib.rn_bn_frozen_bwd(ctypes.byref(p), st) == _C.RN_OK     # the problem the refusals are variations of
    torch.cuda.synchronize()
    assert not bool((T[0]["dy"][:800].float() == 7.0).all())
    p, T = _problem(cuda, "none", [seg(C=12)])
    assert refused(p, T), "C = 12"
    p, T = _problem(cuda, "swish", [dict(seg(), sample_scale=torch.tensor([0.0, 1.25]))])
    assert refused(p, T), "swish with sample_scale"
    p, T = _problem(cuda, "relu", [seg()])
    p.seg[0].dz = None
    assert refused(p, T), "NULL dz"
    p, T = _problem(cuda, "none", [seg()])
    part = torch.zeros((4096,), dtype=torch.float32, device=cuda)
    p.seg[0].dy_colsum_partial = part.data_ptr()
    assert refused(p, T) and bool((part == 0).all()), "dy_colsum_partial"
    p, T = _problem(cuda, "none", [seg()])
    p.seg[0].fwd = None
    assert refused(p, T), "NULL fwd"
    p, T = _problem(cuda, "relu", [seg()])
    p.seg[0].y = None                                 # relu without a residual input and without bits gates on u
    assert refused(p, T), "NULL y where the gate needs it"


# ---- engine -------------------------------------------------------------------------------------------------------------------
def _randomize(model, seed, cuda):
    """gamma / beta as test_gpu_train_kernels.py::test_bottleneck_tail_forward_backward_tight sets them (every branch
    carries signal), and moving statistics that are not the initial 0 / 1"""
    gen = torch.Generator().manual_seed(seed)
    for k, v in model.variables.items():
        if k.endswith("/gamma"):
            zero_init = model.graph.bns[k[:-len("/gamma")]].get("gamma_zero")
            lo, span = (0.2, 0.3) if zero_init else (0.75, 0.5)
            v.copy_((torch.rand(v.shape, generator=gen) * span + lo).to(cuda))
        elif k.endswith("/beta") or k.endswith("/moving_mean"):
            v.copy_((torch.randn(v.shape, generator=gen) * 0.1).to(cuda))
        elif k.endswith("/moving_variance"):
            v.copy_((torch.rand(v.shape, generator=gen) * 0.5 + 0.75).to(cuda))


def _batch(p, cuda, size, B, seed):
    from make_golden import synth_gt
    from retinanet.dataloader import LabelEncoder
    enc = LabelEncoder(p, device=cuda)
    rng = np.random.default_rng(seed)
    gts = [synth_gt(rng, int(rng.integers(2, 6)), size) for _ in range(B)]
    Gmax = max(x[0].shape[0] for x in gts)
    gb, gc, cnt = np.zeros([B, Gmax, 4], np.float32), np.zeros([B, Gmax], np.float32), np.zeros([B], np.int32)
    for i, (b_, c_) in enumerate(gts):
        gb[i, :len(b_)], gc[i, :len(c_)], cnt[i] = b_, c_, len(b_)
    targets = enc.encode_batch(torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(cnt))
    images = torch.randn((B, size, size, 3), generator=torch.Generator().manual_seed(seed)).to(cuda)
    return images, targets


def _resnet_engine(cuda, key, seed=5, size=128, B=2, weight_decay=True):
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=size, freeze=[key])
    p.architecture.batch_norm.use_sync = False
    p.training.use_weight_decay = weight_decay
    builder = ModelBuilder(p, "train", device=cuda, seed=seed)
    model = builder()
    _randomize(model, seed, cuda)
    rx = [builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables]
    eng = TrainEngine(model, B, frozen_regexes=rx, world_size=1)
    model.optimizer.lr = lambda step: 0.01
    images, targets = _batch(p, cuda, size, B, seed)
    return p, model, eng, images, targets


def _frozen_state(model, eng):
    """every tensor a frozen BatchNorm owns: its four variables in the model and the engine's scale / shift tables"""
    ops = [o for o in eng.ops if eng._bn_frozen(o)]
    state = {o["bn"] + sfx: model.variables[o["bn"] + sfx].clone()
             for o in ops for sfx in ("/gamma", "/beta", "/moving_mean", "/moving_variance")}
    for out, grp in eng.bn_groups.items():
        if grp.frozen:
            state["fwd:" + out] = grp.fwd.clone()
    return ops, state


def _assert_frozen_state(model, eng, state):
    for k, v in state.items():
        now = eng.bn_groups[k[4:]].fwd if k.startswith("fwd:") else model.variables[k]
        assert torch.equal(now, v), k


@pytest.mark.parametrize("key", KEYS)
def test_resnet50_trains_with_frozen_batchnorm(cuda, key):
    """The engine builds (before this feature: NotImplementedError) and steps.  Weight decay is off so that a kernel under
    a frozen BatchNorm moves only through the gradient rn_bn_frozen_bwd hands to its weight-gradient launch."""
    p, model, eng, images, targets = _resnet_engine(cuda, key, weight_decay=False)
    scope = {"bn": lambda n: True, "backbone-bn": lambda n: not n.startswith(("fpn", "box-head", "class-head")),
             "fpn-bn": lambda n: n.startswith("fpn"), "head-bn": lambda n: n.startswith(("box-head", "class-head"))}[key]
    ops, state = _frozen_state(model, eng)
    with_bn = [o for o in eng.ops if o.get("bn")]
    assert ops and {o["bn"] for o in ops} == {o["bn"] for o in with_bn if scope(o["bn"])}
    live = [o for o in with_bn if not scope(o["bn"])]
    assert bool(live) == (key != "bn") and {o["bn"] for o in live} == set(eng.bn_state)
    # no gamma / beta of a frozen layer trains; every live one and every kernel does
    for o in ops:
        assert o["bn"] + "/gamma" not in eng.train_names and o["bn"] + "/beta" not in eng.train_names
        assert eng._kvar(o) in eng.train_names
    for o in live:
        assert o["bn"] + "/gamma" in eng.train_names and o["bn"] + "/beta" in eng.train_names
    # no BatchNorm-backward reduction was folded into a data gradient for a frozen layer, none is waiting to be
    frozen_problems = {id(g.problem) for g in eng.bn_groups.values() if g.frozen}
    assert not frozen_problems & set(eng._bn_bwd_pending) and not {o["out"] for o in ops} & set(eng.bn_bwd_fused)
    for g in eng.bn_groups.values():
        if g.frozen:
            for i in range(g.problem.num_segments):
                s = g.problem.seg[i]
                assert not (s.sums or s.bsums or s.gamma or s.beta or s.moving_mean or s.moving_var or s.dgamma or s.dbeta)
                assert not (s.ext_chunks or s.ext_chunks_bwd or s.dy_colsum_partial)
                assert bool(s.act_mask) == (g.ops[i]["act"] in ("relu", "relu6"))
    w0 = eng.P.clone()
    mm0 = {bn: (d["mm"].clone(), d["mv"].clone()) for bn, d in eng.bn_state.items()}
    out = eng.train_step(images, targets)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["weighted-loss"].item())) and bool(torch.isfinite(eng.P).all())
    eng.store_to_model()
    _assert_frozen_state(model, eng, state)
    still = [eng._kvar(o) for o in ops
             if torch.equal(eng._pview(eng._kvar(o)), w0[eng.p_off[eng._kvar(o)][0]:][:eng.p_off[eng._kvar(o)][1]])]
    assert not still, still[:8]
    same = [bn for bn, (mm, mv) in mm0.items() if torch.equal(eng.bn_state[bn]["mm"], mm) and
            torch.equal(eng.bn_state[bn]["mv"], mv)]
    assert not same, same[:8]
    assert eng.syncbn_messages_per_step == 0


def test_executor_path_backbone_bn(cuda):
    """The executor's own route to the engine: Executor._maybe_freeze_layers marks LAYERS (ResNet's BatchNorm layers are
    layers of their own), the model hands their variables to `train_engine` as frozen names.  `backbone-bn` is the key of
    the four that this route turns into frozen BatchNorm under trainable convs (see
    test_frozen_bn_ref_cpu.py::test_executor_freezes_by_layer_like_the_reference for the other three)."""
    from types import SimpleNamespace
    from retinanet.cfg import default_params
    from retinanet.executor import Executor
    from retinanet.model import ModelBuilder
    p = default_params(input_size=128, freeze=["backbone-bn"])
    p.architecture.batch_norm.use_sync = False
    builder = ModelBuilder(p, "train", device=cuda, seed=5)
    model = builder()
    _randomize(model, 5, cuda)
    assert Executor._maybe_freeze_layers(SimpleNamespace(params=p, model_builder=builder, _model=model))
    eng = model.train_engine(2, world_size=1)
    ops, state = _frozen_state(model, eng)
    assert ops and all(not o["bn"].startswith(("fpn", "box-head", "class-head")) for o in ops)
    assert all(eng._kvar(o) in eng.train_names for o in ops) and eng.bn_state
    model.optimizer.lr = lambda step: 0.01
    images, targets = _batch(p, cuda, 128, 2, 5)
    out = eng.train_step(images, targets)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["weighted-loss"].item()))
    eng.store_to_model()
    _assert_frozen_state(model, eng, state)


def _ulp_outliers(got, want64, ulps=2.0):
    """test_gpu_train_kernels.py::_ulp_outliers: fraction of 16-bit elements farther than `ulps` bf16 ulps from the float64
    value (ulp of the element's own magnitude, floored at 2^-8 of the tensor's rms)"""
    w = want64.abs()
    rms = want64.pow(2).mean().sqrt()
    mag = torch.maximum(w, rms * 2.0 ** -8)
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag)) - 7)
    return ((got.double() - want64).abs() > ulps * ulp).double().mean().item()


def test_bottleneck_tail_with_frozen_batchnorm_tight(cuda):
    """test_gpu_train_kernels.py::test_bottleneck_tail_forward_backward_tight's slice — `g2b1_b` (3x3, BN, relu) ->
    `g2b1_out` (1x1, BN, + `g2b0_out`, relu) — with freeze = ["bn"], at 128 x 128 / B = 2 (16 x 16 x 128 / 512 here),
    recomputed in float64 from the engine's own boundary tensors with the frozen arithmetic: u = y scale + shift from the
    MOVING statistics, dy = scale g.  Budgets: the ones of that test, by line of test_gpu_train_kernels.py."""
    from test_gpu_train_kernels import _conv3x3_dgrad_f64, _conv3x3_f64, _conv3x3_wgrad_f64
    p, model, eng, images, targets = _resnet_engine(cuda, "bn")
    with torch.cuda.device(cuda):
        eng._step_args = dict(wdc=0.0, alpha=0.0, unscale=1.0, clip=0.0)
        eng._prepack_dgrad_weights()
        preds = eng.forward(images)
        model.loss(targets, preds, compute_grads=True, grad_scale=1.0, grads_bf16=eng.loss_grad_buffers(), normalizer=None)
        eng._train_step_active = True
        try:
            eng.backward(None)
        finally:
            eng._train_step_active = False
        torch.cuda.synchronize()
    ops = {o["out"]: o for o in eng.ops if o["op"] == "conv"}
    ob, oo = ops["g2b1_b"], ops["g2b1_out"]
    assert eng.tensors["g2b1_b"][:3] == (16, 16, 128) and oo["residual"] == "g2b0_out"
    assert eng._bn_frozen(ob) and eng._bn_frozen(oo)
    rb = lambda t: t.to(eng.h16).double()
    var = model.variables
    f64 = lambda k: var[k].to(cuda).double()

    def fold(bn):
        scale = f64(bn + "/gamma") / torch.sqrt(f64(bn + "/moving_variance") + eng.eps)
        return scale, f64(bn + "/beta") - f64(bn + "/moving_mean") * scale
    x, res, dz = eng.t["g2b1_a"].double(), eng.t["g2b0_out"].double(), eng.grad["g2b1_out"].double()
    wb = rb(var[ob["conv"] + "/kernel"].to(cuda))
    wo = rb(var[oo["conv"] + "/kernel"].to(cuda))[0, 0]
    (sc_b, sh_b), (sc_o, sh_o) = fold(ob["bn"]), fold(oo["bn"])
    # ---- forward (budgets: lines 1149, 1152, 1155, 1159 of test_gpu_train_kernels.py)
    yb64 = _conv3x3_f64(x, wb)
    yb = rb(yb64)
    assert _ulp_outliers(eng.raw["g2b1_b"], yb64, 1.0) < 1e-3                       # :1149
    ub = yb * sc_b + sh_b
    zb = rb(torch.relu(ub))
    assert _ulp_outliers(eng.t["g2b1_b"], torch.relu(ub), 2.0) < 2e-3               # :1152
    yo64 = zb @ wo
    yo = rb(yo64)
    assert _ulp_outliers(eng.raw["g2b1_out"], yo64, 2.0) < 2e-3                     # :1155
    so = rb(yo * sc_o + sh_o) + res
    assert _ulp_outliers(eng.t["g2b1_out"], torch.relu(so), 2.0) < 3e-3             # :1159
    # ---- backward: no mean / xhat term
    dyo = sc_o * (dz * (so > 0))
    dyo_r = rb(dyo)
    dzb64 = dyo_r @ wo.t()
    dwo = zb.reshape(-1, zb.shape[3]).t() @ dyo_r.reshape(-1, dyo_r.shape[3])
    dyb = sc_b * (rb(dzb64) * (ub > 0))
    dyb_r = rb(dyb)
    dx64 = _conv3x3_dgrad_f64(dyb_r, wb)
    dwb = _conv3x3_wgrad_f64(x, dyb_r)

    def cos(a, b):
        a, b = a.double().reshape(-1), b.double().reshape(-1)
        return (a @ b / (a.norm() * b.norm() + 1e-300)).item()

    def rel(a, b):
        return ((a.double() - b).norm() / (b.norm() + 1e-300)).item()

    def kernel_grad(conv):
        c = eng.g.convs[conv]
        return eng._pview(conv + "/kernel", eng.G).reshape(c["cout"], c["k"], c["k"], c["cin"]).permute(1, 2, 3, 0)
    report = {}
    # gradient tensors — dz, dx and the two dy rn_bn_frozen_bwd wrote: cosine > 0.9999, 2 ulp on all but 2 %, 4 ulp on all
    # but 0.5 % (:1187)
    for name, got, want in (("dy(g2b1_out)", eng.dy_of["g2b1_out"], dyo), ("dy(g2b1_b)", eng.dy_of["g2b1_b"], dyb),
                            ("dz(g2b1_b)", eng.grad["g2b1_b"], dzb64), ("dx(g2b1_a)", eng.grad["g2b1_a"], dx64)):
        report[name] = (cos(got, want), _ulp_outliers(got, want, 2.0), _ulp_outliers(got, want, 4.0))
        print(name, report[name])
        assert report[name][0] > 0.9999 and report[name][1] < 2e-2 and report[name][2] < 5e-3, report
    # weight gradients: cosine > 0.9999, 2e-3 relative (:1194)
    for name, got, want in (("dW out", kernel_grad(oo["conv"])[0, 0], dwo), ("dW b", kernel_grad(ob["conv"]), dwb)):
        report[name] = (cos(got, want), rel(got, want))
        print(name, report[name])
        assert report[name][0] > 0.9999 and report[name][1] < 2e-3, report
    # the skip gradient took g, not scale g
    assert eng.grad["g2b0_out"].abs().sum().item() > 0


def _effnet_run(cuda, steps=2):
    from retinanet.cfg import efficientnet_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    size, B = 128, 2
    p = efficientnet_params("efficientnet-b0", input_size=size)
    assert p.floatx.precision == "mixed_float16"
    p.architecture.batch_norm.use_sync = False
    p.training.freeze_variables = ["bn"]
    builder = ModelBuilder(p, "train", device=cuda, seed=11)
    model = builder()
    _randomize(model, 11, cuda)
    eng = TrainEngine(model, B, frozen_regexes=[builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables], world_size=1)
    model.optimizer.lr = lambda step: 0.01
    images, targets = _batch(p, cuda, size, B, 11)
    ops, state = _frozen_state(model, eng)
    w0 = eng.P.clone()
    losses = [float(eng.train_step(images, targets)["weighted-loss"].item()) for _ in range(steps)]
    torch.cuda.synchronize()
    eng.finish_step()
    eng.store_to_model()
    _assert_frozen_state(model, eng, state)
    return eng, ops, w0, losses


def test_efficientnet_b0_float16_frozen_batchnorm(cuda):
    """mixed_float16, swish, depthwise convs, squeeze-excite, drop_connect on, every BatchNorm frozen: builds, two steps,
    frozen state bit-stable, and a second engine from the same seed lands on the same bits"""
    eng, ops, w0, losses = _effnet_run(cuda)
    assert eng.f16 and not eng.bn_state and all(g.frozen for g in eng.bn_groups.values())
    assert {o["op"] for o in ops} >= {"conv", "dwconv", "stem"} and len(eng.dc_masks) > 0
    assert {o["act"] for o in ops} >= {"swish"}
    assert all(np.isfinite(losses)), losses
    assert not torch.equal(eng.P, w0) and bool(torch.isfinite(eng.P).all())
    eng2, _, _, losses2 = _effnet_run(cuda)
    assert losses2 == losses and torch.equal(eng2.P, eng.P) and torch.equal(eng2.V, eng.V) and torch.equal(eng2.E, eng.E)


def test_checkpoint_resume_with_frozen_batchnorm(cuda, tmp_path):
    """save after one step, restore into a fresh engine whose variables (frozen moving statistics included) start somewhere
    else: the scale / shift tables are refilled from the restored statistics and the next step is bit-equal"""
    p, model, eng, images, targets = _resnet_engine(cuda, "bn", seed=7)
    eng.train_step(images, targets)
    prefix = str(tmp_path / "weights_step_1")
    eng.save_checkpoint(prefix)
    _, state = _frozen_state(model, eng)
    want = eng.train_step(images, targets)["weighted-loss"].item()
    torch.cuda.synchronize()
    p2, model2, eng2, images2, targets2 = _resnet_engine(cuda, "bn", seed=7)
    with torch.no_grad():
        for v in model2.variables.values():
            v.add_(0.01)
    eng2.load_from_model()
    tables = [k for k in state if k.startswith("fwd:")]
    assert tables and not any(torch.equal(eng2.bn_groups[k[4:]].fwd, state[k]) for k in tables)   # load_from_model refilled
    eng2.restore_checkpoint(prefix)
    _assert_frozen_state(model2, eng2, state)
    assert eng2.step_count == 1
    got = eng2.train_step(images2, targets2)["weighted-loss"].item()
    torch.cuda.synchronize()
    assert got == want
    assert torch.equal(eng2.P, eng.P) and torch.equal(eng2.V, eng.V) and torch.equal(eng2.E, eng.E)
    _assert_frozen_state(model2, eng2, state)


# ---- two ranks on one device (gloo), modelled on test_gpu_data_parallel.py::test_two_ranks_match_one_process ------------------------
SIZE, B2, SEED = 128, 4, 21


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_build(world, rank, key):
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import synth_gt
    from retinanet.cfg import default_params
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    p = default_params(input_size=SIZE, batch_train=B2, freeze=[key])
    assert p.architecture.batch_norm.use_sync
    p.architecture.backbone.depth = 14
    p.training.optimizer.clipnorm = 1e9
    builder = ModelBuilder(p, "train", device=dev, seed=SEED)
    model = builder()
    _randomize(model, SEED, dev)
    per = B2 // world
    eng = TrainEngine(model, per, frozen_regexes=[builder.FREEZE_VARS_REGEX[key]], world_size=world)
    enc = LabelEncoder(p, device=dev)
    rng = np.random.default_rng(SEED)
    gts = [synth_gt(rng, int(rng.integers(2, 6)), SIZE) for _ in range(B2)]
    images = torch.randn((B2, SIZE, SIZE, 3), generator=torch.Generator().manual_seed(SEED))
    sl = slice(rank * per, (rank + 1) * per)
    gts = gts[sl]
    Gmax = max(x[0].shape[0] for x in gts)
    gb, gc, cnt = np.zeros([per, Gmax, 4], np.float32), np.zeros([per, Gmax], np.float32), np.zeros([per], np.int32)
    for i, (b, c) in enumerate(gts):
        gb[i, :len(b)], gc[i, :len(c)], cnt[i] = b, c, len(b)
    targets = enc.encode_batch(torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(cnt))
    return model, eng, images[sl].to(dev), targets


def _dp_step(world, rank, key):
    from retinanet.distribute import global_normalizer
    model, eng, images, targets = _dp_build(world, rank, key)
    model.optimizer.lr = lambda step: 0.01
    w0 = eng.P.cpu().numpy().copy()
    out = eng.train_step(images, targets)
    torch.cuda.synchronize()
    live = [g for g in eng.bn_groups.values() if not g.frozen]
    r = {"P": eng.P.cpu().numpy(), "w0": w0, "loss": float(out["weighted-loss"].item()),
         "messages": eng.syncbn_messages_per_step, "sync_bn": bool(eng.sync_bn), "live_groups": len(live),
         "live_scopes": sorted({o["bn"].split("/")[0].split("-")[0] for g in live for o in g.ops}),
         "rode": eng.small.c2_normalizer is not None, "pending": eng.small._c2_local is not None,
         "npos": float(targets["num-positives"].sum().item()),
         # the normaliser RetinaNetLoss computes for itself when none rode in a SyncBN message (retinanet_loss.py:38-49)
         "normalizer": float(global_normalizer(targets["num-positives"].sum().to(eng.dev), world, None).item())}
    del model, eng
    torch.cuda.empty_cache()
    return r


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out[rank] = {key: _dp_step(world, rank, key) for key in ("bn", "backbone-bn")}
    dist.destroy_process_group()


def test_two_ranks_with_frozen_batchnorm(cuda):
    """use_sync = True over two ranks.  freeze = ["bn"]: no SyncBN message at all, so the loss normaliser cannot ride in one
    (c2_normalizer stays None, nothing is left pending) and RetinaNetLoss all-reduces it itself — to the value the formula
    gives on the whole batch, (sum(num-positives) + replicas) / replicas; the weights match the one-process run of the
    doubled batch within test_two_ranks_match_one_process's tolerances.  freeze = ["backbone-bn"]: one forward and one
    backward message per LIVE BatchNorm launch group (a message carries all layers of a grouped launch: the head towers'
    levels), all of them FPN / head layers."""
    import torch.multiprocessing as mp
    single = {key: _dp_step(1, 0, key) for key in ("bn", "backbone-bn")}
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=False)   # two children, no more
    deadline = time.monotonic() + 240.0
    try:
        while not ctx.join(timeout=5.0):          # raises on the first non-zero exit, after ending the other child
            assert time.monotonic() < deadline, "a rank did not finish"
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
    r0, r1 = out[0], out[1]
    # ---- every BatchNorm frozen
    s, a, b = single["bn"], r0["bn"], r1["bn"]
    assert a["sync_bn"] and b["sync_bn"] and not s["sync_bn"]
    assert a["messages"] == 0 and b["messages"] == 0 and a["live_groups"] == 0
    assert not (a["rode"] or b["rode"] or a["pending"] or b["pending"])
    assert a["normalizer"] == b["normalizer"] == (a["npos"] + b["npos"] + 2.0) / 2.0
    assert a["npos"] + b["npos"] == s["npos"] and s["normalizer"] == s["npos"] + 1.0
    np.testing.assert_array_equal(a["P"], b["P"])
    upd_1, upd_2 = s["P"] - s["w0"], a["P"] - a["w0"]
    cos = float(np.dot(upd_1, upd_2) / (np.linalg.norm(upd_1) * np.linalg.norm(upd_2)))
    assert cos > 0.98, cos
    assert abs(np.linalg.norm(upd_2) / np.linalg.norm(upd_1) - 1) < 0.03
    assert 0.5 * (a["loss"] + b["loss"]) == pytest.approx(s["loss"], rel=0.02)
    # ---- the backbone's BatchNorm frozen, FPN + heads live
    a, b = r0["backbone-bn"], r1["backbone-bn"]
    assert a["live_groups"] > 0 and set(a["live_scopes"]) <= {"fpn", "box", "class"}
    assert a["messages"] == b["messages"] == 2 * a["live_groups"]
    assert a["rode"] and b["rode"] and not a["pending"]
    np.testing.assert_array_equal(a["P"], b["P"])
