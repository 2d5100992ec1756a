"""GPU: the focal + Huber loss kernels (csrc/rn_loss.hip) away from the workload's shapes and defaults.

  * every logit's gradient against float64 with a RELATIVE tolerance (tests/loss_ref.py: ELEM_RTOL = 4 x the error of a
    float32 restatement of the kernel's formula, measured against float64 — not against the kernel), where the other
    loss tests allow 1e-5 of the LARGEST gradient and so never see an easy example;
  * focal4_kernel's incremental index advance (more than one iteration per thread, a level with fewer anchors than one
    block stride), K / 4 = 1, 25 and 257, the scalar kernel's f32 and 16-bit stores, 1 and 8 levels;
  * alpha, delta, both loss weights, grad_scale and the normaliser off their defaults, Huber at |e| = delta,
    compute_grads=False, the refusals that return before any launch, run-to-run bit identity.
All cases go through RetinaNetLoss; the refusals call the library.  References: oracle.retinanet_loss (float64) and
oracle.focal_loss_elem / focal_loss_grad_elem."""

import numpy as np
import pytest
import torch

import loss_ref as L
import oracle as o

pytestmark = pytest.mark.gpu
RTOL = 1e-5                      # tests/test_gpu_loss.py: sums, and gradients relative to the largest one
ELEM_RTOL = L.elem_rtol()        # per element, relative to the element's own float64 value


def _loss_obj(K, **kw):
    from retinanet.cfg import default_params
    from retinanet.losses import RetinaNetLoss
    p = default_params()
    for k, v in kw.items():
        if k in ("alpha", "gamma", "label_smoothing"):
            p.loss.focal_loss[k] = v
        elif k == "delta":
            p.loss.smooth_l1_loss.delta = v
        else:
            assert k in ("box_loss_weight", "class_loss_weight"), k
            p.loss[k] = v
    return RetinaNetLoss(K, p.loss)


def _levels(cuda, arr, sizes, na, per):
    """[B, A, per] -> {level: [B, h, w, na * per]} on the device"""
    out, off = {}, 0
    for i, (h, w) in enumerate(sizes):
        n = h * w * na
        out[str(3 + i)] = torch.from_numpy(np.ascontiguousarray(arr[:, off:off + n]).reshape(arr.shape[0], h, w, na * per)).to(cuda)
        off += n
    assert off == arr.shape[1]
    return out


def _inputs(cuda, c):
    B = c["logits"].shape[0]
    preds = {"class-predictions": _levels(cuda, c["logits"], c["sizes"], c["na"], c["K"]),
             "box-predictions": _levels(cuda, c["box_preds"], c["sizes"], c["na"], 4)}
    targets = {"num-positives": torch.tensor([c["normalizer"] - 1.0] + [0.0] * (B - 1), device=cuda),
               "_flat": {"class-targets": torch.from_numpy(c["cls_t"]).to(cuda),
                         "box-targets": torch.from_numpy(c["box_t"]).to(cuda)}}
    return targets, preds


def _flat(grads, key, B, per):
    return torch.cat([grads[key][lv].reshape(B, -1, per) for lv in sorted(grads[key], key=int)], dim=1).cpu().numpy()


def _run(cuda, c, grad_scale=None, **kw):
    loss = _loss_obj(c["K"], **kw)
    targets, preds = _inputs(cuda, c)
    out = loss(targets, preds, grad_scale=grad_scale)
    torch.cuda.synchronize()
    B = c["logits"].shape[0]
    return ({k: (v.item() if torch.is_tensor(v) else v) for k, v in out.items()},
            _flat(loss.grads, "class-predictions", B, c["K"]), _flat(loss.grads, "box-predictions", B, 4))


def _case(seed, B, K, na, sizes, normalizer=None, mean=-2.0, std=5.0):
    """random logits over both sigmoid tails, ~5 % positive anchors, ~3 % ignored, one zero box-target coordinate"""
    rng = np.random.default_rng(seed)
    A = sum(h * w * na for h, w in sizes)
    logits = rng.normal(mean, std, (B, A, K)).astype(np.float32)
    box_preds = rng.normal(0, 0.3, (B, A, 4)).astype(np.float32)
    u = rng.random((B, A))
    cls_t = np.full((B, A), -1.0, np.float32)
    pos = u < 0.05
    cls_t[pos] = rng.integers(0, K, int(pos.sum()))
    cls_t[(u >= 0.05) & (u < 0.08)] = -2.0
    cls_t[0, 0], cls_t[-1, -1], cls_t[-1, -2] = K - 1, 0.0, -2.0      # the corners of the index space
    pos = cls_t >= 0
    box_t = np.zeros((B, A, 4), np.float32)
    box_t[pos] = rng.normal(0, 0.5, (int(pos.sum()), 4))
    box_t[0, 0, 1] = 0.0
    return dict(K=K, na=na, sizes=sizes, logits=logits, box_preds=box_preds, cls_t=cls_t, box_t=box_t,
                normalizer=float(pos.sum()) + 1.0 if normalizer is None else float(normalizer))


def _check_vs_oracle(c, got, gamma=1.5, ls=0.0, **ref_kw):
    out, dl, db = got
    ref, rdl, rdb = o.retinanet_loss(c["logits"], c["box_preds"], c["cls_t"], c["box_t"], c["normalizer"], c["K"],
                                     gamma=gamma, label_smoothing=ls, **ref_kw)
    for k in ("class-loss", "box-loss", "weighted-loss"):
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, err_msg=k)
    assert out["num-anchors-matched"] == c["normalizer"]
    np.testing.assert_allclose(dl, rdl, rtol=RTOL, atol=RTOL * np.abs(rdl).max())
    np.testing.assert_allclose(db, rdb, rtol=RTOL, atol=RTOL * np.abs(rdb).max())
    ign = c["cls_t"] == -2.0
    assert ign.any() and (dl[ign] == 0).all()
    assert (db[c["box_t"] == 0] == 0).all()
    if ls == 0.0:
        live = (np.abs(c["logits"]) <= 20.0) & ~ign[..., None]
        rel = np.abs(dl[live] - rdl[live]) / np.abs(rdl[live])
        print("K %d: worst relative gradient error over %d logits with |x| <= 20: %.3g (bound %.3g)"
              % (c["K"], live.sum(), rel.max(), ELEM_RTOL))
        assert rel.max() <= ELEM_RTOL
    return ref, rdl, rdb


# ---- every logit's loss and gradient against float64 ------------------------------------------------------------------
def _sweep_case(K):
    """one level, B = 1, normaliser 1, weights 1: K = 4 — 4096 anchors, anchor a holds x_a in all four logits and is
    positive in class a % 4, so every x meets both labels and every class slot is the positive one in turn; K = 1
    (scalar kernel, a matched anchor has no negative logit) — anchors 2i / 2i + 1 hold x_i as a positive / a negative"""
    x = np.linspace(-20.0, 20.0, 4096).astype(np.float32)
    if K == 4:
        logits = np.repeat(x[None, :, None], 4, axis=2).copy()
        cls_t = (np.arange(4096) % 4).astype(np.float32)[None]
    else:
        logits = np.repeat(x, 2)[None, :, None].copy()
        cls_t = np.where(np.arange(8192) % 2 == 0, 0.0, -1.0).astype(np.float32)[None]
    A = logits.shape[1]
    ignored = [5, 6, 1000, 2047, A - 2, A - 1]
    cls_t[0, ignored] = -2.0
    return dict(K=K, na=1, sizes=[(A // 64, 64)], logits=logits, box_preds=np.zeros((1, A, 4), np.float32), cls_t=cls_t,
                box_t=np.zeros((1, A, 4), np.float32), normalizer=1.0), ignored


@pytest.mark.parametrize("K", [4, 1])
@pytest.mark.parametrize("gamma,ls", [(1.5, 0.0), (2.0, 0.0), (0.5, 0.0), (1.5, 0.1), (2.0, 0.1), (0.5, 0.1)])
def test_every_gradient_within_elem_rtol_of_float64(cuda, K, gamma, ls):
    c, ignored = _sweep_case(K)
    out, dl, db = _run(cuda, c, gamma=gamma, label_smoothing=ls, class_loss_weight=1.0, box_loss_weight=1.0)
    y = (np.arange(K)[None, None, :] == c["cls_t"].astype(np.int32)[..., None])
    want = o.focal_loss_grad_elem(c["logits"], y.astype(np.float64), 0.25, gamma, ls)
    live = np.ones(c["cls_t"].shape, bool)
    live[0, ignored] = False
    assert (dl[~live] == 0).all() and (db == 0).all() and out["box-loss"] == 0.0
    got, want, pos, x = dl[live], want[live], y[live], c["logits"][live]
    assert pos.sum() >= 4000 and (~pos).sum() >= 4000 and np.isfinite(got).all()
    err = np.abs(got - want)
    rel = err / np.abs(want)
    for name, m in (("positives", pos), ("negatives", ~pos)):
        i = np.argmax(np.where(m, rel, 0))
        print("K %d gamma %.1f ls %.1f %s: worst relative error %.3g at x = %.4f (bound %.3g)"
              % (K, gamma, ls, name, rel.flat[i], x.flat[i], ELEM_RTOL))
    if ls == 0.0:
        assert (err <= ELEM_RTOL * np.abs(want)).all()
    else:
        assert (err <= L.mixed_bound(want, ELEM_RTOL)).all()
    total = o.focal_loss_elem(c["logits"], y.astype(np.float64), 0.25, gamma, ls)[live].sum()
    np.testing.assert_allclose(out["class-loss"], total, rtol=RTOL)


@pytest.mark.parametrize("K", [4, 1])
@pytest.mark.parametrize("gamma,ls", [(1.5, 0.0), (2.0, 0.1), (0.5, 0.0)])
def test_logits_where_float32_underflows_stay_finite(cuda, K, gamma, ls):
    """|x| in {40, 88, 100, 1e4}: e^-|x| is tiny, subnormal or 0 in float32, so only an absolute bound can hold:
    1e-6 of the largest gradient (the x = 0, +-1, +-5 anchors among them)"""
    xs = np.array([40, 88, 100, 1e4, 0, 1, 5], np.float32)
    xs = np.concatenate([xs, -xs])
    reps = 8 if K == 4 else 2
    x = np.repeat(xs, reps)
    A = x.size
    logits = np.repeat(x[None, :, None], K, axis=2).copy()
    cls_t = ((np.arange(A) % 4).astype(np.float32) if K == 4 else np.where(np.arange(A) % 2 == 0, 0.0, -1.0))
    cls_t = cls_t.astype(np.float32)[None].copy()
    if K == 4:
        cls_t[0, 4::8] = -1.0                       # all-background anchors too
    c = dict(K=K, na=1, sizes=[(1, A)], logits=logits, box_preds=np.zeros((1, A, 4), np.float32), cls_t=cls_t,
             box_t=np.zeros((1, A, 4), np.float32), normalizer=1.0)
    out, dl, _ = _run(cuda, c, gamma=gamma, label_smoothing=ls)
    y = (np.arange(K)[None, None, :] == cls_t.astype(np.int32)[..., None]).astype(np.float64)
    with np.errstate(over="ignore"):
        want = o.focal_loss_grad_elem(logits, y, 0.25, gamma, ls)
        total = o.focal_loss_elem(logits, y, 0.25, gamma, ls).sum()
    assert np.isfinite(want).all() and np.isfinite(dl).all() and np.isfinite(out["class-loss"])
    err = np.abs(dl - want).max()
    print("K %d gamma %.1f ls %.1f: worst absolute error %.3g of max |grad| %.3g" % (K, gamma, ls, err, np.abs(want).max()))
    assert err <= 1e-6 * np.abs(want).max()
    np.testing.assert_allclose(out["class-loss"], total, rtol=RTOL)


@pytest.mark.parametrize("x", [-30.0, -10.0, -4.595, 0.0, 5.0, 10.0, 20.0])
@pytest.mark.parametrize("K", [4, 1], ids=["background-K4", "positive-K1"])
def test_known_answer_sums(cuda, K, x):
    """every logit equal: class-loss = N L(x) — the per-element LOSS, which the kernels only return summed"""
    A = 4096
    xf = np.float32(x)
    c = dict(K=K, na=1, sizes=[(64, 64)], logits=np.full((1, A, K), xf, np.float32),
             box_preds=np.zeros((1, A, 4), np.float32), cls_t=np.full((1, A), -1.0 if K == 4 else 0.0, np.float32),
             box_t=np.zeros((1, A, 4), np.float32), normalizer=1.0)
    out, dl, _ = _run(cuda, c)
    y = 0.0 if K == 4 else 1.0
    want = A * K * float(o.focal_loss_elem(np.float64(xf), y, 0.25, 1.5, 0.0))
    print("x %g %s: class-loss %.9g, N L(x) %.9g, relative error %.3g (bound %.3g)"
          % (x, "background" if K == 4 else "positive", out["class-loss"], want, abs(out["class-loss"] - want) / want, ELEM_RTOL))
    assert want > 0 and abs(out["class-loss"] - want) <= ELEM_RTOL * want
    g = float(o.focal_loss_grad_elem(np.float64(xf), y, 0.25, 1.5, 0.0))
    assert (dl == dl.flat[0]).all() and abs(float(dl.flat[0]) - g) <= ELEM_RTOL * abs(g)


# ---- index arithmetic -------------------------------------------------------------------------------------------------
def _chunk(items_per_level):
    """the launcher's choice (loss_launch): float4 items per workgroup, the smallest multiple of 256 that keeps the
    launch inside 2048 workgroups, starting at one iteration per 2000 * 256 items"""
    total = sum(items_per_level)
    iters = max(1, -(-total // (2000 * 256)))
    while sum(-(-n // (iters * 256)) for n in items_per_level) > 2048:
        iters += 1
    return iters * 256


@pytest.mark.parametrize("K,na,B,sizes,gamma", [
    (4, 3, 2, [(8, 8), (4, 4), (2, 2)], 1.5),                                   # K / 4 = 1
    (100, 2, 3, [(5, 5), (3, 3), (1, 1)], 1.5),                                 # K / 4 = 25: no divisor of 256
    (1028, 3, 2, [(12, 12), (6, 6), (3, 3), (1, 1)], 2.0),                      # K / 4 = 257 > 256; A = 570
    (8, 1, 2, [(7, 7)], 1.5),                                                   # one level
    (8, 2, 2, [(9, 8), (7, 7), (5, 6), (4, 4), (3, 3), (2, 2), (2, 1), (1, 1)], 2.0),   # eight levels
    (6, 9, 4, [(32, 32), (16, 16), (8, 8)], 1.5),                               # scalar kernel, 290 k logits
    (90, 9, 2, [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], 1.5),              # scalar kernel, grid-stride loop (2.2 M)
], ids=["K4", "K100", "K1028", "1level", "8levels", "K6", "K90"])
def test_index_arithmetic_vs_oracle(cuda, K, na, B, sizes, gamma):
    c = _case(K, B, K, na, sizes)
    if K % 4:
        assert (B * c["logits"].shape[1] * K > 2048 * 256) == (K == 90)       # K90: more logits than one grid pass
    else:
        assert _chunk([B * h * w * na * (K // 4) for h, w in sizes]) == 256
    _check_vs_oracle(c, _run(cuda, c, gamma=gamma), gamma=gamma)


MI = dict(K=8, na=3, B=1500, sizes=[(16, 16), (1, 1)])


@pytest.fixture(scope="module")
def multi_iter(cuda):
    """focal4_kernel with several iterations per thread and a level smaller than one block stride: the case, its float64
    reference and the f32 results (device tensors), computed once"""
    K, na, B, sizes = MI["K"], MI["na"], MI["B"], MI["sizes"]
    items = [B * h * w * na * (K // 4) for h, w in sizes]
    chunk = _chunk(items)
    n_small = sizes[1][0] * sizes[1][1] * na
    assert sum(items) > 2000 * 256 and chunk > 256, "the case no longer makes a thread iterate"
    assert n_small < 256 // (K // 4), "the case no longer wraps more than one image per block stride"
    assert items[1] > chunk, "the small level no longer spans workgroups"
    c = _case(11, B, K, na, sizes)
    A = c["logits"].shape[1]
    rng = np.random.default_rng(12)
    last = np.arange(B - 40, B)
    c["cls_t"][last, A - n_small:] = rng.choice([-2.0, -1.0, 0.0, 3.0, 7.0], (40, n_small)).astype(np.float32)
    pos = c["cls_t"] >= 0
    c["box_t"] = np.where(pos[..., None], rng.normal(0, 0.5, c["box_t"].shape), 0).astype(np.float32)
    c["normalizer"] = float(pos.sum()) + 1.0
    assert (c["cls_t"][last, A - n_small:] >= 0).any() and (c["cls_t"][last, A - n_small:] == -2).any()
    loss = _loss_obj(K)
    targets, preds = _inputs(cuda, c)
    out = loss(targets, preds)
    torch.cuda.synchronize()
    return dict(c=c, chunk=chunk, loss=loss, targets=targets, preds=preds, grads=loss.grads,
                out={k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()})


def test_multi_iteration_advance_vs_oracle(cuda, multi_iter):
    m, B = multi_iter, MI["B"]
    print("chunk", m["chunk"], "float4 items per workgroup:", m["chunk"] // 256, "iterations per thread")
    got = ({k: (v.item() if torch.is_tensor(v) else v) for k, v in m["out"].items()},
           _flat(m["grads"], "class-predictions", B, MI["K"]), _flat(m["grads"], "box-predictions", B, 4))
    _check_vs_oracle(m["c"], got)


def test_multi_iteration_case_is_bit_identical_from_run_to_run(cuda, multi_iter):
    m = multi_iter
    loss = _loss_obj(MI["K"])
    out = loss(m["targets"], m["preds"])
    torch.cuda.synchronize()
    for k in ("box-loss", "class-loss", "weighted-loss", "num-anchors-matched"):
        assert torch.equal(out[k].view(torch.int32), m["out"][k].view(torch.int32)), k
    for key in ("class-predictions", "box-predictions"):
        for lv in m["grads"][key]:
            assert torch.equal(loss.grads[key][lv].view(torch.int32), m["grads"][key][lv].view(torch.int32)), (key, lv)


def _check_16bit(cuda, loss, targets, preds, out32, g32, live_c, live_b, cs, bs, dtype):
    """the 16-bit outputs are, bit for bit, the round-to-nearest-even cast of the f32 gradients; pad channels untouched"""
    bufs = {key: {lv: torch.full(tuple(t.shape[:3]) + (stride,), 7.0, dtype=dtype, device=cuda)
                  for lv, t in preds[key].items()}
            for key, stride in (("class-predictions", cs), ("box-predictions", bs))}
    out16 = loss(targets, preds, grads_bf16=bufs)
    torch.cuda.synchronize()
    assert loss.grads is None
    for k in ("box-loss", "class-loss", "weighted-loss"):
        assert out32[k].item() == out16[k].item(), k
    for key, live in (("class-predictions", live_c), ("box-predictions", live_b)):
        for lv, got in bufs[key].items():
            assert torch.equal(got[..., :live].view(torch.int16), g32[key][lv].to(dtype).view(torch.int16)), (key, lv)
            assert bool((got[..., live:] == 7.0).all()), (key, lv)
        assert max(float(t.abs().max()) for t in g32[key].values()) > 0, key


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_multi_iteration_16bit_gradients_match_the_cast(cuda, multi_iter, dtype):
    """the pixel / channel advance of the 16-bit store (padded strides 32 and 16 for 24 and 12 live channels); float16
    tensors go to the library built for half storage"""
    m = multi_iter
    _check_16bit(cuda, _loss_obj(MI["K"]), m["targets"], m["preds"], m["out"], m["grads"], 24, 12, 32, 16, dtype)


@pytest.mark.parametrize("K,na,cs", [(6, 3, 20), (90, 2, 184)])
def test_scalar_kernel_16bit_gradients_match_the_cast(cuda, K, na, cs):
    """K % 4 != 0: focal_kernel<1> packs and stores one 16-bit gradient per logit, not one quad"""
    c = _case(100 + K, 2, K, na, [(4, 4), (3, 2), (1, 1)])
    loss = _loss_obj(K)
    targets, preds = _inputs(cuda, c)
    out32 = loss(targets, preds)
    g32 = loss.grads
    _check_16bit(cuda, loss, targets, preds, out32, g32, na * K, na * 4, cs, 4 * ((na * 4 + 3) // 4) + 4, torch.bfloat16)
    _check_vs_oracle(c, ({k: (v.item() if torch.is_tensor(v) else v) for k, v in out32.items()},
                         _flat(g32, "class-predictions", 2, K), _flat(g32, "box-predictions", 2, 4)))


# ---- refusals that return before any launch (loss_launch: every RN_CHECK_ARG below sits in front of the first kernel) --
def _raw(cuda, offs, B=1, K=4, strides=None, na=1):
    from retinanet import _C
    lib = _C.lib()
    nl = len(offs) - 1
    n = max(1, max(offs))
    cl = [torch.zeros((B * n * K,), device=cuda) for _ in range(nl)]
    bl = [torch.zeros((B * n * 4,), device=cuda) for _ in range(nl)]
    dcl, dbl = [torch.full_like(t, 3.0) for t in cl], [torch.full_like(t, 3.0) for t in bl]
    cls_t, box_t = torch.full((B, n), -1.0, device=cuda), torch.zeros((B, n, 4), device=cuda)
    norm, out = torch.ones((1,), device=cuda), torch.full((4,), -9.0, device=cuda)
    ws = torch.empty((lib.rn_loss_workspace_bytes(B, n, K),), dtype=torch.uint8, device=cuda)
    tail = (_C.i64_array(offs), nl, B, K, _C.ptr(cls_t), _C.ptr(box_t), _C.ptr(norm), 0.25, 1.5, 0.0, 0.1, 50.0, 1.0, 1.0,
            _C.ptr(out), _C.ptr(ws), ws.numel(), _C.current_stream())
    if strides is None:
        st = lib.rn_retinanet_loss_fwd_bwd(_C.ptr_array(cl), _C.ptr_array(bl), _C.ptr_array(dcl), _C.ptr_array(dbl), *tail)
    else:
        g16 = [torch.full((B * n * 64,), 3.0, dtype=torch.bfloat16, device=cuda) for _ in range(nl)]
        st = lib.rn_retinanet_loss_fwd_bwd_bf16(_C.ptr_array(cl), _C.ptr_array(bl), _C.ptr_array(g16), _C.ptr_array(g16),
                                                strides[0], strides[1], na, *tail)
    torch.cuda.synchronize()
    untouched = bool((out == -9.0).all()) and all(bool((t == 3.0).all()) for t in dcl + dbl)
    return st, (lib.rn_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("kw,msg", [
    (dict(offs=list(range(0, 40, 4))), "bad num_levels=9"),                     # nine levels
    (dict(offs=[4, 8]), "level_offsets[0] must be 0"),
    (dict(offs=[0, 4, 4, 8]), "empty level 1"),
    (dict(offs=[0, 6], K=8, na=3, strides=(20, 12)), "bad strides 20 / 12"),    # class stride below na * K
    (dict(offs=[0, 6], K=8, na=3, strides=(26, 12)), "bad strides 26 / 12"),    # not a multiple of 4
    (dict(offs=[0, 6], K=8, na=3, strides=(24, 14)), "bad strides 24 / 14"),
], ids=["nine-levels", "offset0", "empty-level", "class-stride-small", "class-stride-odd", "box-stride-odd"])
def test_refusals_before_any_launch(cuda, kw, msg):
    from retinanet import _C
    st, err, untouched = _raw(cuda, **kw)
    assert st == _C.RN_EINVAL and msg in err and untouched, (st, err)


def test_eight_levels_are_accepted_by_the_library(cuda):
    st, err, untouched = _raw(cuda, offs=list(range(0, 36, 4)))
    assert st == 0 and not untouched, err


# ---- parameters off their defaults ------------------------------------------------------------------------------------
def test_every_loss_parameter_off_its_default(cuda):
    kw = dict(alpha=0.4, delta=0.5, box_loss_weight=3.0, class_loss_weight=2.0)
    c = _case(21, 2, 8, 3, [(12, 10), (6, 5), (3, 2)], normalizer=37.0)
    c["box_preds"] *= 2.0                                    # both Huber regions at delta = 0.5
    e = np.abs(c["box_preds"] - c["box_t"])[c["box_t"] != 0]
    assert (e > 0.5).sum() > 20 and (e < 0.5).sum() > 20
    got = _run(cuda, c, grad_scale=1024.0, **kw)
    _check_vs_oracle(c, got, grad_scale=1024.0, **kw)
    # the loss scale reaches the gradients and only them
    base = _run(cuda, c, grad_scale=1.0, **kw)
    assert all(got[0][k] == base[0][k] for k in got[0])
    assert np.array_equal(got[1], base[1] * np.float32(1024)) and np.array_equal(got[2], base[2] * np.float32(1024))


def test_huber_at_delta_and_zero_targets(cuda):
    """delta = 0.5, box weight 4, normaliser 1, grad_scale 1: the gradient factor is exactly 1, so the gradient must BE
    e (|e| <= delta) or +-delta, bit for bit.  A target of 0.0 or -0.0 switches the coordinate off."""
    d = np.float32(0.5)
    below, above = np.nextafter(np.float32(1.5), np.float32(0)), np.nextafter(np.float32(1.5), np.float32(2))
    # (prediction, target) pairs; e = p - t is exact in float32 for each
    pairs = [(1.5, 1.0), (below, 1.0), (above, 1.0), (0.5, 1.0), (2.0 - below, 1.0), (2.0 - above, 1.0),
             (4.0, 1.0), (-2.0, 1.0), (1.25, 1.0), (0.875, 1.0), (3.0, 0.0), (-3.0, -0.0), (0.25, 0.0), (0.0, -0.0),
             (-1.0, -1.5), (-1.5, -1.0)]
    p = np.array([a for a, _ in pairs], np.float32).reshape(1, 4, 4)
    t = np.array([b for _, b in pairs], np.float32).reshape(1, 4, 4)
    assert np.signbit(t[0, 2, 3]) and np.signbit(t[0, 3, 1])
    c = dict(K=4, na=1, sizes=[(2, 2)], logits=np.zeros((1, 4, 4), np.float32), box_preds=p,
             cls_t=np.zeros((1, 4), np.float32), box_t=t, normalizer=1.0)
    out, _, db = _run(cuda, c, delta=0.5, box_loss_weight=4.0)
    e = (p - t).astype(np.float32)
    assert np.array_equal((p.astype(np.float64) - t).astype(np.float32), e)
    want = np.where(np.abs(e) <= d, e, np.where(e > 0, d, -d)).astype(np.float32)
    want[t == 0] = 0.0
    assert sorted(set(np.abs(e[0, 0]) - d)) == sorted({0.0, float(below - 1.5), float(above - 1.5)})
    assert np.array_equal(db, want), (db, want)
    assert (db[0, 2, 2:] == 0).all() and (db[0, 3, :2] == 0).all()                 # 0.0 and -0.0 targets
    assert db[0, 1, 2] == d and db[0, 1, 3] == -d                                  # both signs of the linear region
    ref = o.retinanet_loss(c["logits"], p, c["cls_t"], t, 1.0, 4, delta=0.5, box_loss_weight=4.0)[0]
    np.testing.assert_allclose(out["box-loss"], ref["box-loss"], rtol=1e-6)


def test_compute_grads_false_same_scalars_and_grads_left_alone(cuda):
    c = _case(31, 2, 8, 3, [(4, 4), (2, 2)])
    loss = _loss_obj(8)
    targets, preds = _inputs(cuda, c)
    a = {k: v.clone() for k, v in loss(targets, preds).items() if torch.is_tensor(v)}
    grads = loss.grads
    keep = {key: {lv: t.clone() for lv, t in d.items()} for key, d in grads.items()}
    b = loss(targets, preds, compute_grads=False)
    torch.cuda.synchronize()
    assert sorted(a) == ["box-loss", "class-loss", "num-anchors-matched", "weighted-loss"]
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert loss.grads is grads
    assert all(torch.equal(grads[key][lv], keep[key][lv]) for key in keep for lv in keep[key])
    fresh = _loss_obj(8)
    fresh(targets, preds, compute_grads=False)
    assert fresh.grads is None
