"""GPU: the auxiliary IoU head end to end — `iou-targets` from the label encoder, the IoU-prediction loss and its
gradients, one training step through the third head, serving with the head pruned.  References: tests/aux_ref.py
(float32 IoU targets, float64 loss) and the float64 model restatement oracle/model_ref.py, extended here."""
import re

import numpy as np
import pytest
import torch

import aux_ref

pytestmark = pytest.mark.gpu

SIZE, B, GMAX = 128, 2, 8
HEAD = "auxillary-head"
# six boxes (cx, cy, w, h): one per pyramid level 7 .. 3 sized like that level's anchors (the first equals the level-7
# base anchor: IoU exactly 1), and a small one no anchor overlaps by half, which only the forced match assigns
GT = np.array([[64, 64, 512, 512], [32, 32, 250, 260], [48, 80, 120, 130], [40, 24, 60, 70], [100, 100, 30, 34],
               [20, 100, 14, 18]], np.float32)
GT_CLS = np.array([3, 17, 5, 0, 79, 41], np.float32)


def _params(aux=True, weight=1.0, size=SIZE, num_convs=1, filters=64, **kw):
    from retinanet.cfg import default_params
    p = default_params(input_size=size, **kw)
    p.architecture.auxillary_head.use_auxillary_head = aux
    p.architecture.auxillary_head.num_convs = num_convs
    p.architecture.auxillary_head.filters = filters
    p.loss.auxillary_loss_weight = weight
    p.encoder_params.match_iou, p.encoder_params.ignore_iou = 0.5, 0.4
    p.architecture.batch_norm.use_sync = False
    return p


def _gt_batch(counts=(6, 0)):
    gb, gc = np.zeros([B, GMAX, 4], np.float32), np.zeros([B, GMAX], np.float32)
    for i, n in enumerate(counts):
        gb[i, :n], gc[i, :n] = GT[:n], GT_CLS[:n]
    return torch.from_numpy(gb), torch.from_numpy(gc), torch.tensor(list(counts), dtype=torch.int32)


@pytest.fixture(scope="module")
def encoded(cuda):
    """targets of (six boxes, no box) from the new entry point and from the old one, and the float32 reference"""
    from retinanet.dataloader import LabelEncoder
    enc, enc_old = LabelEncoder(_params(True), device=cuda), LabelEncoder(_params(False), device=cuda)
    new, old = enc.encode_batch(*_gt_batch()), enc_old.encode_batch(*_gt_batch())
    torch.cuda.synchronize()
    anchors = enc.anchors.boxes.cpu().numpy()
    ref_m = np.stack([aux_ref.match_anchor_boxes(anchors, GT, 0.5, 0.4),
                      aux_ref.match_anchor_boxes(anchors, GT[:0], 0.5, 0.4)])
    ref_t = np.stack([aux_ref.iou_targets_f32(anchors, GT, ref_m[0]), aux_ref.iou_targets_f32(anchors, GT[:0], ref_m[1])])
    return dict(enc=enc, new=new, old=old, anchors=anchors, ref_m=ref_m, ref_t=ref_t,
                bnd=[int(b) for b in enc.anchors.anchor_boundaries])


# ---- targets -----------------------------------------------------------------------------------------------------
def test_iou_targets_bit_identical_to_the_float32_reference(encoded):
    e = encoded
    A = e["anchors"].shape[0]
    assert A == 3069 and e["bnd"] == [0, 2304, 2880, 3024, 3060, 3069]
    m = e["new"]["_flat"]["matches"].cpu().numpy()
    assert np.array_equal(m, e["ref_m"])
    for i in range(5):      # the boxes were chosen for this: every level trains the head
        assert (m[0, e["bnd"][i]:e["bnd"][i + 1]] >= 0).any(), f"level {3 + i} has no positive anchor"
    assert (m[0] == -1).any() and (m[0] == -2).any() and (m[1] == -1).all()
    got = e["new"]["_flat"]["iou-targets"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (B, A)
    assert np.array_equal(got.view(np.uint32), e["ref_t"].view(np.uint32))
    assert (got[0][m[0] >= 0] > 0).all() and got[0].max() == 1.0 and (got[m < 0] == -1.0).all()


def test_other_targets_equal_the_old_entry_point(encoded):
    new, old = encoded["new"], encoded["old"]
    for k in ("matches", "class-targets", "box-targets"):
        a, b = new["_flat"][k], old["_flat"][k]
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert torch.equal(new["num-positives"].view(torch.int32), old["num-positives"].view(torch.int32))
    assert "iou-targets" not in old and "iou-targets" not in old["_flat"]


def test_per_level_views_and_single_sample(encoded):
    e = encoded
    flat = e["new"]["_flat"]["iou-targets"]
    assert sorted(e["new"]["iou-targets"]) == list("34567")
    for i, lv in enumerate("34567"):
        s = SIZE // 2 ** int(lv)
        v = e["new"]["iou-targets"][lv]
        assert tuple(v.shape) == (B, s, s, 9)
        assert torch.equal(v.reshape(B, -1), flat[:, e["bnd"][i]:e["bnd"][i + 1]])
    one = e["enc"].encode_sample(torch.from_numpy(GT), torch.from_numpy(GT_CLS))
    assert tuple(one["iou-targets"]["3"].shape) == (16, 16, 9)
    assert torch.equal(one["_flat"]["iou-targets"][0], flat[0])


# ---- loss --------------------------------------------------------------------------------------------------------
W_AUX, GSCALE = 0.75, 0.5     # exact in float32, so the float64 reference sees the very factors the kernel does


def _predictions(cuda, seed=5):
    rng = np.random.default_rng(seed)
    preds = {"class-predictions": {}, "box-predictions": {}, "iou-predictions": {}}
    for lv in "34567":
        s = SIZE // 2 ** int(lv)
        preds["class-predictions"][lv] = torch.from_numpy(rng.normal(-4.6, 1.0, (B, s, s, 9 * 80)).astype(np.float32)).to(cuda)
        preds["box-predictions"][lv] = torch.from_numpy(rng.normal(0, 0.3, (B, s, s, 36)).astype(np.float32)).to(cuda)
        preds["iou-predictions"][lv] = torch.from_numpy(rng.uniform(-2, 2, (B, s, s, 9)).astype(np.float32)).to(cuda)
    return preds


def _flat_levels(d):
    return np.concatenate([d[lv].float().cpu().numpy().reshape(B, -1) for lv in "34567"], axis=1)


@pytest.fixture(scope="module")
def loss_case(cuda, encoded):
    """the float64 reference of the loss and its gradient for one set of random predictions, computed once"""
    preds = _predictions(cuda)
    t = encoded["new"]["_flat"]["iou-targets"].cpu().numpy()
    normalizer = float(encoded["new"]["num-positives"].sum().item()) + 1.0
    ref_loss, ref_grad = aux_ref.iou_loss_f64(_flat_levels(preds["iou-predictions"]), t, normalizer, W_AUX, GSCALE)
    return dict(preds=preds, t=t, normalizer=normalizer, ref_loss=ref_loss, ref_grad=ref_grad)


def _loss(weight=W_AUX):
    from retinanet.losses import RetinaNetLoss
    return RetinaNetLoss(80, _params(True, weight).loss)


def test_iou_loss_and_f32_gradients_vs_float64(cuda, encoded, loss_case):
    c = loss_case
    loss = _loss()
    out = loss(encoded["new"], c["preds"], grad_scale=GSCALE)
    torch.cuda.synchronize()
    assert torch.is_tensor(out["iou-prediction-loss"]) and out["iou-prediction-loss"].is_cuda
    assert torch.is_tensor(out["weighted-loss"]) and out["weighted-loss"].is_cuda
    got_loss = out["iou-prediction-loss"].item()
    print("iou-prediction-loss", got_loss, "float64", c["ref_loss"], "rel", abs(got_loss - c["ref_loss"]) / c["ref_loss"])
    assert c["ref_loss"] > 0.1
    np.testing.assert_allclose(got_loss, c["ref_loss"], rtol=1e-5)      # tests/test_gpu_loss.py RTOL: the same kind of sum
    got = _flat_levels(loss.grads["iou-predictions"]).astype(np.float64)
    for lv in "34567":
        assert loss.grads["iou-predictions"][lv].shape == c["preds"]["iou-predictions"][lv].shape
    live = c["t"] > -1.0
    assert live.sum() == 134 and (got[~live] == 0.0).all()
    rel = np.abs(got[live] - c["ref_grad"][live]) / np.abs(c["ref_grad"][live])
    print("f32 gradient: max relative error %.3g (bound %.3g)" % (rel.max(), 8 * 2.0 ** -24))
    assert rel.max() <= 8 * 2.0 ** -24
    # the class and box gradients are there as before
    assert set(loss.grads) == {"class-predictions", "box-predictions", "iou-predictions"}


def test_weighted_loss_adds_the_auxiliary_term(cuda, encoded, loss_case):
    c = loss_case
    on = _loss()(encoded["new"], c["preds"], compute_grads=False)
    two = {k: v for k, v in c["preds"].items() if k != "iou-predictions"}
    off = _loss()(encoded["new"], two, compute_grads=False)
    torch.cuda.synchronize()
    assert off["iou-prediction-loss"] == 0.0 and isinstance(off["iou-prediction-loss"], float)   # today's dict
    for k in ("box-loss", "class-loss", "num-anchors-matched"):
        assert on[k].item() == off[k].item()
    want = np.float32(off["weighted-loss"].item()) + np.float32(W_AUX) * np.float32(on["iou-prediction-loss"].item())
    got = np.float32(on["weighted-loss"].item())
    print("weighted-loss", got, "expected", want)
    assert abs(float(got) - float(want)) <= float(np.spacing(np.float32(want)))


def _ulp_distance(a, b):
    """distance in representable values between two 16-bit float tensors of one dtype"""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16bit_gradients_into_padded_dy_tensors(cuda, encoded, loss_case, dtype):
    c = loss_case
    bufs = {"class-predictions": {}, "box-predictions": {}, "iou-predictions": {}}
    for lv in "34567":
        s = SIZE // 2 ** int(lv)
        bufs["class-predictions"][lv] = torch.zeros((B, s, s, 768), dtype=dtype, device=cuda)
        bufs["box-predictions"][lv] = torch.zeros((B, s, s, 64), dtype=dtype, device=cuda)
        bufs["iou-predictions"][lv] = torch.zeros((B, s, s, 64), dtype=dtype, device=cuda)
    loss = _loss()
    out = loss(encoded["new"], c["preds"], grad_scale=GSCALE, grads_bf16=bufs)
    torch.cuda.synchronize()
    assert loss.grads is None
    np.testing.assert_allclose(out["iou-prediction-loss"].item(), c["ref_loss"], rtol=1e-5)
    off, worst = 0, 0
    for lv in "34567":
        g = bufs["iou-predictions"][lv].cpu()
        n = g.shape[1] * g.shape[2] * 9
        assert (g[..., 9:].float() == 0).all() and (g[..., 9:].view(torch.int16) == 0).all(), f"level {lv}: pad channels"
        want = torch.from_numpy(c["ref_grad"][:, off:off + n]).to(dtype).reshape(B, g.shape[1], g.shape[2], 9)
        worst = max(worst, int(_ulp_distance(g[..., :9].contiguous(), want).max()))
        dead = torch.from_numpy(c["t"][:, off:off + n] <= -1.0).reshape(B, g.shape[1], g.shape[2], 9)
        assert (g[..., :9][dead].float() == 0).all()
        off += n
    print("16-bit gradient: worst distance", worst, "ulp")
    assert worst <= 1


def test_two_runs_are_bit_identical(cuda, encoded, loss_case):
    runs = []
    for _ in range(2):
        loss = _loss()
        out = loss(encoded["new"], loss_case["preds"], grad_scale=GSCALE)
        torch.cuda.synchronize()
        runs.append((out["iou-prediction-loss"].clone(), out["weighted-loss"].clone(),
                     [loss.grads["iou-predictions"][lv].clone() for lv in "34567"]))
    a, b = runs
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[2], b[2]))


def test_zero_box_batch(cuda, encoded, loss_case):
    targets = encoded["enc"].encode_batch(*_gt_batch((0, 0)))
    assert (targets["_flat"]["iou-targets"] == -1.0).all() and float(targets["num-positives"].sum()) == 0.0
    loss = _loss()
    out = loss(targets, loss_case["preds"])
    torch.cuda.synchronize()
    assert out["iou-prediction-loss"].item() == 0.0
    assert all((loss.grads["iou-predictions"][lv] == 0).all() for lv in "34567")
    bufs = {k: {lv: torch.zeros(tuple(loss_case["preds"][k][lv].shape[:3]) + (768 if k[0] == "c" else 64,),
                                dtype=torch.bfloat16, device=cuda) for lv in "34567"} for k in loss_case["preds"]}
    loss(targets, loss_case["preds"], grads_bf16=bufs)
    torch.cuda.synchronize()
    assert all((bufs["iou-predictions"][lv].view(torch.int16) & 0x7FFF == 0).all() for lv in "34567")


def test_targets_without_iou_are_refused(cuda, encoded, loss_case):
    with pytest.raises(KeyError, match="iou-targets"):
        _loss()(encoded["old"], loss_case["preds"])


# ---- training wiring -------------------------------------------------------------------------------------------------
TSIZE = 256


def _train_setup(cuda, aux, weight, seed=3):
    """ResNet-26, 256 x 256, two images, BalanceFeatures, stem + first block group frozen — the graph of
    tests/test_gpu_train_step.py — with a one-conv, 64-filter auxiliary head"""
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = _params(aux, weight, size=TSIZE, balanced=True)
    p.architecture.backbone.depth = 26
    model = ModelBuilder(p, "train", device=cuda, seed=seed)()
    g = torch.Generator().manual_seed(seed)
    for k, v in model.variables.items():        # the same draws, in the same order, with and without the head
        if k.startswith(HEAD):
            continue
        if k.endswith("/gamma"):
            lo, span = (0.1, 0.2) if model.graph.bns[k[:-len("/gamma")]]["gamma_zero"] else (0.75, 0.5)
            v.copy_((torch.rand(v.shape, generator=g) * span + lo).to(cuda))
        elif k.endswith("/beta"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(cuda))
        elif "head" in k and k.endswith("/kernel"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.02).to(cuda))
    ga = torch.Generator().manual_seed(seed + 100)
    for k, v in model.variables.items():
        if k.startswith(HEAD) and k.endswith("/kernel"):
            v.copy_((torch.randn(v.shape, generator=ga) * 0.05).to(cuda))
        elif k.startswith(HEAD) and k.endswith("/gamma"):
            v.copy_((torch.rand(v.shape, generator=ga) * 0.5 + 0.75).to(cuda))
    eng = TrainEngine(model, B, frozen_regexes=[re.compile(r"^(conv2d|batch_normalization)(_[1-7])?/")])
    enc = LabelEncoder(p, device=cuda)
    gb, gc, cnt = _gt_batch((6, 3))
    targets = enc.encode_batch(gb * (TSIZE / SIZE), gc, cnt)     # the same boxes on the larger image
    images = torch.randn((B, TSIZE, TSIZE, 3), generator=torch.Generator().manual_seed(seed + 1))
    return p, model, eng, targets, images


def _fwd_loss_bwd(eng, model, images, targets):
    """what TrainEngine.train_step does in front of the optimizer: forward, loss with 16-bit gradients written into the
    prediction convs' dy tensors, backward"""
    eng.G.zero_()
    preds = eng.forward(images.to(eng.dev))
    out = model.loss(targets, preds, compute_grads=True, grad_scale=1.0, grads_bf16=eng.loss_grad_buffers())
    eng.backward(None)
    torch.cuda.synchronize()
    return preds, out


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _engine_grad(eng, k):
    got = eng._pview(k, eng.G)
    if k.endswith("/kernel"):
        c = eng.g.convs[k[:-len("/kernel")]]
        got = got.reshape(c["cout"], c["k"], c["k"], c["cin"]).permute(1, 2, 3, 0)
    return got.cpu()


def _ref_trainer(p, variables, frozen, dtype):
    """oracle/model_ref.py::RefTrainer with the third head and the IoU-prediction loss (model/builder.py:70-101,
    losses/loss_impl.py:108-131)"""
    from model_ref import RefTrainer, _r

    class AuxRefTrainer(RefTrainer):
        def aux_head(self, feats):
            aux, act, outs = self.p.architecture.auxillary_head, self.p.architecture.activation.type, {}
            for level, x in feats.items():
                for i in range(aux.num_convs):
                    x = self._cs(x, f"{HEAD}/{HEAD}-{i}-conv2d")
                    x = self._bn(x, f"{HEAD}/{HEAD}-{i}-p{level}-{self.bn_tag}")
                    x = _r(self._act(x, act), self.bf)
                outs[level] = self._cs(x, f"{HEAD}/{HEAD}-prediction-conv2d", f32=True).permute(0, 2, 3, 1).contiguous()
            return outs

        def forward_train(self, images_nhwc):
            feats = self.fpn(self.backbone(images_nhwc.to(self.dtype)))
            if self.p.architecture.feature_fusion.use_balanced_features:
                feats = self.balance(feats)
            for f in feats.values():
                f.retain_grad()
            self.feats = feats
            return {"class-predictions": self.head(feats, "class-head"), "box-predictions": self.head(feats, "box-head"),
                    "iou-predictions": self.aux_head(feats)}

        def iou_loss(self, preds, iou_t, num_pos):
            n = iou_t.shape[0]
            x = torch.cat([preds["iou-predictions"][l].reshape(n, -1) for l in "34567"], dim=1)
            t = torch.as_tensor(iou_t, dtype=self.dtype)
            return (((x - t) ** 2) * (t > -1.0).to(self.dtype)).sum() / (float(num_pos) + 1.0)

    return AuxRefTrainer(p, variables, frozen_names=frozen, emulate_bf16=True, dtype=dtype)


def test_train_step_gradients_vs_float64_reference(cuda):
    """Forward, loss and backward of one training step with the head on, against autograd through the float64
    restatement with the same 16-bit rounding points.  Criterion of the head-tower checks in
    tests/test_gpu_train_step.py: the layers next to the loss > 0.995 cosine; every other tensor within 0.06 of the
    cosine the float32 evaluation of the same restatement reaches (its own arithmetic noise)."""
    # in the float64 restatement the auxiliary term's gradient at the pyramid is 0.46 - 0.59 of the two other heads' at
    # weight 1 (levels 3 .. 7): at weight 2 the two parts are about equal, so a missing or doubled part shows
    w = 2.0
    p, model, eng, targets, images = _train_setup(cuda, True, w)
    aux_names = [k for k in eng.train_names if k.startswith(HEAD)]
    assert len(aux_names) == 5 * 2 + 2 + 2 and set(eng.loss_grad_buffers()) == set(model.graph.outputs)
    assert all(tuple(t.shape[-1:]) == (64,) for t in eng.loss_grad_buffers()["iou-predictions"].values())
    preds, out = _fwd_loss_bwd(eng, model, images, targets)
    flat = targets["_flat"]
    npos = float(targets["num-positives"].sum().item())
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ref = _ref_trainer(p, model.variables, eng.frozen, dtype)
        rp = ref.forward_train(images)
        rl = ref.loss(rp, flat["class-targets"].cpu().numpy(), flat["box-targets"].cpu().numpy(), npos)
        iou = ref.iou_loss(rp, flat["iou-targets"].cpu().numpy(), npos)
        (rl["weighted-loss"] + w * iou).backward(retain_graph=True)
        at_pyramid = {lv: f.grad.clone() for lv, f in ref.feats.items()}     # (a later pass would add to .grad)
        aux_part = torch.autograd.grad(w * iou, list(ref.feats.values()))
        refs[dtype] = (ref, rp, rl, iou, aux_part, at_pyramid)
    ref, rp, rl, iou, aux_part, at_pyramid = refs[torch.float64]
    ref32, at_pyramid32 = refs[torch.float32][0], refs[torch.float32][5]
    assert set(eng.train_names) == set(ref.leaf)
    assert out["iou-prediction-loss"].item() == pytest.approx(float(iou.detach()), rel=0.02)
    assert out["weighted-loss"].item() == pytest.approx(float((rl["weighted-loss"] + w * iou).detach()), rel=0.02)
    for lv in "34567":
        got, want = preds["iou-predictions"][lv].float().cpu(), rp["iou-predictions"][lv].detach()
        assert tuple(got.shape) == tuple(want.shape) == (B, TSIZE // 2 ** int(lv), TSIZE // 2 ** int(lv), 9)
        assert (got.double() - want).norm() / want.norm() < 0.08, lv
    rows = {}
    for k in aux_names:
        if k.endswith("/bias") and "prediction" not in k:
            continue   # bias in front of BatchNorm: analytically zero gradient
        want = ref.leaf[k].grad
        got = _engine_grad(eng, k).reshape(want.shape)
        rows[k] = (_cos(got, want), _cos(ref32.leaf[k].grad, want), float(got.double().norm() / want.norm()))
        print("%-70s cos %.5f  floor %.5f  norm ratio %.4f" % ((k,) + rows[k]))
    assert len(rows) == 13
    assert rows[f"{HEAD}/{HEAD}-prediction-conv2d/kernel"][0] > 0.995
    assert rows[f"{HEAD}/{HEAD}-prediction-conv2d/bias"][0] > 0.995
    assert min(r[0] - r[1] for r in rows.values()) > -0.06, rows
    assert all(abs(r[2] - 1) < 0.35 for r in rows.values()), rows
    # the gradient that reaches the pyramid (BalanceFeatures' outputs): the sum of the three heads' contributions
    names = [o["inp"] for o in eng.ops if o.get("group") == "aux_tower0"]
    for i, (lv, name) in enumerate(zip("34567", names)):
        got = eng.grad["bal:" + name if name in eng.bal_src else name].float().cpu().permute(0, 3, 1, 2)
        want, want32 = at_pyramid[lv], at_pyramid32[lv]
        shares = (float(aux_part[i].norm() / want.norm()), float((want - aux_part[i]).norm() / want.norm()))
        cos, floor = _cos(got, want), _cos(want32, want)
        parts = (_cos(got, aux_part[i]), _cos(got, want - aux_part[i]))
        print("pyramid level %s: cos %.5f floor %.5f; against the auxiliary part alone %.5f, the two other heads alone %.5f "
              "(their shares of the norm %.3f, %.3f)" % ((lv, cos, floor) + parts + shares))
        assert cos > floor - 0.06, (lv, cos, floor)
        assert min(shares) > 0.25 and cos > max(parts) + 0.1, (lv, shares, cos, parts)
    # one whole step on top: finite, the loss dict carries the device scalar, the head's weights move
    before = {k: eng._pview(k).clone() for k in aux_names}
    step = eng.train_step(images.to(cuda), targets)
    torch.cuda.synchronize()
    assert torch.is_tensor(step["iou-prediction-loss"]) and np.isfinite(step["iou-prediction-loss"].item())
    assert np.isfinite(step["total-loss"].item()) and torch.isfinite(eng.P).all()
    moved = [k for k in aux_names if not torch.equal(before[k], eng._pview(k))]
    assert set(moved) >= {k for k in aux_names if not (k.endswith("/bias") and "prediction" not in k)}


def test_zero_weight_leaves_every_other_gradient_bit_identical(cuda):
    _, m_on, e_on, t_on, images = _train_setup(cuda, True, 0.0)
    _, m_off, e_off, t_off, _ = _train_setup(cuda, False, 0.0)
    shared = [k for k in e_off.train_names]
    assert shared == [k for k in e_on.train_names if not k.startswith(HEAD)]
    assert all(torch.equal(m_on.variables[k], m_off.variables[k]) for k in m_off.variables)
    _, out_on = _fwd_loss_bwd(e_on, m_on, images, t_on)
    _, out_off = _fwd_loss_bwd(e_off, m_off, images, t_off)
    assert out_on["weighted-loss"].item() == out_off["weighted-loss"].item()
    assert out_on["iou-prediction-loss"].item() > 0.0
    diff = [k for k in shared
            if not torch.equal(e_on._pview(k, e_on.G).view(torch.int32), e_off._pview(k, e_off.G).view(torch.int32))]
    assert not diff, diff[:8]
    assert sum(float(e_off._pview(k, e_off.G).abs().sum()) for k in shared) > 0
    for k in e_on.train_names:
        if k.startswith(HEAD):
            assert (e_on._pview(k, e_on.G) == 0).all(), k
    # the launches of the two other heads are the head-off engine's
    plan = lambda e: [n for n, _ in e.conv_launches if "aux" not in n and "pred_iou" not in n]
    assert plan(e_on) == plan(e_off)


def test_checkpoint_round_trip(cuda, tmp_path):
    _, model, eng, targets, images = _train_setup(cuda, True, 1.0)
    for _ in range(2):
        eng.train_step(images.to(cuda), targets)
    prefix = str(tmp_path / "weights_step_2")
    eng.save_checkpoint(prefix)
    _, model2, eng2, _, _ = _train_setup(cuda, True, 1.0, seed=11)
    aux_names = [k for k in eng.train_names if k.startswith(HEAD)]
    assert any(not torch.equal(eng._pview(k), eng2._pview(k)) for k in aux_names)
    eng2.restore_checkpoint(prefix)
    torch.cuda.synchronize()
    assert eng2.step_count == 2
    for k in aux_names:
        for arena, arena2 in ((eng.P, eng2.P), (eng.V, eng2.V), (eng.E, eng2.E)):
            assert torch.equal(eng._pview(k, arena).view(torch.int32), eng2._pview(k, arena2).view(torch.int32)), k
    stats = [k for k in model.variables if k.startswith(HEAD) and k.endswith(("/moving_mean", "/moving_variance"))]
    assert len(stats) == 10
    for k in stats:
        assert torch.equal(model.variables[k], model2.variables[k]), k
        assert not torch.equal(model.variables[k], torch.full_like(model.variables[k], 0.0 if "mean" in k else 1.0)), k
    assert torch.equal(eng.P.view(torch.int32), eng2.P.view(torch.int32))


def test_frozen_head_above_trainable_layers_is_refused(cuda):
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = _params(True, 1.0)
    builder = ModelBuilder(p, "train", device=cuda)
    with pytest.raises(NotImplementedError, match=HEAD):
        TrainEngine(builder(), B, frozen_regexes=[builder.FREEZE_VARS_REGEX["resnet_initial"]])


# ---- serving ---------------------------------------------------------------------------------------------------------
def test_serving_prunes_the_head(cuda):
    from retinanet.model import ModelBuilder
    b_on, b_off = ModelBuilder(_params(True), "val", device=cuda), ModelBuilder(_params(False), "val", device=cuda)
    for b in (b_on, b_off):
        b.params.inference.score_threshold = 0.005
    on, off = b_on(), b_off()
    assert all(torch.equal(on.variables[k], off.variables[k]) for k in off.variables)
    images = torch.randn((B, SIZE, SIZE, 3), generator=torch.Generator().manual_seed(1337)).to(cuda)
    raw = on(images, training=False)
    assert sorted(raw) == ["box-predictions", "class-predictions", "iou-predictions"]
    assert tuple(raw["iou-predictions"]["3"].shape) == (B, 16, 16, 9) and raw["iou-predictions"]["3"].dtype == torch.float32
    assert float(raw["iou-predictions"]["3"].abs().max()) > 0
    raw_off = off(images, training=False)
    for k in raw_off:
        assert all(torch.equal(raw[k][lv], raw_off[k][lv]) for lv in raw_off[k]), k
    for capture in (False, True):
        det_on = {k: v.clone() for k, v in b_on.add_post_processing_stage(on, capture_graph=capture)(images).items()}
        det_off = {k: v.clone() for k, v in b_off.add_post_processing_stage(off, capture_graph=capture)(images).items()}
        torch.cuda.synchronize()
        assert int(det_off["valid_detections"].sum()) > 0
        for k in det_off:
            assert det_on[k].dtype == det_off[k].dtype and torch.equal(det_on[k], det_off[k]), (k, capture)
    serve_on, serve_off = on.inference_engine(B, serving=True), off.inference_engine(B)
    assert [n for _, n in serve_on.steps] == [n for _, n in serve_off.steps]
    assert len(on.inference_engine(B).steps) > len(serve_on.steps)
    assert "iou-predictions" not in serve_on.outputs and off.inference_engine(B, serving=True) is serve_off
