"""RetinaNetLoss on the GPU (reference retinanet/losses/retinanet_loss.py:9-83 and
retinanet/losses/loss_impl.py:4-105).

`RetinaNetLoss(num_classes, params)(targets, predictions)` returns the reference's loss dict.
One fused HIP launch set computes the focal + Huber sums AND the gradients with respect to
every level's logits / box predictions (stored in `.grads` for the backward pass), so the
autograd tape of the reference is replaced by closed-form derivatives.

Distributed: the normaliser is all-reduced over `process_group` exactly where the reference
calls replica_context.all_reduce (retinanet_loss.py:46-49).  With `loss.normalizer.use_moving_average` it is instead the
reference's replica-local moving average of sum(num-positives) + 1 (retinanet_loss.py:19-44), a device scalar that
rn_loss_normalizer_ema updates in front of the loss launches: no all-reduce, no zero-debias.
"""
from __future__ import annotations

import logging

import torch

from retinanet import _C


class RetinaNetLoss:
    def __init__(self, num_classes, params, process_group=None):
        self._num_classes = int(num_classes)
        self._alpha = float(params.focal_loss.alpha)
        self._gamma = float(params.focal_loss.gamma)
        self._label_smoothing = float(params.focal_loss.label_smoothing)
        self._delta = float(params.smooth_l1_loss.delta)
        self._box_loss_weight = float(params.box_loss_weight)
        self._class_loss_weight = float(params.class_loss_weight)
        self._auxillary_loss_weight = float(params.auxillary_loss_weight)
        # loss.normalizer.use_moving_average (retinanet_loss.py:19-35): a replica-local f32 scalar that starts at 0.0
        # and is updated on the device by every call (rn_loss_normalizer_ema); created by the first call, on the
        # device of its targets
        self.use_moving_average_normalizer = bool(params.normalizer.use_moving_average)
        self.moving_average_normalizer = None
        if self.use_moving_average_normalizer:
            self.normalizer_momentum = float(params.normalizer.momentum)
            logging.warning("Using moving average loss normalizer with momentum: {}".format(self.normalizer_momentum))
        self._pg = process_group
        self._ws = None
        self.grads = None

    def _num_replicas(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self._pg)
        return 1

    def __call__(self, targets, predictions, compute_grads=True, grad_scale=None, grads_bf16=None, normalizer=None):
        """normalizer: optional device f32[1] = all_reduce_sum(sum(num-positives) + 1) / replicas already computed by
        the caller (the training engine folds that scalar into its first SyncBN message) — else computed here.
        grads_bf16 = {"class-predictions": {level: bf16[B,H,W,stride]}, "box-predictions": {...}}: write the
        gradients as bf16 into these (channel-padded) tensors instead of fp32 `self.grads` — the training engine
        passes the dy tensors of the prediction convs, so no fp32 gradient is materialised.
        With `iou-predictions` among the predictions (the auxiliary head, retinanet_loss.py:72-82) a second launch set
        adds the IoU-prediction loss: `iou-prediction-loss` and the updated `weighted-loss` are device scalars, the
        gradients go to `.grads["iou-predictions"]` / `grads_bf16["iou-predictions"]`."""
        lib = _C.lib()
        cls_pred = predictions["class-predictions"]
        box_pred = predictions["box-predictions"]
        levels = sorted(cls_pred.keys(), key=int)
        flat = targets["_flat"]
        cls_t, box_t = flat["class-targets"], flat["box-targets"]
        dev = cls_t.device
        B = cls_t.shape[0]
        K = self._num_classes
        # normaliser = all_reduce_sum(sum(num-positives) + 1) / replicas  (retinanet_loss.py:38-49)
        from retinanet.distribute import global_normalizer
        R = self._num_replicas()
        if self.use_moving_average_normalizer:
            # retinanet_loss.py:40-44: each replica updates and uses its own moving average — no all-reduce, no division
            # by the replica count, whatever the caller handed in; the update runs on every call (forward pass)
            if self.moving_average_normalizer is None:
                self.moving_average_normalizer = torch.zeros((1,), dtype=torch.float32, device=dev)
            npos = targets["num-positives"].to(dev, torch.float32).contiguous()
            normalizer = self.moving_average_normalizer
            with torch.cuda.device(dev):
                _C.check(lib.rn_loss_normalizer_ema(_C.ptr(npos), npos.numel(), self.normalizer_momentum,
                                                    _C.ptr(normalizer), _C.ptr(normalizer), _C.current_stream()),
                         "rn_loss_normalizer_ema")
        elif normalizer is None:
            normalizer = global_normalizer(targets["num-positives"].sum(), R, self._pg)
        else:
            normalizer = normalizer.reshape(1).to(torch.float32).contiguous()
        offs = [0]
        cl, bl = [], []
        for lv in levels:
            c = cls_pred[lv]
            b = box_pred[lv]
            if c.dtype != torch.float32 or b.dtype != torch.float32:
                raise TypeError("predictions must be float32 (the reference's prediction convs are fp32)")
            c = c.contiguous()
            b = b.contiguous()
            n_l = c.numel() // (B * K)
            offs.append(offs[-1] + n_l)
            cl.append(c)
            bl.append(b)
        if offs[-1] != cls_t.shape[1]:
            raise ValueError(f"predictions cover {offs[-1]} anchors, targets {cls_t.shape[1]}")
        bf16_out = compute_grads and grads_bf16 is not None
        dcl = [torch.empty_like(c) for c in cl] if compute_grads and not bf16_out else None
        dbl = [torch.empty_like(b) for b in bl] if compute_grads and not bf16_out else None
        need = lib.rn_loss_workspace_bytes(B, offs[-1], K)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        out = torch.empty((4,), dtype=torch.float32, device=dev)
        if grad_scale is None:
            grad_scale = 1.0 / R  # per_replica_loss = total / replicas  (executor.py:421)
        with torch.cuda.device(dev):
            if bf16_out:
                gc = [grads_bf16["class-predictions"][lv] for lv in levels]
                gb = [grads_bf16["box-predictions"][lv] for lv in levels]
                na = cl[0].shape[-1] // K
                for c, b, tc, tb in zip(cl, bl, gc, gb):
                    if (tc.dtype not in (torch.bfloat16, torch.float16) or tb.dtype != tc.dtype or not tc.is_contiguous()
                            or not tb.is_contiguous() or tc.shape[:-1] != c.shape[:-1] or tb.shape[:-1] != b.shape[:-1]
                            or tc.shape[-1] != gc[0].shape[-1] or tb.shape[-1] != gb[0].shape[-1]):
                        raise ValueError("grads_bf16 tensors must be contiguous 16-bit [B,H,W,stride] like the predictions")
                lib = _C.lib(gc[0].dtype == torch.float16)   # the build whose 16-bit type the gradient tensors hold
                _C.check(lib.rn_retinanet_loss_fwd_bwd_bf16(
                    _C.ptr_array(cl), _C.ptr_array(bl), _C.ptr_array(gc), _C.ptr_array(gb), gc[0].shape[-1],
                    gb[0].shape[-1], na, _C.i64_array(offs), len(levels), B, K, _C.ptr(cls_t), _C.ptr(box_t),
                    _C.ptr(normalizer), self._alpha, self._gamma, self._label_smoothing, self._delta,
                    self._box_loss_weight, self._class_loss_weight, float(grad_scale), _C.ptr(out), _C.ptr(self._ws),
                    self._ws.numel(), _C.current_stream()), "rn_retinanet_loss_fwd_bwd_bf16")
            else:
                _C.check(lib.rn_retinanet_loss_fwd_bwd(
                    _C.ptr_array(cl), _C.ptr_array(bl), _C.ptr_array(dcl), _C.ptr_array(dbl),
                    _C.i64_array(offs), len(levels), B, K, _C.ptr(cls_t), _C.ptr(box_t), _C.ptr(normalizer),
                    self._alpha, self._gamma, self._label_smoothing, self._delta, self._box_loss_weight,
                    self._class_loss_weight, float(grad_scale), _C.ptr(out), _C.ptr(self._ws), self._ws.numel(),
                    _C.current_stream()), "rn_retinanet_loss_fwd_bwd")
        if bf16_out:
            self.grads = None
        elif compute_grads:
            self.grads = {"class-predictions": dict(zip(levels, dcl)), "box-predictions": dict(zip(levels, dbl))}
        losses = {"box-loss": out[0], "class-loss": out[1], "weighted-loss": out[2],
                  "num-anchors-matched": out[3], "iou-prediction-loss": 0.0}
        if "iou-predictions" in predictions:
            iou = self._iou_loss(flat, predictions["iou-predictions"], levels, offs, B, normalizer, out[2:3],
                                 float(grad_scale), compute_grads, grads_bf16 if bf16_out else None)
            losses["iou-prediction-loss"], losses["weighted-loss"] = iou[0], iou[1]
        return losses

    def _iou_loss(self, flat, iou_pred, levels, offs, B, normalizer, weighted, grad_scale, compute_grads, grads_bf16):
        """IouPredictionLoss (loss_impl.py:108-131) over all levels: f32[2] = {iou-prediction-loss, weighted-loss +
        auxillary_loss_weight * iou-prediction-loss}, on the device; nothing here waits for the GPU."""
        if "iou-targets" not in flat:
            raise KeyError("the predictions hold `iou-predictions` but the targets no `iou-targets`: encode them with "
                           "architecture.auxillary_head.use_auxillary_head on")
        iou_t = flat["iou-targets"]
        dev = iou_t.device
        na = iou_pred[levels[0]].shape[-1]
        pl, strides = [], set()
        for i, lv in enumerate(levels):
            p = iou_pred[lv]
            if p.dtype != torch.float32:
                raise TypeError("predictions must be float32 (the reference's prediction convs are fp32)")
            if p.dim() != 4 or p.shape[-1] != na or p.numel() != B * (offs[i + 1] - offs[i]):
                raise ValueError(f"iou-predictions of level {lv}: shape {tuple(p.shape)} for "
                                 f"{offs[i + 1] - offs[i]} anchors per image, {na} per location")
            # the engines hand out the first `na` channels of the map their prediction conv writes (a multiple of 4
            # channels): such a view is read in place through its pixel stride
            base = p._base
            if (not p.is_contiguous() and base is not None and base.is_contiguous() and base.dim() == 4
                    and base.shape[:3] == p.shape[:3] and base.data_ptr() == p.data_ptr()):
                strides.add(int(base.shape[3]))
            else:
                p = p.contiguous()
                strides.add(na)
            pl.append(p)
        if len(strides) > 1:
            pl, strides = [p.contiguous() for p in pl], {na}
        pstride = strides.pop()
        if iou_t.shape[1] != offs[-1]:
            raise ValueError(f"predictions cover {offs[-1]} anchors, iou-targets {iou_t.shape[1]}")
        lib = _C.lib()
        need = lib.rn_iou_loss_workspace_bytes(B, offs[-1])
        if getattr(self, "_ws_iou", None) is None or self._ws_iou.numel() < need:
            self._ws_iou = torch.empty((need,), dtype=torch.uint8, device=dev)
        out = torch.empty((2,), dtype=torch.float32, device=dev)
        tail = (_C.i64_array(offs), len(levels), B, _C.ptr(iou_t), _C.ptr(normalizer), _C.ptr(weighted),
                self._auxillary_loss_weight, grad_scale, _C.ptr(out), _C.ptr(self._ws_iou), self._ws_iou.numel(),
                _C.current_stream())
        with torch.cuda.device(dev):
            if grads_bf16 is not None:
                gi = [grads_bf16["iou-predictions"][lv] for lv in levels]
                for p, t in zip(pl, gi):
                    if (t.dtype not in (torch.bfloat16, torch.float16) or t.dtype != gi[0].dtype or not t.is_contiguous()
                            or t.shape[:-1] != p.shape[:-1] or t.shape[-1] != gi[0].shape[-1] or t.shape[-1] < na):
                        raise ValueError("grads_bf16 tensors must be contiguous 16-bit [B,H,W,stride] like the predictions")
                lib = _C.lib(gi[0].dtype == torch.float16)   # the build whose 16-bit type the gradient tensors hold
                _C.check(lib.rn_iou_loss_fwd_bwd_bf16(_C.ptr_array(pl), pstride, _C.ptr_array(gi), gi[0].shape[-1], na,
                                                      *tail),
                         "rn_iou_loss_fwd_bwd_bf16")
            else:
                dl = [torch.empty(p.shape, dtype=torch.float32, device=dev) for p in pl] if compute_grads else None
                _C.check(lib.rn_iou_loss_fwd_bwd(_C.ptr_array(pl), pstride, na, _C.ptr_array(dl) if dl else None, *tail),
                         "rn_iou_loss_fwd_bwd")
                if compute_grads:
                    self.grads["iou-predictions"] = dict(zip(levels, dl))
        return out
