"""Independent numpy references for the auxiliary IoU head, written from the reference's own lines:

* `iou_elementwise_f32` / `iou_targets_f32`: dataloader/utils.py:17-46 with pair_wise=False and
  dataloader/label_encoder.py:96-97 — float32, one rounding per TensorFlow op (numpy float32 arithmetic rounds every
  add / multiply / divide once, to nearest even, as the separate TF kernels do);
* `match_anchor_boxes`: label_encoder.py:27-55 on the same float32 IoU, for choosing test boxes and checking them;
* `iou_loss_f64`: losses/loss_impl.py:108-131 and losses/retinanet_loss.py:72-82 — the masked sum-reduced MSE, its
  normalisation and its gradient in float64.
"""
import numpy as np

F32 = np.float32


def _corners(b):
    half = b[..., 2:] / F32(2.0)
    return np.concatenate([b[..., :2] - half, b[..., :2] + half], axis=-1)


def iou_elementwise_f32(boxes1, boxes2):
    """compute_iou(boxes1, boxes2, pair_wise=False): row i of boxes1 against row i of boxes2, both f32[N,4] cxcywh"""
    b1, b2 = np.asarray(boxes1, F32), np.asarray(boxes2, F32)
    c1, c2 = _corners(b1), _corners(b2)
    lu = np.maximum(c1[:, :2], c2[:, :2])
    rd = np.minimum(c1[:, 2:], c2[:, 2:])
    inter = np.maximum(F32(0.0), rd - lu)
    inter_area = inter[:, 0] * inter[:, 1]
    a1 = b1[:, 2] * b1[:, 3]
    a2 = b2[:, 2] * b2[:, 3]
    union = np.maximum((a1 + a2) - inter_area, F32(1e-8))
    out = np.clip(inter_area / union, F32(0.0), F32(1.0))
    assert out.dtype == F32
    return out


def iou_pairwise_f32(gt_boxes, anchors):
    """compute_iou(gt_boxes, anchors, pair_wise=True) -> f32[G, A]"""
    g, a = np.asarray(gt_boxes, F32), np.asarray(anchors, F32)
    G, A = g.shape[0], a.shape[0]
    return iou_elementwise_f32(np.repeat(g, A, axis=0), np.tile(a, (G, 1))).reshape(G, A)


def match_anchor_boxes(anchors, gt_boxes, match_iou, ignore_iou):
    """label_encoder.py:27-55 -> i32[A] in {-2, -1, 0 .. G-1}"""
    anchors = np.asarray(anchors, F32)
    gt_boxes = np.asarray(gt_boxes, F32).reshape(-1, 4)
    A = anchors.shape[0]
    if gt_boxes.shape[0] == 0:
        return np.full([A], -1, np.int32)
    iou = iou_pairwise_f32(gt_boxes, anchors)
    max_ious = iou.max(axis=0)
    matches = np.where(max_ious > F32(match_iou), iou.argmax(axis=0), -1)
    matches = np.where((max_ious >= F32(ignore_iou)) & (F32(match_iou) > max_ious), -2, matches)
    best = iou.argmax(axis=1)                       # per GT: its best anchor (first maximum)
    one_hot = np.zeros(iou.shape, np.float32)
    one_hot[np.arange(gt_boxes.shape[0]), best] = 1.0
    forced = one_hot.max(axis=0) > 0
    matches = np.where(forced, one_hot.argmax(axis=0), matches)
    return matches.astype(np.int32)


def iou_targets_f32(anchors, gt_boxes, matches):
    """label_encoder.py:79-97: gather from the GT boxes padded with two zero rows, elementwise IoU against the anchors,
    -1 wherever matches <= -1"""
    anchors = np.asarray(anchors, F32)
    gt_pad = np.concatenate([np.zeros([2, 4], F32), np.asarray(gt_boxes, F32).reshape(-1, 4)], axis=0)
    matched = gt_pad[np.asarray(matches) + 2]
    iou = iou_elementwise_f32(anchors, matched)
    return np.where(np.asarray(matches) > -1, iou, F32(-1.0)).astype(F32)


def iou_loss_f64(preds, targets, normalizer, auxillary_loss_weight=1.0, grad_scale=1.0):
    """preds, targets [B, A] (every level, concatenated) -> (iou-prediction-loss, d(weight * grad_scale * loss)/dpreds),
    float64: sum over target > -1 of (pred - target)^2, divided by the normalizer"""
    p, t = np.asarray(preds, np.float64), np.asarray(targets, np.float64)
    w = (t > -1.0).astype(np.float64)
    loss = float((w * (p - t) ** 2).sum() / float(normalizer))
    grad = 2.0 * (p - t) * w * (float(auxillary_loss_weight) * float(grad_scale) / float(normalizer))
    return loss, grad
