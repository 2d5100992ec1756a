"""CPU: the auxiliary IoU head in the static graph (variables, outputs, launch groups, freeze / decay name patterns),
its builder, and known answers of the numpy references in tests/aux_ref.py."""
import numpy as np
import pytest

import aux_ref

HEAD = "auxillary-head"
LEVELS = (3, 4, 5, 6, 7)


def _params(size=128, aux=True, num_convs=2, filters=64):
    from retinanet.cfg import default_params
    p = default_params(input_size=size)
    p.architecture.auxillary_head.use_auxillary_head = aux
    p.architecture.auxillary_head.num_convs = num_convs
    p.architecture.auxillary_head.filters = filters
    return p


def _graphs(size=128, **kw):
    from retinanet.model.graph import build_retinanet_graph
    return build_retinanet_graph(_params(size, aux=False)), build_retinanet_graph(_params(size, aux=True), **kw)


def _expected_variables(bn_tag="batch_normalization", cin=256, filters=64, num_convs=2, na=9):
    """name -> (shape, init, value) in the order Keras creates them: every BatchNorm first (detection_head.py:68-74),
    then the shared convs, then the prediction conv"""
    want = {}
    for i in range(num_convs):
        for lv in LEVELS:
            bn = f"{HEAD}/{HEAD}-{i}-p{lv}-{bn_tag}"
            want[bn + "/gamma"] = ((filters,), "const", 1.0)
            want[bn + "/beta"] = ((filters,), "const", 0.0)
            want[bn + "/moving_mean"] = ((filters,), "const", 0.0)
            want[bn + "/moving_variance"] = ((filters,), "const", 1.0)
    for i in range(num_convs):
        c = f"{HEAD}/{HEAD}-{i}-conv2d"
        want[c + "/kernel"] = ((3, 3, cin if i == 0 else filters, filters), "normal_0.01", None)
        want[c + "/bias"] = ((filters,), "const", 0.0)
    c = f"{HEAD}/{HEAD}-prediction-conv2d"
    want[c + "/kernel"] = ((3, 3, filters if num_convs else cin, na), "normal_0.01", None)
    want[c + "/bias"] = ((na,), "const", 0.0)      # -log((1 - 0.5) / 0.5) = 0
    return want


def test_graph_inventory():
    g0, g = _graphs(128)
    new = [k for k in g.var_specs if k not in g0.var_specs]
    want = _expected_variables()
    assert new == list(want)
    for k, (shape, init, value) in want.items():
        spec = g.var_specs[k]
        assert tuple(spec["shape"]) == shape and spec["init"] == init, k
        if init == "const":
            assert spec["value"] == value, k
        assert spec.get("trainable", True) == (not k.endswith(("/moving_mean", "/moving_variance"))), k
    # outputs: one f32 map of num_anchors channels per level
    assert set(g.outputs) == {"class-predictions", "box-predictions", "iou-predictions"}
    assert sorted(g.outputs["iou-predictions"]) == [str(lv) for lv in LEVELS]
    for lv in LEVELS:
        assert list(g.tensors[g.outputs["iou-predictions"][str(lv)]]) == [128 // 2 ** lv, 128 // 2 ** lv, 9, "f32"]
    # everything that existed stays what it was: var specs (and their order), ops, launch groups, tensors, outputs
    assert [(k, g.var_specs[k]) for k in g0.var_specs] == list(g0.var_specs.items())
    assert list(g.var_specs)[:len(g0.var_specs)] == list(g0.var_specs)
    assert g.ops[:len(g0.ops)] == g0.ops
    assert [(k, g.tensors[k]) for k in g0.tensors] == list(g0.tensors.items())
    assert all(g.outputs[k] == g0.outputs[k] for k in g0.outputs)
    assert [(k, g.convs[k]) for k in g0.convs] == list(g0.convs.items())
    # the head's own launch groups, none shared with the other two heads
    groups0 = {o.get("group") for o in g0.ops}
    own = [o for o in g.ops[len(g0.ops):]]
    assert {o.get("group") for o in own} == {"aux_tower0", "aux_tower1", "pred_iou"}
    assert not ({o.get("group") for o in own} & groups0)
    assert all(o["out"].startswith(HEAD) for o in own) and len(own) == 3 * len(LEVELS)
    # it reads the same features as the other heads
    assert [o["inp"] for o in own if o["group"] == "aux_tower0"] == \
        [o["inp"] for o in g0.ops if o.get("group") == "tower0"][:len(LEVELS)]


def test_graph_reads_balanced_features_and_initial_values():
    import torch
    from retinanet.cfg import default_params
    from retinanet.model.graph import build_retinanet_graph, init_variables
    p = default_params(input_size=128, balanced=True)
    p.architecture.auxillary_head.use_auxillary_head = True
    p.architecture.auxillary_head.num_convs, p.architecture.auxillary_head.filters = 1, 64
    g = build_retinanet_graph(p)
    box = [o["inp"] for o in g.ops if o.get("group") == "tower0"][:5]
    assert [o["inp"] for o in g.ops if o.get("group") == "aux_tower0"] == box
    v = init_variables(g, seed=3)
    pred = f"{HEAD}/{HEAD}-prediction-conv2d"
    assert torch.equal(v[pred + "/bias"], torch.zeros(9))
    k = v[pred + "/kernel"]
    assert tuple(k.shape) == (3, 3, 64, 9) and 0.005 < float(k.std()) < 0.02     # RandomNormal(stddev=0.01)
    # the variables in front of the head draw the same values as without it
    p.architecture.auxillary_head.use_auxillary_head = False
    v0 = init_variables(build_retinanet_graph(p), seed=3)
    assert all(torch.equal(v[k], t) for k, t in v0.items())


def test_sync_batch_norm_and_separable_names():
    _, g = _graphs(128, sync_bn_names=True)
    want = _expected_variables("sync_batch_normalization")
    assert [k for k in g.var_specs if k.startswith(HEAD)] == list(want)
    from retinanet.model.graph import build_retinanet_graph
    p = _params(128)
    p.architecture.conv_2d.use_seperable_conv = True
    gs = build_retinanet_graph(p)
    names = [k for k in gs.var_specs if k.startswith(HEAD) and "normalization" not in k]
    assert names == [f"{HEAD}/{HEAD}-0-conv2d/depthwise_kernel", f"{HEAD}/{HEAD}-0-conv2d/pointwise_kernel",
                     f"{HEAD}/{HEAD}-0-conv2d/bias", f"{HEAD}/{HEAD}-1-conv2d/depthwise_kernel",
                     f"{HEAD}/{HEAD}-1-conv2d/pointwise_kernel", f"{HEAD}/{HEAD}-1-conv2d/bias",
                     f"{HEAD}/{HEAD}-prediction-conv2d/depthwise_kernel",
                     f"{HEAD}/{HEAD}-prediction-conv2d/pointwise_kernel", f"{HEAD}/{HEAD}-prediction-conv2d/bias"]
    assert tuple(gs.var_specs[f"{HEAD}/{HEAD}-prediction-conv2d/pointwise_kernel"]["shape"]) == (1, 1, 64, 9)
    assert tuple(gs.var_specs[f"{HEAD}/{HEAD}-0-conv2d/depthwise_kernel"]["shape"]) == (3, 3, 256, 1)


def test_pruned_graph_is_the_head_off_graph():
    """what `serving_default` runs: the launches of the same model built without the head"""
    from retinanet.model.graph import prune_auxillary_head
    g0, g = _graphs(128)
    gp = prune_auxillary_head(g)
    assert gp.ops == g0.ops and list(gp.tensors.items()) == list(g0.tensors.items())
    assert list(gp.var_specs.items()) == list(g0.var_specs.items()) and gp.outputs == g0.outputs
    assert list(gp.convs.items()) == list(g0.convs.items()) and list(gp.bns.items()) == list(g0.bns.items())
    assert prune_auxillary_head(g0) is g0


def test_name_patterns_select_the_reference_sets():
    """The reference's patterns as written (model/builder.py:19-30): `backbone`, `backbone-bn` and `resnet_initial`
    exclude fpn, box-head and class-head only, so they catch the auxiliary head; the `head` patterns name the two
    other heads, so they do not."""
    from retinanet.model import ModelBuilder
    rx = ModelBuilder.FREEZE_VARS_REGEX
    assert rx["backbone"].pattern == r"^(?!((fpn)|(box-head)|(class-head)))"
    assert rx["head"].pattern == r"^((box-head)|(class-head))(?!.*prediction)"
    _, g = _graphs(128)
    aux = [k for k in g.var_specs if k.startswith(HEAD)]
    bn = [k for k in aux if "batch_normalization" in k]
    assert len(aux) == 46 and len(bn) == 40
    hit = {name: [k for k in aux if r.search(k)] for name, r in rx.items()}
    assert hit["backbone"] == aux
    assert hit["backbone-bn"] == bn
    assert hit["bn"] == bn
    assert hit["resnet_initial"] == aux     # `...-conv2d/`, `...-batch_normalization/` end every layer name of the head
    assert hit["fpn"] == hit["fpn-bn"] == hit["head"] == hit["head-bn"] == []
    # weight decay (executor.py:301-327): every variable of a trainable layer whose last name part holds `kernel`
    decayed = [k for k in aux if "kernel" in k.rsplit("/", 1)[-1]]
    assert decayed == [f"{HEAD}/{HEAD}-0-conv2d/kernel", f"{HEAD}/{HEAD}-1-conv2d/kernel",
                       f"{HEAD}/{HEAD}-prediction-conv2d/kernel"]
    # sync-BN naming variant: the same sets
    _, gs = _graphs(128, sync_bn_names=True)
    auxs = [k for k in gs.var_specs if k.startswith(HEAD)]
    assert [k for k in auxs if rx["resnet_initial"].search(k)] == auxs
    assert [k for k in auxs if rx["backbone-bn"].search(k)] == [k for k in auxs if "sync_batch_normalization" in k]


def test_builder_refuses_missing_activation():
    from retinanet.model.head import build_auxillary_head
    with pytest.raises(ValueError, match="activation_fn"):
        build_auxillary_head(2, 64, 9, 3, 7, conv_2d_op_params={}, normalization_op_params={}, activation_fn=None)
    head = build_auxillary_head(2, 64, 9, 3, 7, conv_2d_op_params={}, normalization_op_params={}, activation_fn="relu")
    assert (head.name, head.num_convs, head.filters, head.output_filters, head.prediction_bias) == \
        (HEAD, 2, 64, 9, 0.0)


# ---- known answers of the references -----------------------------------------------------------------------------
def test_iou_known_answers():
    a = np.array([[10, 10, 4, 6], [10, 10, 4, 6], [10, 10, 4, 4], [0, 0, 2, 2]], np.float32)
    b = np.array([[10, 10, 4, 6], [20, 20, 4, 6], [12, 10, 4, 4], [1, 1, 2, 2]], np.float32)
    got = aux_ref.iou_elementwise_f32(a, b)
    assert got.dtype == np.float32
    assert got[0] == np.float32(1.0)                # identical
    assert got[1] == np.float32(0.0)                # disjoint
    # half overlap: 4 x 4 boxes shifted by 2 in x: intersection 2 x 4 = 8, union 16 + 16 - 8 = 24
    assert got[2] == np.float32(8.0) / np.float32(24.0)
    # quarter overlap: intersection 1, union 4 + 4 - 1
    assert got[3] == np.float32(1.0) / np.float32(7.0)
    assert np.array_equal(aux_ref.iou_pairwise_f32(a[:2], b[:3])[0], aux_ref.iou_elementwise_f32(a[[0, 0, 0]], b[:3]))


def test_iou_targets_known_answers():
    anchors = np.array([[10, 10, 4, 4], [12, 10, 4, 4], [50, 50, 4, 4], [30, 30, 8, 8]], np.float32)
    gt = np.array([[10, 10, 4, 4], [30, 30, 8, 8]], np.float32)
    matches = np.array([0, 0, -1, -2], np.int32)
    t = aux_ref.iou_targets_f32(anchors, gt, matches)
    assert t.dtype == np.float32
    assert t.tolist() == [1.0, float(np.float32(8.0) / np.float32(24.0)), -1.0, -1.0]
    # match -2 against a box the anchor equals: still -1 (the gathered row of _pad_labels is a zero box anyway)
    assert aux_ref.iou_targets_f32(anchors, gt, np.array([1, 1, 1, 1], np.int32))[3] == 1.0
    # no ground truth at all
    assert (aux_ref.iou_targets_f32(anchors, np.zeros([0, 4], np.float32), np.full([4], -1, np.int32)) == -1).all()


def test_matcher_known_answers():
    anchors = np.array([[10, 10, 4, 4], [12, 10, 4, 4], [50, 50, 4, 4], [31, 30, 8, 8], [100, 100, 2, 2]], np.float32)
    gt = np.array([[10, 10, 4, 4], [30, 30, 8, 8], [90, 90, 2, 2]], np.float32)
    m = aux_ref.match_anchor_boxes(anchors, gt, match_iou=0.5, ignore_iou=0.3)
    # anchor 1 overlaps gt 0 by 1/3 -> ignored; anchor 3 overlaps gt 1 by 56 / 72 -> matched; gt 2 touches no anchor:
    # its first-maximum anchor is anchor 0 (all zeros), forced over the IoU match, the lowest GT index winning ties
    assert m.tolist() == [0, -2, -1, 1, -1]
    assert aux_ref.match_anchor_boxes(anchors, np.zeros([0, 4], np.float32), 0.5, 0.4).tolist() == [-1] * 5


def test_iou_loss_reference():
    p = np.array([[0.5, 2.0, -1.0, 0.25]])
    t = np.array([[1.0, -1.0, -1.0, 0.0]])
    loss, grad = aux_ref.iou_loss_f64(p, t, normalizer=2.0, auxillary_loss_weight=3.0, grad_scale=0.5)
    assert loss == pytest.approx((0.25 + 0.0625) / 2.0, abs=0, rel=1e-15)
    assert grad.tolist() == [[2 * -0.5 * 0.75, 0.0, 0.0, 2 * 0.25 * 0.75]]
