"""The small graph of the restatement tests (test_join_ref_cpu.py, test_forward_ref_cpu.py): every kind of op and join on
tensors of a few thousand elements, and the engine-local form of its op list.  No GPU code."""


def _graph():
    from retinanet.model.graph import Graph
    g = Graph()
    g.tensor("x0", 16, 16, 8)

    def conv(out, inp, k, cout, stride=1, act=None, residual=None, group=None, pad=None, bn=True, out_dtype="bf16",
             name=None, bias=False):
        name = name or out + "_conv"
        if name not in g.convs:
            g.add_conv_layer(name, k, g.tensors[inp][2], cout, stride, bias=bias, init="variance_scaling")
        if bn:
            g.add_bn_layer(out + "_bn", cout)
        return g.conv(out, inp, name, out + "_bn" if bn else None, act=act, residual=residual, group=group,
                      out_dtype=out_dtype, pad=pad)
    # bottleneck with a projection shortcut (1x1 / 2), 3x3 / 2 inside
    conv("a_sc", "x0", 1, 16, stride=2, pad=0)
    conv("a_a", "x0", 1, 8, act="relu")
    conv("a_b", "a_a", 3, 8, stride=2, act="relu", pad=1)
    conv("a_out", "a_b", 1, 16, act="relu", residual="a_sc")
    # identity bottleneck; b_b's BatchNorm is frozen under its trainable conv
    conv("b_a", "a_out", 1, 8, act="relu")
    conv("b_b", "b_a", 3, 8, act="relu")
    conv("b_out", "b_b", 1, 16, act="relu", residual="a_out")
    # MBConv: expand, depthwise (SAME), squeeze-excite, project + drop_connect + skip
    conv("m_exp", "b_out", 1, 32, act="swish")
    g.add_dw_layer("m_dw_layer", 3, 32, 1, "variance_scaling")
    g.add_bn_layer("m_dw_bn", 32)
    g.dwconv("m_dw", "m_exp", "m_dw_layer", bn="m_dw_bn", act="swish")
    g.add_se_layer("m_se", 32, 8)
    g.ops.append(dict(op="se", tensor="m_dw", se="m_se"))
    conv("m_proj", "m_dw", 1, 16, residual="b_out")
    g.ops[-1]["survival"] = 0.9
    # pyramid: lateral conv, the top two levels by max-pooling, top-down, one out-conv per level
    conv("c6pre", "b_out", 1, 8)
    for lv, prev in ((1, "c6pre"), (2, "p_in1")):
        H = g.tensors[prev][0] // 2
        g.tensor(f"p_in{lv}", H, H, 8)
        g.ops.append(dict(op="maxpool", out=f"p_in{lv}", inp=prev, k=2, stride=2, pad_top=0, pad_left=0))
    conv("p_in0", "m_proj", 1, 8)
    g.tensor("p_td0", 8, 8, 8)
    g.tensor("p_td1", 4, 4, 8)
    g.ops.append(dict(op="topdown", ins=["p_in0", "p_in1", "p_in2"], outs=["p_td0", "p_td1", "p_in2"], act="relu"))
    for lv, src in enumerate(("p_td0", "p_td1", "p_in2")):
        conv(f"p_out{lv}", src, 3, 8, group="fpn_out")
    g.ops.append(dict(op="balance", tensors=["p_out0", "p_out1", "p_out2"], mid=1))
    for head in ("cls", "box"):      # both heads' prediction convs share one group: two launches, one label
        for lv in range(3):
            conv(f"{head}{lv}", f"p_out{lv}", 3, 4, group="pred", bn=False, out_dtype="f32", name=head + "_pred", bias=True)
    return g


def _local_ops(g):
    """TrainEngine._prepare_graph: squeeze-excite runs out of place, later readers are redirected to its output"""
    tensors, ops, alias = dict(g.tensors), [], {}
    for op in g.ops:
        o = dict(op)
        for key in ("inp", "residual"):
            if o.get(key) in alias:
                o[key] = alias[o[key]]
        if o["op"] == "se":
            t = o["tensor"]
            o["inp"], o["out"] = alias.get(t, t), t + ":se"
            tensors[o["out"]] = g.tensors[t]
            alias[t] = o["out"]
        ops.append(o)
    return tensors, ops
