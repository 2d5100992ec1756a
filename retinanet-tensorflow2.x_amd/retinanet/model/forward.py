"""The inference form of the forward pass, built the same way by both engines: BatchNorm and conv bias folded into the
conv epilogue — every layer when serving (`InferenceEngine`), the frozen `resnet_initial` layers and the fused stage-1
bottleneck blocks in training (`TrainEngine`).  Weight packing and folding at stable addresses, the conv launch geometry
(pixel pairs, split planes, grouped launches), the stem, max-pool and FPN top-down steps, and the index of which ops read
which tensor live here, once."""
from __future__ import annotations

import ctypes
import os

import torch

from retinanet import _C


def padded_outputs(g):
    """{network output tensor: channels its buffer holds}: the conv kernels write f32 outputs four channels at a time
    (rn_conv2d_nhwc_fwd: Cout % 4 == 0), so a prediction map whose channel count is no multiple of 4 — the auxiliary
    head's num_anchors = 9 — lives in a buffer padded to the next one.  The packed weights and the bias carry zeros in
    the pad rows, the engines hand out the live channels as a view (`output_view`)."""
    out = {}
    for d in g.outputs.values():
        for name in d.values():
            C = g.tensors[name][2]
            if g.tensors[name][3] == "f32" and C % 4:
                out[name] = -(-C // 4) * 4
    return out


def output_view(t, C):
    """the first C channels of output buffer `t` (the buffer itself when it holds no pad channels)"""
    return t if t.shape[3] == C else t[..., :C]


def split_by_depth(g, ops):
    """A grouped forward launch whose segments differ in K depth by 2x or more (the FPN lateral 1x1 convs: 512 / 1024 /
    2048 input channels) as two launches, the deep segments first.  The persistent kernels hand every XCD a contiguous range
    of tiles, so in one launch a single XCD ends up with all 50 of the 64-step tiles and most of the 32-step ones (181 K
    steps per CU there against 87 on average: 229 us for 103 us of work at B = 32).  On their own the deep segments are
    one round of tiles; the rest is a homogeneous launch.  Forward launches without BatchNorm only (a group with live
    BatchNorm shares one statistics message); RNET_GROUP_SPLIT=0 keeps one launch (A/B)."""
    if len(ops) < 2 or os.environ.get("RNET_GROUP_SPLIT", "1") == "0":
        return [ops]
    depth = [g.convs[o["conv"]]["k"] ** 2 * g.convs[o["conv"]]["cin"] for o in ops]
    deep = [o for o, d in zip(ops, depth) if d >= 2 * min(depth)]
    rest = [o for o, d in zip(ops, depth) if d < 2 * min(depth)]
    return [deep, rest] if deep and rest else [ops]


def pixel_pair_kernel(w):
    """HWIO [3, 3, C, C] kernel of a 3x3 / stride-1 convolution -> the [3, 3, 2C, 2C] kernel of the SAME convolution over
    pixel pairs: two horizontally adjacent pixels of the NHWC tensor seen as one pixel of 2C channels ([N, H, W, C] and
    [N, H, W/2, 2C] are the same bytes).  Output pixel 2X + a (a = 0, 1), tap s reads input pixel 2X + a + s - 1 =
    2(X + S - 1) + b: pair column S = (a + s - 1) // 2 + 1, half b = (a + s - 1) % 2; every other entry is zero."""
    C = w.shape[2]
    out = torch.zeros((3, 3, 2 * C, 2 * C), dtype=w.dtype, device=w.device)
    for a in (0, 1):
        for s_ in (0, 1, 2):
            t = a + s_ - 1
            S, b = t // 2 + 1, t % 2
            out[:, S, b * C:(b + 1) * C, a * C:(a + 1) * C] = w[:, s_]
    return out


def pixel_pair_ok(lib, g, op, B, opts, splitk_ws=None):
    """Does conv `op` run in pixel-pair form?  The 64-channel 3x3 layers of ResNet stage 1 (resnet.py:236-239 at 160 x 160)
    fill half a 128-column tile of every MFMA kernel here; on the 128-row kernel, which stages the pixels once per tap,
    they ran at 2.9x their HBM time (round 4: 120 - 131 us against 43 at B = 32).  As a convolution over pixel pairs the
    layer is 128 -> 128 channels on half as many pixels — the shape the halo kernel's 512 x 128 tiles take: twice the MACs
    (half of the paired kernel is zeros), one staging of the pixels per channel chunk.  Same products in the same order
    per output, so the same values.  Only where that kernel takes the paired shape (rn_conv_kernel_id == 3: enough tiles)
    and the layer runs in inference form (frozen `resnet_initial` layers in training, every layer when serving)."""
    if op.get("op") != "conv":
        return False
    c = g.convs[op["conv"]]
    H, W, C, _ = g.tensors[op["inp"]]
    if (c["k"], c["stride"], op["pad"]) != (3, 1, 1) or c["cin"] != c["cout"] or c["cout"] > 64 or c["cin"] % 8 or W % 2:
        return False
    if op.get("group") is not None or op.get("residual") or op.get("out_dtype", "bf16") != "bf16" or C != c["cin"]:
        return False
    p = _C.attach_splitk_workspace(_C.ConvProblem(), splitk_ws)
    p.opts = opts
    p.R = p.S = 3
    p.stride_h = p.stride_w = p.pad_top = p.pad_left = 1
    p.act, p.out_dtype, p.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, 1
    s = p.seg[0]
    s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = B, H, W // 2, 2 * C, 2 * C, H, W // 2, 2 * C
    return lib.rn_conv_kernel_id(ctypes.byref(p)) == 3


def w_pair_ok(lib, g, cname, B, opts):
    """True when the f32 conv `cname` (one kernel shared by the pyramid levels of a grouped launch) is narrow enough that
    its two weight planes go along Cout (rn_conv_segment.w_pair): 36 box-regression channels fill 72 of the 128 columns
    of the halo kernel's 512 x 128 tiles; along Cin they were a 64-column tile of the 128-row kernel at 2 x the K depth."""
    c = g.convs[cname]
    if lib.rn_conv_cout_pad(c["cout"]) > 64:
        return False                                        # wide layers (class prediction) already run 256-row tiles
    ops = [o for o in g.ops if o["op"] == "conv" and o["conv"] == cname]
    groups = {o.get("group") for o in ops}
    if len(groups) != 1 or None in groups:
        return False
    tn = g.tensors
    shapes = [tn[o["inp"]][:2] + (tn[o["inp"]][2],) + tn[o["out"]][:2] for o in ops]
    cout = -(-c["cout"] // 4) * 4     # the channels the launch writes (padded_outputs)
    return _C.pair_form_kernel(lib, B, c["k"], c["stride"], ops[0]["pad"], c["cin"], cout, shapes, opts) > 0


def stem_pool_partner(g, stem_op, readers):
    """The MaxPool op that rn_stem_conv_bn_relu_pool can absorb: the ResNet stem (7x7/2, 64 channels, relu | relu6)
    whose only reader is a 3x3 / stride-2 pool with SAME pads (resnet.py:288-307); None otherwise (EfficientNet's
    3x3 swish stem has no pool).  readers: tensor_readers(g.ops)."""
    c = g.convs[stem_op["conv"]]
    if c["k"] != 7 or c["cout"] != 64 or stem_op.get("act") not in ("relu", "relu6"):
        return None
    users = readers.get(stem_op["out"], [])
    if len(users) != 1 or users[0][0]["op"] != "maxpool":
        return None
    pool = users[0][0]
    if pool["k"] != 3 or pool["stride"] != 2 or pool["pad_top"] not in (0, 1) or pool["pad_left"] not in (0, 1):
        return None
    return pool


def half_activations(params):
    """`mixed_float16` (BASELINE config 5): IEEE-half activations / packed weights on librnet_hip_f16.so; RNET_F16=0
    keeps bfloat16 storage under that policy"""
    return (str(getattr(getattr(params, "floatx", None), "precision", "")) == "mixed_float16"
            and os.environ.get("RNET_F16", "1") != "0")


def tensor_readers(ops):
    """tensor name -> [(op, role)] of every op that reads it, in op order; role = the op field that names the tensor"""
    readers = {}
    for o in ops:
        for role in ("inp", "residual", "tensor", "ins", "tensors"):
            v = o.get(role)
            for t in (v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(t, str):
                    readers.setdefault(t, []).append((o, role))
    return readers


def fold_bn(variables, bn, bias, eps, dev, repeat=1):
    """(scale, shift, bias) of a conv epilogue in inference form: BN = x*scale + shift with scale = gamma/sqrt(var+eps),
    shift = beta - mean*scale; the Conv2D layer's bias stays separate (it is added before the layer's output is rounded
    to bf16).  repeat=2: pixel-pair form, the per-channel vectors once per pixel of the pair."""
    f32 = lambda n: variables[bn + n].to(dev, torch.float32)
    scale = shift = None
    if bn:
        scale = f32("/gamma") / torch.sqrt(f32("/moving_variance") + eps)
        shift = f32("/beta") - f32("/moving_mean") * scale
    bias = None if bias is None else bias.to(dev, torch.float32)
    return tuple(None if t is None else t.repeat(repeat) if repeat > 1 else t.contiguous() for t in (scale, shift, bias))


class FoldedConvs:
    """Packed weights and folded BatchNorm / bias vectors of the convs that run in inference form (every conv when serving;
    the frozen `resnet_initial` layers in training).  The first load packs and folds; every later one (a reload of the
    model's variables, a restored checkpoint) copies in place: launch descriptors and captured graphs keep the addresses.
    Each op's weight form is decided once — stem, pixel pair, two planes along Cout (w_pair), split-bf16 planes or plain.
    `eligible(op)`: the engine's rule for a conv that may take the pixel-pair form."""

    def __init__(self, lib, g, B, dev, h16, opts, splitk_ws, eps, eligible=lambda op: True):
        self.lib, self.g, self.B, self.dev, self.h16, self.opts = lib, g, B, dev, h16, opts
        self.splitk_ws, self.eps, self.eligible = splitk_ws, eps, eligible
        self.packed = {}    # conv / depthwise / squeeze-excite weight name -> packed buffer
        self.fold = {}      # op output -> [scale, shift, bias]
        self._pp, self._wp = {}, {}

    def pixel_pair(self, op):
        """True when conv `op` runs in pixel-pair form (pixel_pair_ok): decided once per op"""
        if op["out"] not in self._pp:
            self._pp[op["out"]] = bool(self.eligible(op)) and pixel_pair_ok(self.lib, self.g, op, self.B, self.opts,
                                                                              self.splitk_ws)
        return self._pp[op["out"]]

    def w_pair(self, cname):
        """w_pair_ok, decided once per conv from the shapes of the grouped launch it runs in"""
        if cname not in self._wp:
            self._wp[cname] = w_pair_ok(self.lib, self.g, cname, self.B, self.opts)
        return self._wp[cname]

    def w_form(self, op):
        """(w_terms, w_pair) of conv `op`: split-bf16 planes of the dtype=float32 prediction convs, the narrow one's along
        Cout (rn_conv_segment); (1, False) elsewhere"""
        if op.get("out_dtype") != "f32" or op["op"] != "conv":
            return 1, False
        return (1, True) if self.w_pair(op["conv"]) else (_C.PRED_W_TERMS, False)

    def buffer(self, key, shape):
        buf = self.packed.get(key)
        if buf is None:
            buf = self.packed[key] = torch.empty(shape, dtype=self.h16, device=self.dev)
        return buf

    def stable(self, key, tensor):
        old = self.packed.get(key)
        if old is None:
            self.packed[key] = tensor.contiguous()
        else:
            old.copy_(tensor)

    def refold(self, key, new):
        old = self.fold.get(key)
        if old is None:
            self.fold[key] = list(new)
        else:
            for dst, src in zip(old, new):
                if src is not None:
                    dst.copy_(src)

    def load(self, variables, op):
        """(re)pack the kernel of conv / stem `op` and refold its BatchNorm and bias"""
        lib, st = self.lib, _C.current_stream()
        cname = op["conv"]
        c = self.g.convs[cname]
        k, cin, cout = c["k"], c["cin"], c["cout"]
        w = variables[c.get("kvar", cname + "/kernel")].to(self.dev, torch.float32).contiguous()
        cinp = lib.rn_conv_cin_pad(cin)
        terms, pair = self.w_form(op)
        repeat = 1
        if op["op"] == "stem":
            buf = self.buffer(cname, (lib.rn_conv_cout_pad(cout), k, 32))
            _C.check(lib.rn_pack_stem_weight_rs(_C.ptr(w), k, k, cout, _C.ptr(buf), st), "rn_pack_stem_weight_rs")
        elif self.pixel_pair(op):    # 64-channel 3x3 layer as a 128 -> 128 convolution over pixel pairs
            w2 = pixel_pair_kernel(w).contiguous()
            cinp2 = lib.rn_conv_cin_pad(2 * cin)
            buf = self.buffer(cname, (lib.rn_conv_cout_pad(2 * cout), 3, 3, cinp2))
            _C.check(lib.rn_pack_conv_weight(_C.ptr(w2), 3, 3, 2 * cin, 2 * cout, cinp2, _C.ptr(buf), st),
                     "rn_pack_conv_weight")
            repeat = 2
        elif pair:                   # narrow f32 layer (box prediction): the two planes along Cout
            buf = self.buffer(cname, (lib.rn_conv_pair_rows(cout), k, k, cinp))
            _C.check(lib.rn_pack_conv_weight_pair(_C.ptr(w), 0, k, k, cin, cout, cinp, _C.ptr(buf), st),
                     "rn_pack_conv_weight_pair")
        elif terms > 1:              # f32 layer (detection_head.py:80-88): its f32 kernel as split-bf16 planes
            buf = self.buffer(cname, (lib.rn_conv_cout_pad(cout), k, k, terms * cinp))
            _C.check(lib.rn_pack_conv_weight_split(_C.ptr(w), 0, k, k, cin, cout, cinp, terms, _C.ptr(buf), st),
                     "rn_pack_conv_weight_split")
        else:
            buf = self.buffer(cname, (lib.rn_conv_cout_pad(cout), k, k, cinp))
            _C.check(lib.rn_pack_conv_weight(_C.ptr(w), k, k, cin, cout, cinp, _C.ptr(buf), st), "rn_pack_conv_weight")
        fold = fold_bn(variables, op.get("bn"), variables.get(cname + "/bias"), self.eps, self.dev, repeat)
        if fold[2] is not None and op.get("out_dtype") == "f32" and fold[2].numel() % 4:   # padded_outputs: zero bias there
            fold = fold[:2] + (torch.nn.functional.pad(fold[2], (0, -fold[2].numel() % 4)),)
        self.refold(op["out"], fold)

    def load_dw(self, variables, op):
        """(re)pack the [k][k][C][1] kernel of depthwise op `op` to [k*k][C] and refold its BatchNorm"""
        d = self.g.dws[op["dw"]]
        w = variables[d["kvar"]].to(self.dev, torch.float32).contiguous()
        buf = self.buffer(op["dw"], (d["k"] * d["k"], d["C"]))
        _C.check(self.lib.rn_pack_depthwise_weight(_C.ptr(w), d["k"], d["C"], _C.ptr(buf), _C.current_stream()),
                 "rn_pack_depthwise_weight")
        self.refold(op["out"], fold_bn(variables, op.get("bn"), None, self.eps, self.dev))

    def load_se(self, variables, op):
        """the two 1x1 kernels ([out][in], storage type) and f32 biases of squeeze-excite op `op`, as
        rn_squeeze_excite_inplace reads them: `<se>:w1`, `:b1`, `:w2`, `:b2`"""
        name = op["se"]
        se = self.g.ses[name]
        f32 = lambda n: variables[name + n].to(self.dev, torch.float32)
        self.stable(name + ":w1", f32("/conv2d/kernel").reshape(se["C"], se["se"]).t().to(self.h16))
        self.stable(name + ":b1", f32("/conv2d/bias"))
        self.stable(name + ":w2", f32("/conv2d_1/kernel").reshape(se["se"], se["C"]).t().to(self.h16))
        self.stable(name + ":b2", f32("/conv2d_1/bias"))

    def se_args(self, op, x, B, ws):
        """arguments of rn_squeeze_excite_inplace for op `op` on tensor x (workspace ws), without the stream"""
        name, se, pk = op["se"], self.g.ses[op["se"]], self.packed
        return (x.data_ptr(), B, x.shape[1] * x.shape[2], se["C"], pk[name + ":w1"].data_ptr(), pk[name + ":b1"].data_ptr(),
                pk[name + ":w2"].data_ptr(), pk[name + ":b2"].data_ptr(), se["se"], ws.data_ptr(), ws.numel())

    def fill_dw(self, seg, op):
        """weights and inference-form epilogue (folded BatchNorm) of the segment of depthwise op `op`"""
        scale, shift, _ = self.fold[op["out"]]
        seg.w = self.packed[op["dw"]].data_ptr()
        seg.scale = scale.data_ptr() if scale is not None else None
        seg.shift = shift.data_ptr() if shift is not None else None

    def fill(self, seg, op, t):
        """weights and inference-form epilogue of the segment of conv `op`: folded scale / shift / bias, residual"""
        scale, shift, bias = self.fold[op["out"]]
        seg.w = self.packed[op["conv"]].data_ptr()
        seg.scale = scale.data_ptr() if scale is not None else None
        seg.shift = shift.data_ptr() if shift is not None else None
        seg.bias = bias.data_ptr() if bias is not None else None
        seg.residual = t[op["residual"]].data_ptr() if op.get("residual") else None
        terms, pair = self.w_form(op)
        seg.w_terms, seg.w_pair = terms, 1 if pair else 0


def conv_problem(g, ops, B, opts, splitk_ws, x_of, y_of, pair, act=None):
    """rn_conv_problem of one forward launch over `ops` (one op, or a group whose ops share k / stride / pad / act / output
    dtype): the launch geometry and every segment's x, y and shapes; `pair(op)`: the segment runs in pixel-pair form (the
    same bytes as [N, H, W/2, 2C]).  act: the launch's activation id, default the ops' own.  Weights and epilogue are the
    caller's (FoldedConvs.fill in inference form)."""
    first = ops[0]
    c0 = g.convs[first["conv"]]
    p = _C.attach_splitk_workspace(_C.ConvProblem(), splitk_ws)
    p.opts = opts
    p.R = p.S = c0["k"]
    p.stride_h = p.stride_w = c0["stride"]
    p.pad_top = p.pad_left = first["pad"]
    p.act = _C.ACT_IDS[first["act"]] if act is None else act
    p.out_dtype = _C.RN_DT_F32 if first["out_dtype"] == "f32" else _C.RN_DT_BF16
    p.num_segments = len(ops)
    for i, op in enumerate(ops):
        c = g.convs[op["conv"]]
        if (c["k"], c["stride"], op["pad"], op["act"], op["out_dtype"]) != \
                (c0["k"], c0["stride"], first["pad"], first["act"], first["out_dtype"]):
            raise ValueError(f"conv group {first.get('group')} mixes shapes")
        x, y = x_of(op), y_of(op)
        s = p.seg[i]
        s.x, s.y = x.data_ptr(), y.data_ptr()
        s.N, s.H, s.W, s.Cin, s.pix_stride = B, x.shape[1], x.shape[2], c["cin"], x.shape[3]
        s.Ho, s.Wo, s.Cout = y.shape[1], y.shape[2], y.shape[3]   # (= c["cout"], or padded_outputs' count)
        if pair(op):
            s.W, s.Wo, s.Cin, s.Cout, s.pix_stride = x.shape[2] // 2, y.shape[2] // 2, 2 * c["cin"], 2 * c["cout"], 2 * x.shape[3]
    return p


def dw_problem(g, ops, B, x_of, y_of, w_of, act):
    """rn_dw_problem of one depthwise launch over `ops` (one op, or a group whose ops share k / stride / pads / act):
    geometry, x / w / y of every segment; act: the launch's activation id.  The epilogue (scale / shift) is the caller's."""
    first = ops[0]
    d0 = g.dws[first["dw"]]
    p = _C.DwProblem()
    p.k, p.stride, p.pad_top, p.pad_left = d0["k"], d0["stride"], first["pad_top"], first["pad_left"]
    p.act, p.num_segments = act, len(ops)
    for i, op in enumerate(ops):
        d = g.dws[op["dw"]]
        if (d["k"], d["stride"], op["pad_top"], op["pad_left"], op["act"]) != \
                (d0["k"], d0["stride"], first["pad_top"], first["pad_left"], first["act"]):
            raise ValueError(f"depthwise group {first.get('group')} mixes shapes")
        x, y = x_of(op), y_of(op)
        s = p.seg[i]
        s.x, s.w, s.y = x.data_ptr(), w_of(op), y.data_ptr()
        s.N, s.H, s.W, s.C, s.Ho, s.Wo = B, x.shape[1], x.shape[2], d["C"], y.shape[1], y.shape[2]
    return p


def conv_launch_name(prefix, ops, taken):
    """`<prefix><group | output>`, `:rest` appended for the second launch of a group that split_by_depth cut in two"""
    name = prefix + (ops[0].get("group") or ops[0]["out"])
    return name + ":rest" if name in taken else name


def stem_input(tensors, stem_op, B, h16, dev):
    """(k, (pad_top, pad_left), Hp, Wp, buffer) of the first-layer conv's input: the image repacked to a zero-bordered
    half-precision NHWC4 buffer (rn_pack_image_nhwc4)"""
    Hs, Ws = tensors[stem_op["out"]][:2]
    k = stem_op.get("k", 7)
    pad = (stem_op.get("pad_top", 3), stem_op.get("pad_left", 3))
    H, W, _, _ = tensors["images"]
    Hp = max((Hs - 1) * 2 + k, H + pad[0])
    Wp = -(-max((Ws - 1) * 2 + 8, W + pad[1]) // 8) * 8
    return k, pad, Hp, Wp, torch.empty((B, Hp, Wp, 4), dtype=h16, device=dev)


def stem_problem(eng, y, cout, w_ptr, act, scale=None, shift=None):
    """rn_conv_problem of the first-layer conv of engine `eng` (its stem_in / Hp / Wp / stem_k): k row taps x 8 column
    taps x 4 channels over the NHWC4 image, stride 2, writing y"""
    p = _C.attach_splitk_workspace(_C.ConvProblem(), eng.splitk_ws)
    p.opts = eng.launch_opts
    p.R, p.S, p.stride_h, p.stride_w, p.pad_top, p.pad_left = eng.stem_k, 1, 2, 2, 0, 0
    p.act, p.out_dtype, p.num_segments = act, _C.RN_DT_BF16, 1
    s = p.seg[0]
    s.x, s.w, s.y = eng.stem_in.data_ptr(), w_ptr, y.data_ptr()
    s.scale, s.shift, s.residual = scale, shift, None
    s.N, s.H, s.W, s.Cin, s.pix_stride = eng.B, eng.Hp, eng.Wp, 32, 4
    s.Ho, s.Wo, s.Cout = y.shape[1], y.shape[2], cout
    return p


def stem_pool_step(lib, p, pool, z):
    """ResNet stem in inference form (stem_problem `p`: folded BatchNorm, relu) and the MaxPool op `pool` as one launch
    writing z: the stem output stays on chip"""
    s = p.seg[0]
    a = (s.x, s.w, s.scale, s.shift, z.data_ptr(), s.N, s.H, s.W, s.Ho, s.Wo, p.R, s.Cout, p.act, pool["k"],
         pool["stride"], pool["pad_top"], pool["pad_left"], z.shape[1], z.shape[2])
    return lambda st: _C.check(lib.rn_stem_conv_bn_relu_pool(*a, st), "rn_stem_conv_bn_relu_pool")


def maxpool_step(lib, op, t, B):
    x, y = t[op["inp"]], t[op["out"]]
    a = (x.data_ptr(), y.data_ptr(), B, x.shape[1], x.shape[2], x.shape[3], op["k"], op["stride"], op["pad_top"],
         op["pad_left"], y.shape[1], y.shape[2])
    return lambda st: _C.check(lib.rn_maxpool2d_nhwc(*a, st), "rn_maxpool2d_nhwc")


class FusionState:
    """Device side of a weighted top-down op (`op["fusion"]`: fast_attention | fast_channel_attention): per fusion the
    addresses of its two f32 variables (`addr_of(name)`: a buffer that stays where it is — the launches read the weights
    on the device, so a reload or an optimizer step shows in the next launch or graph replay) and the coefficient block
    rn_fpn_topdown_fused writes in front of its top-down launches, which the backward launches of the same step read."""

    def __init__(self, lib, op, C, dev, addr_of):
        self.mode = _C.FUSION_IDS[op["fusion"]]
        self.names = [tuple(pair) for pair in op["fusion_vars"]]
        self.coef = [torch.empty((lib.rn_fpn_fusion_coef_bytes(C),), dtype=torch.uint8, device=dev) for _ in self.names]
        self.w = [(addr_of(lo), addr_of(up)) for lo, up in self.names]
        self.arrays = (_C.ptr_array_of([w[0] for w in self.w]), _C.ptr_array_of([w[1] for w in self.w]),
                       _C.ptr_array(self.coef))


def topdown_step(lib, op, t, B, keep, fusion=None):
    """FPN top-down pass (upsample + fusion + activation over the levels); the pointer arrays go to `keep`.  `fusion`:
    the FusionState of an op with a weighted fusion mode."""
    ins, outs = [t[n] for n in op["ins"]], [t[n] for n in op["outs"]]
    pin, pout = _C.ptr_array(ins), _C.ptr_array(outs)
    keep += [pin, pout]
    if op.get("fusion"):
        keep.append(fusion)
        a = (pin, pout) + fusion.arrays + (len(ins), B, ins[0].shape[1], ins[0].shape[2], ins[0].shape[3],
                                            _C.ACT_IDS[op["act"]], fusion.mode)
        return lambda st: _C.check(lib.rn_fpn_topdown_fused(*a, st), "rn_fpn_topdown_fused")
    a = (pin, pout, len(ins), B, ins[0].shape[1], ins[0].shape[2], ins[0].shape[3], _C.ACT_IDS[op["act"]])
    return lambda st: _C.check(lib.rn_fpn_topdown(*a, st), "rn_fpn_topdown")
