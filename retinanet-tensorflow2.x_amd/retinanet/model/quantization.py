"""INT8 serving of the detection heads (`export --precision int8`, DESIGN.md "INT8 serving").

The reference's deployment path ends in a calibrated INT8 TensorRT engine (export.py:79-104, 305-344).  Here the two
shared heads — more than half of the model's arithmetic — run on `rn_conv3x3_i8_fwd` (csrc/rn_conv_i8.hip):

  * `QuantizationTable`: one symmetric per-tensor scale for every head input and tower output, per pyramid level, under
    the graph's tensor names; what `<mode>/quantization.json` holds.
  * `Calibrator`: runs the bf16 / f16 `InferenceEngine` on calibration batches and reads those tensors from its static
    buffers — `minmax` (s = max|x| / 127) or `entropy` (2048-bin histogram of |x|, TensorRT-style KL threshold search).
  * `Int8Heads`: the launches an `InferenceEngine(..., quantization=table)` runs instead of the heads' bf16 convs.

Numerics contract of a quantised conv (include/rnet_hip.h): int32 accumulation, then the separately rounded fp32 steps
t = acc * mul[c]; t += add[c]; t = act(t); int8 output clamp(rint(t / s_out), -127, 127) or the f32 value itself, with
  mul = s_in * w_scale[c] * bn_scale[c],   add = bias[c] * bn_scale[c] + bn_shift[c]
folded in float64 and rounded once to f32 (`fold_epilogue`)."""
from __future__ import annotations

import ctypes
import glob
import json
import os

import numpy as np
import torch

from retinanet import _C

FORMAT = "retinanet-mi355x-quantization"
FORMAT_VERSION = 1
BINS = _C.RN_CALIB_BINS
LEVELS = 128
HEADS = ("class-head", "box-head")
METHODS = ("entropy", "minmax")


# ---- which ops are quantised, and which configs are refused ------------------------------------------------------------
def _own(name):
    return any(name.startswith(h + "_") for h in HEADS)


def head_plan(graph):
    """The conv ops of `class-head/*` and `box-head/*` in graph order, or NotImplementedError naming what this mode does
    not serve: separable heads, swish, head widths that are no multiple of 64 (or beyond the int32 accumulator bound)."""
    if any(o["op"] == "dwconv" and _own(o["out"]) for o in graph.ops):
        raise NotImplementedError("int8 serving: separable detection heads (use_seperable_conv, the EfficientNet configs) "
                                  "are not quantised")
    ops = [o for o in graph.ops if o["op"] == "conv" and _own(o["out"])]
    if not ops:
        raise NotImplementedError("int8 serving: the graph has no class-head / box-head convs")
    for o in ops:
        c = graph.convs[o["conv"]]
        if o["act"] not in (None, "none", "relu", "relu6"):
            raise NotImplementedError(f"int8 serving: activation {o['act']!r} of {o['out']} (none, relu and relu6 only; "
                                      "swish has no int8 form here)")
        if (c["k"], c["stride"], o["pad"]) != (3, 1, 1) or o.get("residual"):
            raise NotImplementedError(f"int8 serving: {o['out']} is not a plain 3x3 / stride 1 convolution")
        if c["cin"] % 64 or not 64 <= c["cin"] <= 512:
            raise NotImplementedError(f"int8 serving: {o['out']} has {c['cin']} input channels; head filters must be a "
                                      "multiple of 64 in [64, 512]")
        if o["out_dtype"] == "f32" and c["cout"] % 4:
            raise NotImplementedError(f"int8 serving: {o['out']} has {c['cout']} prediction channels; a multiple of 4 is needed")
    return ops


def calibrated_tensors(graph):
    """names of the tensors that carry a scale: every head conv's input (the FPN outputs and the tower outputs)"""
    names = []
    for o in head_plan(graph):
        if o["inp"] not in names:
            names.append(o["inp"])
    return names


# ---- the table ---------------------------------------------------------------------------------------------------------
class QuantizationTable:
    def __init__(self, scales, method, num_images):
        if method not in METHODS:
            raise ValueError(f"calibration method {method!r}: one of {METHODS}")
        self.scales = {str(k): float(v) for k, v in scales.items()}
        bad = [k for k, v in self.scales.items() if not (np.isfinite(v) and v > 0)]
        if bad:
            raise ValueError(f"scales must be finite and positive: {bad[:3]}")
        self.method, self.num_images = method, int(num_images)

    @property
    def key(self):
        return (self.method, self.num_images, tuple(sorted(self.scales.items())))

    def to_json(self):
        return {"format": FORMAT, "version": FORMAT_VERSION, "method": self.method, "num_images": self.num_images,
                "scales": dict(self.scales)}

    @classmethod
    def from_json(cls, d):
        if d.get("format") != FORMAT or d.get("version") != FORMAT_VERSION:
            raise ValueError(f"not a quantization table of format {FORMAT} version {FORMAT_VERSION}")
        return cls(d["scales"], d["method"], d["num_images"])

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_json(), f, indent=2)   # repr of a float round-trips exactly

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_json(json.load(f))


# ---- scales from statistics (host, float64) ------------------------------------------------------------------------------
def minmax_scale(amax):
    return float(amax) / 127.0 if amax > 0 else 1.0


def kl_threshold_bin(hist):
    """TensorRT-style entropy calibration over a histogram of |x|: the number of bins i in 128 .. len(hist) whose clipped
    distribution loses the least information.  Reference distribution: hist[:i] with the clipped tail folded into its last
    bin.  Candidate: hist[:i] merged into 128 groups (group j = bins [j*i // 128, (j+1)*i // 128)) and spread back evenly
    over the non-zero bins of each group, zeros preserved.  Returns the first i of minimal KL(reference || candidate)."""
    h = np.asarray(hist, dtype=np.float64)
    n = h.size
    csum = np.concatenate([[0.0], np.cumsum(h)])              # counts: exact in float64
    cnz = np.concatenate([[0], np.cumsum(h > 0)])
    total = csum[-1]
    best, best_i = None, None
    steps = np.arange(LEVELS + 1)
    for i in range(LEVELS, n + 1):
        ref = h[:i].copy()
        ref[i - 1] += total - csum[i]
        rs = ref.sum()
        if rs <= 0:
            continue
        b = (steps * i) // LEVELS
        gs, gn = csum[b[1:]] - csum[b[:-1]], cnz[b[1:]] - cnz[b[:-1]]
        val = np.divide(gs, gn, out=np.zeros(LEVELS), where=gn > 0)
        cand = np.repeat(val, np.diff(b)) * (h[:i] > 0)
        cs = cand.sum()
        if cs <= 0:
            continue
        p, q = ref / rs, cand / cs
        m = p > 0
        if (q[m] <= 0).any():
            continue                                           # infinite divergence
        d = float(np.sum(p[m] * np.log(p[m] / q[m])))
        if best is None or d < best:
            best, best_i = d, i
    return n if best_i is None else best_i


def entropy_scale(hist, amax):
    if not amax > 0:
        return 1.0
    return float(np.float64(kl_threshold_bin(hist)) * (np.float64(amax) / len(hist)) / 127.0)


def fold_epilogue(s_in, w_scale, bias, bn, eps):
    """(mul, add) f32 of one quantised conv at one level.  bn: None or (gamma, beta, moving_mean, moving_variance)."""
    ws = np.asarray(w_scale, dtype=np.float64)
    b = np.zeros_like(ws) if bias is None else np.asarray(bias, dtype=np.float64)
    if bn is None:
        scale, shift = np.ones_like(ws), np.zeros_like(ws)
    else:
        gamma, beta, mean, var = (np.asarray(v, dtype=np.float64) for v in bn)
        scale = gamma / np.sqrt(var + np.float64(eps))
        shift = beta - mean * scale
    return (np.float64(s_in) * ws * scale).astype(np.float32), (b * scale + shift).astype(np.float32)


# ---- calibration ---------------------------------------------------------------------------------------------------------
class Calibrator:
    """Per-tensor scales of the head inputs and tower outputs of a bf16 / f16 `InferenceEngine` from calibration batches.

        table = Calibrator(model.inference_engine(batch_size, serving=True), "entropy").run(batches)

    `batches`: a list of f32 [B,H,W,3] image tensors (already normalised), or a callable returning a fresh iterator of
    them — `entropy` walks them twice (max |x| first, then the histogram over [0, max])."""

    def __init__(self, engine, method="entropy"):
        if method not in METHODS:
            raise ValueError(f"calibration method {method!r}: one of {METHODS}")
        if engine.int8 is not None:
            raise ValueError("calibration reads the 16-bit engine's tensors, not an int8 engine's")
        self.method, self.eng = method, engine
        self.names = calibrated_tensors(self.eng.g)
        dev = self.eng.dev
        self.amax = torch.zeros(len(self.names), dtype=torch.float32, device=dev)
        self.hist = torch.zeros((len(self.names), BINS), dtype=torch.int64, device=dev)
        self.num_images = 0

    def _walk(self, batches, ranges=None):
        eng, lib = self.eng, self.eng.lib
        count = 0
        for images in (batches() if callable(batches) else batches):
            eng(images.to(eng.dev))
            count += int(images.shape[0])
            st = _C.current_stream()
            for i, name in enumerate(self.names):
                t = eng.t[name]
                C = eng.g.tensors[name][2]
                pixels = t.shape[0] * t.shape[1] * t.shape[2]
                if ranges is None:
                    _C.check(lib.rn_calib_absmax(_C.ptr(t), pixels, C, t.shape[3], _C.ptr(self.amax[i:]), st), "rn_calib_absmax")
                elif ranges[i] > 0:
                    _C.check(lib.rn_calib_histogram(_C.ptr(t), pixels, C, t.shape[3], float(ranges[i]), _C.ptr(self.hist[i]), st),
                             "rn_calib_histogram")
        if count == 0:
            raise ValueError("calibration needs at least one batch of images")
        return count

    def run(self, batches, num_images=None):
        with torch.cuda.device(self.eng.dev):
            n = self._walk(batches)
            amax = self.amax.cpu().numpy()
            if self.method == "minmax":
                scales = {name: minmax_scale(a) for name, a in zip(self.names, amax)}
            else:
                self._walk(batches, ranges=amax)
                hist = self.hist.cpu().numpy()
                scales = {name: entropy_scale(hist[i], amax[i]) for i, name in enumerate(self.names)}
        self.num_images = n if num_images is None else int(num_images)
        return QuantizationTable(scales, self.method, self.num_images)


def list_calibration_images(images_dir, num_images):
    files = sorted(f for pat in ("*.jpg", "*.jpeg", "*.png") for f in glob.glob(os.path.join(images_dir, pat)))
    files = files[:max(int(num_images), 0)]
    if not files:
        raise ValueError(f"no calibration images (*.jpg, *.jpeg, *.png) in {images_dir!r}")
    return files


def calibration_batches(files, params, batch_size, device):
    """callable -> iterator of f32 [batch_size,H,W,3] batches of `files`, decoded and prepared like `prepare_image`
    (normalise, aspect-preserving resize, zero pad); a short last batch is padded by repeating its last image"""
    from retinanet.dataloader.preprocessing_pipeline import PreprocessingPipeline
    from retinanet.dataloader.tfrecord_parser import decode_image
    pre = PreprocessingPipeline(params.input.input_shape, params.dataloader_params)
    B = int(batch_size)

    def batches():
        with torch.cuda.device(device):
            for i in range(0, len(files), B):
                imgs = []
                for path in files[i:i + B]:
                    with open(path, "rb") as f:
                        raw = decode_image(f.read())
                    imgs.append(pre.normalize_and_resize_with_pad(torch.from_numpy(raw).to(device))["image"])
                imgs += [imgs[-1]] * (B - len(imgs))
                yield torch.stack(imgs)
    return batches


def calibrate_from_directory(model, params, images_dir, num_images, batch_size, method):
    files = list_calibration_images(images_dir, num_images)
    cal = Calibrator(model.inference_engine(int(batch_size), serving=True), method)
    return cal.run(calibration_batches(files, params, batch_size, model.device), num_images=len(files))


# ---- the engine's INT8 launches --------------------------------------------------------------------------------------------
class Int8Heads:
    """The head launches of an `InferenceEngine` built with a quantisation table: one `rn_quantize_i8` launch over the
    FPN outputs (shared by both heads), one `rn_conv3x3_i8_fwd` launch per grouped head launch (`tower{i}`: both heads,
    all levels; `pred_class`, `pred_box`: f32 into the engine's output buffers).  Buffers, packed weights and the mul / add
    vectors are allocated once; `load` repacks and refolds in place, so captured graphs keep their addresses."""

    def __init__(self, eng, table):
        g = eng.g
        self.eng, self.table = eng, table
        self.ops = head_plan(g)
        self.outs = {o["out"] for o in self.ops}
        self.names = calibrated_tensors(g)
        missing = [n for n in self.names if n not in table.scales]
        if missing:
            raise ValueError(f"quantization table has no scale for {missing[:3]} ({len(missing)} tensors)")
        self.sources = [n for n in self.names if n not in self.outs]       # the FPN outputs: quantised by one launch
        self.launches = []   # (step name, ops) of every rn_conv3x3_i8_fwd launch, in launch order
        self.problems = {}
        self.packed, self.w_scale, self.mul, self.add = {}, {}, {}, {}
        dev = eng.dev
        for n in self.names:
            H, W, C, _ = g.tensors[n]
            buf = torch.empty((eng.B, H, W, C), dtype=torch.int8, device=dev)
            if n in self.outs:
                eng.t[n] = buf             # a tower output exists in int8 only
            else:
                eng.t[n + ":i8"] = buf
        for o in self.ops:
            c = g.convs[o["conv"]]
            if o["conv"] not in self.packed:
                nbytes = eng.lib.rn_conv_i8_weight_bytes(c["cin"], c["cout"])
                self.packed[o["conv"]] = torch.empty((nbytes,), dtype=torch.int8, device=dev)
                self.w_scale[o["conv"]] = torch.empty((c["cout"],), dtype=torch.float32, device=dev)
            self.mul[o["out"]] = torch.empty((c["cout"],), dtype=torch.float32, device=dev)
            self.add[o["out"]] = torch.empty((c["cout"],), dtype=torch.float32, device=dev)

    def x_name(self, op):
        return op["inp"] if op["inp"] in self.outs else op["inp"] + ":i8"

    def load(self, variables):
        """(re)pack the head kernels to int8 and refold every level's mul / add, in place"""
        eng, g = self.eng, self.eng.g
        st = _C.current_stream()
        host = lambda n: variables[n].detach().to(torch.float32).cpu().numpy()
        ws = {}
        for cname in self.packed:
            c = g.convs[cname]
            w = variables[c.get("kvar", cname + "/kernel")].to(eng.dev, torch.float32).contiguous()
            _C.check(eng.lib.rn_pack_conv_weight_i8(_C.ptr(w), 0, c["cin"], c["cout"], _C.ptr(self.packed[cname]),
                                                    _C.ptr(self.w_scale[cname]), st), "rn_pack_conv_weight_i8")
            ws[cname] = self.w_scale[cname].cpu().numpy()
        for o in self.ops:
            cname, bn = o["conv"], o.get("bn")
            bias = host(cname + "/bias") if (cname + "/bias") in variables else None
            stats = None if not bn else tuple(host(bn + s) for s in ("/gamma", "/beta", "/moving_mean", "/moving_variance"))
            mul, add = fold_epilogue(self.table.scales[o["inp"]], ws[cname], bias, stats, eng.eps)
            self.mul[o["out"]].copy_(torch.from_numpy(mul))
            self.add[o["out"]].copy_(torch.from_numpy(add))

    def quantize_step(self):
        eng = self.eng
        p = _C.QuantProblem()
        if len(self.sources) > _C.RN_CONV_MAX_SEGMENTS:
            raise NotImplementedError("int8 serving: more than 10 pyramid levels")
        p.num_segments = len(self.sources)
        for i, n in enumerate(self.sources):
            x, y = eng.t[n], eng.t[n + ":i8"]
            s = p.seg[i]
            s.x, s.y, s.pixels = x.data_ptr(), y.data_ptr(), x.shape[0] * x.shape[1] * x.shape[2]
            s.C, s.pix_stride, s.inv_scale = y.shape[3], x.shape[3], float(np.float32(1.0) / np.float32(self.table.scales[n]))
        eng._keep.append(p)
        pref, lib = ctypes.byref(p), eng.lib
        reads, writes = set(self.sources), {n + ":i8" for n in self.sources}
        return (lambda st: _C.check(lib.rn_quantize_i8(pref, st), "rn_quantize_i8")), "quantize_i8:heads", reads, writes

    def conv_step(self, ops, name):
        eng = self.eng
        first = ops[0]
        p = _C.ConvI8Problem()
        p.act = _C.ACT_IDS[first["act"]]
        p.out_dtype = _C.RN_DT_F32 if first["out_dtype"] == "f32" else _C.RN_DT_I8
        p.num_segments = len(ops)
        for i, o in enumerate(ops):
            if (o["act"], o["out_dtype"]) != (first["act"], first["out_dtype"]):
                raise ValueError(f"conv group {first.get('group')} mixes activations / output types")
            x, y = eng.t[self.x_name(o)], eng.t[o["out"]]
            s = p.seg[i]
            s.x, s.w, s.y = x.data_ptr(), self.packed[o["conv"]].data_ptr(), y.data_ptr()
            s.mul, s.add = self.mul[o["out"]].data_ptr(), self.add[o["out"]].data_ptr()
            s.out_inv_scale = float(np.float32(1.0) / np.float32(self.table.scales[o["out"]])) if p.out_dtype == _C.RN_DT_I8 else 1.0
            s.N, s.H, s.W, s.Cin, s.Cout = eng.B, x.shape[1], x.shape[2], x.shape[3], y.shape[3]
        eng._keep.append(p)
        self.launches.append((name, list(ops)))
        self.problems[name] = p
        pref, lib = ctypes.byref(p), eng.lib
        reads, writes = {self.x_name(o) for o in ops}, {o["out"] for o in ops}
        return (lambda st: _C.check(lib.rn_conv3x3_i8_fwd(pref, st), f"rn_conv3x3_i8_fwd[{name}]")), reads, writes
