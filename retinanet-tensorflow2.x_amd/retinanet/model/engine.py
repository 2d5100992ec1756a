"""Executors that turn the static layer graph into HIP launches.

`InferenceEngine` is the MI355X replacement of `model(images, training=False)` for the Keras
model the reference builds (retinanet/model/builder.py:94-106): weights are packed once to the
MFMA-friendly bf16 [Cout][R][S][Cin] layout, BatchNorm (inference mode: moving statistics) and
conv bias are applied in the conv epilogue together with the activation and the residual add (rounded to bf16
where the reference holds a bf16 tensor between two layers: rnet_hip.h, rn_conv_segment), all activations live in buffers allocated once, and the
launch list is fixed — so the whole forward pass can be captured in a HIP graph
(`capture_graph=True`) and replayed with one host call instead of ~70.
"""
from __future__ import annotations

import ctypes
import os

import torch

from retinanet import _C
from .bottleneck import Bottleneck64, fused_blocks
from .forward import (FoldedConvs, FusionState, conv_launch_name, conv_problem, dw_problem, fold_bn, maxpool_step, output_view,
                      padded_outputs, split_by_depth, stem_input, stem_pool_partner, stem_pool_step, stem_problem, tensor_readers, topdown_step)
from .forward import pixel_pair_kernel, pixel_pair_ok  # noqa: F401  (host-side helpers, importable from here as before)


class InferenceEngine:
    def __init__(self, graph, variables, batch_size, device, bn_epsilon=1e-3, capture_graph=False, f16=False,
                 launch_opts=None, quantization=None):
        self.g = graph
        self.B = int(batch_size)
        self.dev = torch.device(device)
        self.eps = float(bn_epsilon)
        self.f16 = bool(f16)   # `mixed_float16`: IEEE-half activations on librnet_hip_f16.so, else bfloat16
        self.h16 = torch.float16 if self.f16 else torch.bfloat16
        self._DT = {"bf16": self.h16, "f32": torch.float32}
        self.lib = _C.lib(self.f16)
        # rn_launch_opts of THIS engine's conv launches (kernel-family overrides for tests / A/B timing; the library has
        # no process-wide knobs)
        if isinstance(launch_opts, dict):
            launch_opts = _C.LaunchOpts(**launch_opts)
        self.launch_opts = launch_opts.copy() if launch_opts is not None else _C.LaunchOpts()
        self._keep = []     # ctypes structs / arrays that must outlive the launches
        self.dw_launches = []   # (name, rn_dw_problem) of every depthwise launch
        self.se_launches = []   # (name, N, HW, C, se) of every rn_squeeze_excite_inplace launch
        self.steps = []     # list of (callable, name)
        self.t = {}         # tensor name -> torch tensor
        self.readers = tensor_readers(self.g.ops)
        self._graph = None
        self._capture = bool(capture_graph)
        with torch.cuda.device(self.dev):
            self._alloc()
            # INT8 serving of the detection heads (retinanet/model/quantization.py): a QuantizationTable turns the
            # class-head / box-head convs into rn_quantize_i8 + rn_conv3x3_i8_fwd launches; backbone and FPN stay as they are
            self.int8 = None
            if quantization is not None:
                from .quantization import Int8Heads
                self.int8 = Int8Heads(self, quantization)
            # split-K of the persistent conv kernels' last round: the launches of this engine run in order on one stream
            self.splitk_ws = _C.new_splitk_workspace(self.lib, self.dev, default_on=True)
            self.folded = FoldedConvs(self.lib, self.g, self.B, self.dev, self.h16, self.launch_opts, self.splitk_ws,
                                      self.eps)
            self.load_variables(variables)
            # second stream (see _side_launch): its conv launches need a split-K workspace of their own — launches
            # that share one must be ordered on one stream
            # Measured (round 5, one box, tools/bench_infer.py): batch 8 3.554 -> 3.512 ms; batch 1 1.572 -> 1.594 ms — at
            # batch 1 a fork / join pair costs more than the ~15 us launch it takes off the chain, so the default is two
            # streams from batch 4 up.  RNET_INFER_STREAMS=1 / 2 forces either.
            ns = os.environ.get("RNET_INFER_STREAMS", "")
            self.two_streams = (ns == "2") if ns in ("1", "2") else self.B >= 4
            self.splitk_ws_side = (_C.new_splitk_workspace(self.lib, self.dev, default_on=True)
                                   if self.two_streams else None)
            self.side_steps = set()   # names of the launches that go to the second stream
            self.step_io = {}         # step name -> (tensor names read, tensor names written)
            self._build()
            self._side_stream = (_C.concurrent_stream(self.lib, self.dev, [torch.cuda.current_stream(self.dev)])[0]
                                 if self.side_steps else None)
            self._events = [torch.cuda.Event() for _ in range(2 * len(self.side_steps))]

    # ---- buffers ---------------------------------------------------------------------------
    def _alloc(self):
        # ResNet stage-1 bottleneck blocks as ONE launch each (rn_bottleneck64_fwd, retinanet/model/bottleneck.py): their
        # inner tensors are never written, so they get no buffer
        blocks = fused_blocks(self.lib, self.g, self.B, lambda blk: True)
        self._bneck_skip = {o["out"] for blk in blocks for o in blk["ops"]}     # outputs of fused ops
        inner = self._bneck_skip - {blk["name"] for blk in blocks}
        padded = padded_outputs(self.g)
        for name, (H, W, C, dt) in self.g.tensors.items():
            if name not in inner:
                self.t[name] = torch.empty((self.B, H, W, padded.get(name, C)), dtype=self._DT[dt], device=self.dev)
        self.bneck = {blk["ops"][0]["out"]: Bottleneck64(self.lib, self.g, blk, self.B, self.dev, self.launch_opts,
                                                         self.t[blk["x"]], self.t[blk["name"]]) for blk in blocks}
        stem = next(o for o in self.g.ops if o["op"] == "stem")
        self.stem_k, self.stem_pad, self.Hp, self.Wp, self.stem_in = stem_input(self.g.tensors, stem, self.B, self.h16,
                                                                                self.dev)
        se_ops = [o for o in self.g.ops if o["op"] == "se"]
        if se_ops:
            nbytes = max(self.lib.rn_se_workspace_bytes(self.B, self.g.ses[o["se"]]["C"]) for o in se_ops)
            self.se_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    # ---- weights -----------------------------------------------------------------------------
    def load_variables(self, variables):
        """(Re)pack conv kernels and refold BN/bias from a name -> tensor dict (in place after the first call)."""
        fc = self.folded
        for op in self.g.ops:
            if op["op"] == "se":
                fc.load_se(variables, op)
            elif op["op"] == "dwconv":
                fc.load_dw(variables, op)
            elif op["op"] == "conv" and self.int8 is not None and op["out"] in self.int8.outs:
                continue                                                              # int8 heads: packed below
            elif op["op"] in ("conv", "stem") and op["out"] not in self._bneck_skip:   # fused blocks: packed below
                fc.load(variables, op)
            elif op["op"] == "topdown" and op.get("fusion"):
                # f32, copied in place: the top-down launch (captured or not) reads them on the device
                for name in (n for pair in op["fusion_vars"] for n in pair):
                    fc.stable(name, variables[name].to(self.dev, torch.float32).reshape(-1).clone())
        for fb in self.bneck.values():
            fb.load(variables, self.eps)
        if self.int8 is not None:
            self.int8.load(variables)

    # ---- launch list -------------------------------------------------------------------------
    def _side_launch(self, ops, second_of_split):
        """Launches that leave the main stream.  At batch 1 (BASELINE configs[0]: the reference's latency protocol) every
        launch is a fraction of the chip wide and ~15 us of fixed latency long, so a launch that nothing on the critical
        path waits for can run BESIDE it on a second stream — in a captured graph a parallel branch:
          * the projection shortcut of a ResNet stage's first block (resnet.py:220-228): read again only as the `residual`
            of the block's last conv, three launches later;
          * a prediction conv whose outputs are network outputs, next to the other head's (detection_head.py:80-88);
          * the second launch of a grouped launch that split_by_depth cut in two.
        Results are what they were: every launch computes the same tiles from the same inputs.  RNET_INFER_STREAMS=1
        keeps one stream (A/B)."""
        if not self.two_streams:
            return False
        if second_of_split:
            return True
        outs_ = [o["out"] for o in ops]
        roles = [r for t in outs_ for _, r in self.readers.get(t, [])]
        if roles and all(r == "residual" for r in roles):
            return True
        net_outs = {n for d in self.g.outputs.values() for n in d.values()}
        if not roles and all(t in net_outs for t in outs_):
            # only when another launch follows that does not need it (the class head's prediction conv)
            later = [o for o in self.g.ops if o["op"] == "conv" and o["out"] in net_outs and o["out"] not in outs_]
            idx = {id(o): i for i, o in enumerate(self.g.ops)}
            return any(idx[id(o)] > max(idx[id(q)] for q in ops) for o in later)
        return False

    def _add_conv_launch(self, ops, second_of_split=False):
        side = self._side_launch(ops, second_of_split)
        p = conv_problem(self.g, ops, self.B, self.launch_opts, self.splitk_ws_side if side else self.splitk_ws,
                         lambda o: self.t[o["inp"]], lambda o: self.t[o["out"]], self.folded.pixel_pair)
        for i, op in enumerate(ops):
            self.folded.fill(p.seg[i], op, self.t)
        self._keep.append(p)
        lib = self.lib
        pref = ctypes.byref(p)
        self.conv_problems = getattr(self, "conv_problems", {})
        name = conv_launch_name("conv:", ops, self.conv_problems)
        self.conv_problems[name] = p   # for profilers: lib.rn_conv_tile_rows(byref(p))

        def run(st):
            _C.check(lib.rn_conv2d_nhwc_fwd(pref, st), f"rn_conv2d_nhwc_fwd[{name[5:]}]")
        self.steps.append((run, name))
        self.step_io[name] = ({t for o in ops for t in (o["inp"], o.get("residual")) if t}, {o["out"] for o in ops})
        if side:
            self.side_steps.add(name)

    def _add_step(self, fn, name, reads, writes, side=False):
        self.steps.append((fn, name))
        self.step_io[name] = (reads, writes)
        if side:
            self.side_steps.add(name)

    def _add_int8_launches(self, ops):
        """the grouped head launch `ops` on the int8 kernels: the quantiser in front of the first one, then one launch per
        10 segments"""
        q = self.int8
        if not q.launches:
            self._add_step(*q.quantize_step())
        n = _C.RN_CONV_MAX_SEGMENTS
        for j in range(0, len(ops), n):
            sub = ops[j:j + n]
            name = conv_launch_name("conv_i8:", sub, q.problems)
            fn, reads, writes = q.conv_step(sub, name)
            self._add_step(fn, name, reads, writes, side=self._side_launch(sub, j > 0))

    def _add_dw_launch(self, ops):
        p = dw_problem(self.g, ops, self.B, lambda o: self.t[o["inp"]], lambda o: self.t[o["out"]],
                       lambda o: self.folded.packed[o["dw"]].data_ptr(), _C.ACT_IDS[ops[0]["act"]])
        for i, op in enumerate(ops):
            self.folded.fill_dw(p.seg[i], op)
        self._keep.append(p)
        lib = self.lib
        pref = ctypes.byref(p)
        name = ops[0].get("group") or ops[0]["out"]
        self.dw_launches.append(("dwconv:" + name, p))

        def run(st):
            _C.check(lib.rn_depthwise_conv2d_nhwc_fwd(pref, st), f"rn_depthwise_conv2d_nhwc_fwd[{name}]")
        self.steps.append((run, "dwconv:" + name))
        self.step_io["dwconv:" + name] = ({o["inp"] for o in ops}, {o["out"] for o in ops})

    def _build(self):
        lib = self.lib
        B = self.B
        done_groups = set()
        fused_pools = set()   # MaxPool outputs written by the fused stem launch
        for op in self.g.ops:
            kind = op["op"]
            if kind == "stem":
                img = self.t["images"]
                H, W = img.shape[1], img.shape[2]
                pin, pimg = self.stem_in.data_ptr(), img.data_ptr()

                def pack(st, pimg=pimg, pin=pin, H=H, W=W, pt=self.stem_pad[0], pl=self.stem_pad[1]):
                    _C.check(lib.rn_pack_image_nhwc4(pimg, B, H, W, pt, pl, self.Hp, self.Wp, pin, st),
                             "rn_pack_image_nhwc4")
                self.steps.append((pack, "pack_stem_input"))
                self.step_io["pack_stem_input"] = ({"images"}, {":stem_in"})
                scale, shift, _ = self.folded.fold[op["out"]]
                p = stem_problem(self, self.t[op["out"]], self.g.convs[op["conv"]]["cout"],
                                 self.folded.packed[op["conv"]].data_ptr(), _C.ACT_IDS[op["act"]], scale.data_ptr(),
                                 shift.data_ptr())
                self._keep.append(p)
                pref = ctypes.byref(p)
                pool = stem_pool_partner(self.g, op, self.readers)
                if pool is not None:   # ResNet: stem + BatchNorm + relu + MaxPool in one launch, the stem output stays on chip
                    fused_pools.add(pool["out"])
                    self.steps.append((stem_pool_step(lib, p, pool, self.t[pool["out"]]), "conv:stem"))
                    self.step_io["conv:stem"] = ({":stem_in"}, {pool["out"]})
                    continue

                def stem(st, pref=pref):
                    _C.check(lib.rn_conv2d_nhwc_fwd(pref, st), "rn_conv2d_nhwc_fwd[stem]")
                self.steps.append((stem, "conv:stem"))
                self.step_io["conv:stem"] = ({":stem_in"}, {op["out"]})
            elif kind == "conv" and op["out"] in self._bneck_skip:
                fb = self.bneck.get(op["out"])
                if fb is not None:                 # the block's first op in graph order carries the launch
                    self.steps.append((fb.launch, fb.name))
                    self.step_io[fb.name] = ({fb.blk["x"]}, {fb.blk["name"]})
            elif kind == "conv" and self.int8 is not None and op["out"] in self.int8.outs:
                grp = op.get("group") or op["out"]
                if grp not in done_groups:
                    done_groups.add(grp)
                    self._add_int8_launches([o for o in self.g.ops if o["op"] == "conv" and (o.get("group") or o["out"]) == grp])
            elif kind == "conv":
                grp = op.get("group")
                if grp is None:
                    self._add_conv_launch([op])
                elif grp not in done_groups:
                    done_groups.add(grp)
                    for j, sub in enumerate(split_by_depth(self.g, [o for o in self.g.ops if o["op"] == "conv" and o.get("group") == grp])):
                        self._add_conv_launch(sub, second_of_split=j > 0)
            elif kind == "dwconv":
                grp = op.get("group")
                if grp is None:
                    self._add_dw_launch([op])
                elif grp not in done_groups:
                    done_groups.add(grp)
                    self._add_dw_launch([o for o in self.g.ops if o["op"] == "dwconv" and o.get("group") == grp])
            elif kind == "se":
                x = self.t[op["tensor"]]
                name, se = op["se"], self.g.ses[op["se"]]
                args = self.folded.se_args(op, x, B, self.se_ws)
                self.se_launches.append(("se:" + op["tensor"], B, x.shape[1] * x.shape[2], se["C"], se["se"]))

                def se_run(st, args=args, name=name):
                    _C.check(lib.rn_squeeze_excite_inplace(*args, st), f"rn_squeeze_excite_inplace[{name}]")
                self.steps.append((se_run, "se:" + op["tensor"]))
                self.step_io["se:" + op["tensor"]] = ({op["tensor"]}, {op["tensor"]})
            elif kind == "maxpool":
                if op["out"] in fused_pools:
                    continue
                self.steps.append((maxpool_step(lib, op, self.t, B), "maxpool:" + op["out"]))
                self.step_io["maxpool:" + op["out"]] = ({op["inp"]}, {op["out"]})
            elif kind == "topdown":
                fusion = None
                if op.get("fusion"):
                    fusion = FusionState(lib, op, self.t[op["ins"][0]].shape[3], self.dev,
                                         lambda n: self.folded.packed[n].data_ptr())
                self.steps.append((topdown_step(lib, op, self.t, B, self._keep, fusion), "fpn_topdown"))
                self.step_io["fpn_topdown"] = (set(op["ins"]), set(op["outs"]))
            elif kind == "balance":
                ts = [self.t[n] for n in op["tensors"]]
                pin = _C.ptr_array(ts)
                self._keep.append(pin)
                mid = op["mid"]
                scratch = torch.empty_like(ts[mid])
                self._keep.append(scratch)
                H0, W0, C = ts[0].shape[1], ts[0].shape[2], ts[0].shape[3]

                def bal(st, pin=pin, L=len(ts), mid=mid, H0=H0, W0=W0, C=C, sp=scratch.data_ptr()):
                    _C.check(lib.rn_balance_features(pin, pin, L, mid, B, H0, W0, C, sp, st),
                             "rn_balance_features")
                self.steps.append((bal, "balance_features"))
                self.step_io["balance_features"] = (set(op["tensors"]), set(op["tensors"]))
            else:
                raise ValueError(kind)
        self.outputs = {k: {lv: output_view(self.t[n], self.g.tensors[n][2]) for lv, n in d.items()}
                        for k, d in self.g.outputs.items()}

    # ---- run -----------------------------------------------------------------------------------
    def _launch_all(self):
        st = _C.current_stream()
        if not self.side_steps:
            for fn, _ in self.steps:
                fn(st)
            return
        # two streams (see _side_launch): a side launch is ordered behind everything the main stream has enqueued so far
        # (event fork), the main stream waits for it in front of the first launch that touches what it wrote (or
        # overwrites what it read), and at the end.  Under torch.cuda.graph the events become graph edges.
        main, side = torch.cuda.current_stream(), self._side_stream
        sst = ctypes.c_void_p(side.cuda_stream)
        pending, ne = [], 0
        for fn, name in self.steps:
            reads, writes = self.step_io.get(name, (None, None))
            if name in self.side_steps:
                fork, done = self._events[ne], self._events[ne + 1]
                ne += 2
                fork.record(main)
                side.wait_event(fork)
                fn(sst)
                done.record(side)
                pending.append((done, reads, writes))
                continue
            keep = []
            for done, r_s, w_s in pending:
                if reads is None or (w_s & (reads | writes)) or (r_s & writes):
                    main.wait_event(done)
                else:
                    keep.append((done, r_s, w_s))
            pending = keep
            fn(st)
        for done, _, _ in pending:
            main.wait_event(done)

    def __call__(self, images):
        """images f32[B,H,W,3] (already normalised) -> prediction dict of static output buffers."""
        if tuple(images.shape) != tuple(self.t["images"].shape):
            raise ValueError(f"expected images of shape {tuple(self.t['images'].shape)}, got {tuple(images.shape)}")
        with torch.cuda.device(self.dev):
            if images.data_ptr() != self.t["images"].data_ptr():
                self.t["images"].copy_(images, non_blocking=True)
            if self._capture:
                if self._graph is None:
                    self._launch_all()  # warm-up outside capture (lazy module loads, attribute sets)
                    torch.cuda.synchronize()
                    self._graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self._graph):
                        self._launch_all()
                self._graph.replay()
            else:
                self._launch_all()
        return self.outputs
