"""TrainEngine — the MI355X replacement of Executor._train_step (retinanet/executor.py:409-441).

One call = forward (training-mode BatchNorm) -> RetinaNetLoss forward+backward -> backward
through heads / BalanceFeatures / FPN / ResNet -> weight decay + per-tensor and global clipping
-> data-parallel all-reduce (RCCL) -> SGD momentum + EMA, all as HIP launches on static buffers.

There is no autograd tape: the backward pass is the closed-form gradient of every layer,
scheduled from the same static graph as the forward pass.
  * conv backward = wgrad (transpose-read MFMA kernel, deterministic split-K) + dgrad (the
    forward implicit-GEMM kernel run on dy with flipped/transposed weights; stride-2 layers go
    through a zero-insertion upsample), gradients of multi-consumer tensors are accumulated in
    the dgrad epilogue (residual add in place);
  * BatchNorm forward/backward are two-stage reductions; with `use_sync` and >1 rank the
    per-group [sum, sumsq] / [sum g, sum g*xhat] vectors are all-reduced between the stages
    (SyncBatchNormalization, model/utils.py:10-12);
  * layers frozen whole (training.freeze_variables, executor.py:154-176) keep inference-mode BN folded
    into their conv / depthwise epilogue and get no backward at all while nothing below them trains; above trainable
    layers (`fpn`, `head`) they run like the next form without weight, bias, gamma or beta gradients, their
    data-gradient weight packs made once when weights are loaded; a frozen BatchNorm under a trainable conv
    (the `bn` / `*-bn` keys) runs in inference mode inside the step: the raw conv launch, rn_bn_apply
    with a constant scale / shift table, and one elementwise rn_bn_frozen_bwd in the backward pass —
    no statistics, no reductions, no gamma / beta gradients, no SyncBN message;
  * parameters, gradients, momentum and EMA live in four flat fp32 arenas (conv kernels in the
    compute layout [Cout][R][S][Cin]); the optimizer is three multi-tensor launches and also
    refreshes the bf16 compute copy of every kernel.
The stem trains too (configs without `freeze_variables`): its weight gradient runs the same wgrad
kernel on the packed NHWC4 image (7 row taps x 32 = 8 column taps x 4 channels), the 3x3/2 SAME
max-pool has a gather-form backward.
"""
from __future__ import annotations

import ctypes
import functools
import os
from typing import NamedTuple

import numpy as np
import torch

from retinanet import _C
from .bottleneck import Bottleneck64, fused_blocks
from .data_parallel import GradientOverlap, SmallMessages
from .forward import (FoldedConvs, FusionState, conv_launch_name, conv_problem, dw_problem, fold_bn, half_activations, maxpool_step,
                      output_view, padded_outputs, split_by_depth, stem_input, stem_pool_partner, stem_pool_step, stem_problem, tensor_readers,
                      topdown_step)

_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
_SEG_DTYPE = np.dtype([("offset", "<i8"), ("size", "<i8"), ("wd", "<i4"), ("bb", "<i4"), ("nb", "<i4"),
                       ("pad", "<i4"), ("bf", "<i8")])


def _hwio_to_ohwi(w):
    return w.permute(3, 0, 1, 2).contiguous()


def _ohwi_to_hwio(w):
    return w.permute(1, 2, 3, 0).contiguous()


class BnGroup(NamedTuple):
    """The training-mode BatchNorm of one launch (TrainEngine.bn_groups, keyed by the first op's output)"""
    problem: _C.BnProblem
    sums: torch.Tensor     # [sum | sumsq] of every segment + the slot C2 rides in (the SyncBN forward message)
    bsums: torch.Tensor    # [sum g | sum g*xhat] of every segment (the SyncBN backward message)
    ws: torch.Tensor       # workspace of the two-stage reductions (partial sums, ticket counters)
    dys: list              # per op: gradient at the conv output, written by rn_bn_bwd_apply / rn_bn_frozen_bwd
    ops: list
    fwd: torch.Tensor = None   # [mean | invstd | scale | shift] of every segment
    frozen: bool = False   # BatchNorm in inference mode under a trainable conv: fwd holds the folded moving statistics


class BackwardStep:
    """One entry of TrainEngine.bwd_steps.  run(stream) enqueues it; side: only the optimizer reads its results (weight /
    bias gradients), so the two-stream backward runs it on the weight-gradient stream; writes: the variables whose
    gradient it completes (bucket readiness of the overlapped all-reduce); wgrad: (problem, dw, workspace, FLOPs) of a
    weight-gradient launch that _group_wgrad_steps may merge with same-shape layers."""
    __slots__ = ("run", "side", "writes", "wgrad")

    def __init__(self, run, side=False, writes=(), wgrad=None):
        self.run, self.side, self.writes, self.wgrad = run, side, writes, wgrad

    def __call__(self, st):
        return self.run(st)


class GradientJoins:
    """Who writes an activation-gradient buffer first and who accumulates, decided once while the backward pass is planned:
    the steps run in the order they are planned, so the first step that asks for a buffer stores into it and every later
    one adds.  `buffers`: key -> gradient buffer (any mapping: the class only looks keys up); `balanced`: the pyramid levels
    whose readers read BalanceFeatures' copy, so their gradient goes to the `bal:` key.  writers: key -> the labels of the
    steps that wrote it, in order."""

    def __init__(self, buffers, balanced=()):
        self.buffers, self.balanced = buffers, balanced
        self.writers = {}

    def add(self, name, label, balanced=True):
        """(gradient buffer of tensor `name`, accumulate: an earlier step has written it) for a step that can do either.
        balanced=False: the step's forward read the tensor itself, not the balanced copy (residual inputs)."""
        key = "bal:" + name if balanced and name in self.balanced else name
        buf = self.buffers[key]
        before = self.writers.setdefault(key, [])
        before.append(label)
        return buf, len(before) > 1

    def sole(self, name, label):
        """Gradient buffer of tensor `name` for a step whose kernel overwrites it: an earlier writer's contribution would
        be lost, so there must be none."""
        buf = self.buffers[name]
        before = self.writers.setdefault(name, [])
        if before:
            raise RuntimeError(f"{label} overwrites the gradient of {name}, which {before[0]} has already written")
        before.append(label)
        return buf


def mean_loss_dict(outs):
    """The loss dict of an accumulated optimizer step from those of its micro-steps: the mean of every entry, except
    l2-regularization, which is the last micro-step's (the weights do not change inside a step)."""
    out = {}
    for k, last in outs[-1].items():
        if k == "l2-regularization" or not (torch.is_tensor(last) or isinstance(last, (int, float))):
            out[k] = last
            continue
        total = outs[0][k]
        for o in outs[1:]:
            total = total + o[k]
        out[k] = total / len(outs)
    return out


class TrainEngine:
    def __init__(self, model, batch_size, frozen_regexes=(), process_group=None, world_size=None, frozen_names=(),
                 launch_opts=None, wide_pred_terms=None, force_dp=None, accumulation_steps=1):
        """launch_opts: `_C.LaunchOpts` (or a dict of its fields) copied into every rn_conv_problem / rn_wgrad_problem of
        THIS engine (include/rnet_hip.h rn_launch_opts) — kernel-family overrides for tests and A/B timing; the library
        has no process-wide knobs.
        wide_pred_terms: bf16 weight planes the TRAINING forward of the wide dtype=float32 prediction conv (the class
        head's 720-channel layer, detection_head.py:80-88) multiplies by — 2 = the split-bf16 form of its f32 kernel
        (inference / export always use it), 1 = rb(w) only.  Default: RNET_TRAIN_PRED_W_TERMS, else
        params.training.prediction_weight_planes, else 2 (the reference's f32 layer).  History: round 5 made ONE plane the
        default on an A/B taken at the reference's initialisation, where the logits are bias + a small kernel term (spread
        0.33): class-loss moved by 3.1e-7 relative.  Round 6 repeated the A/B in the trained-detector regime — the class-
        prediction kernel scaled by 7, logit spread 2.3 (tools/ab_pred_planes.py --pred-scale 7,
        profiles/r06_ab_pred_planes_scale7.json): the class-loss moves by 4.3e-5 relative, above the 1e-5 the contract
        allows for the loss (gradient cosines stay > 0.99999) — so the default went back to two planes; one plane remains
        a documented opt-in worth 0.8 ms of the 29 ms step.  The narrow box-regression layer always keeps both planes.
        force_dp (default RNET_FORCE_DP=1): run the data-parallel machinery — SyncBN messages, the bucketed gradient
        all-reduce overlapped with the backward pass, the clip flag read — although this engine has ONE replica, over
        whatever process group it was given (a 1-rank `nccl` group: bench.py's `extra.dp_overhead`, the cost of that
        machinery on one GPU; losses and gradients equal the plain step's).
        accumulation_steps (training.gradient_accumulation_steps): N micro-batches of `batch_size` images per optimizer step,
        taken one after another the way the reference takes its replicas side by side (DESIGN "Gradient accumulation");
        1 = the plain train_step, and nothing of the accumulation exists."""
        self.model = model
        self.accumulation_steps = int(accumulation_steps)
        if self.accumulation_steps < 1:
            raise ValueError(f"accumulation_steps must be an integer >= 1, not {accumulation_steps!r}")
        self.g = model.graph
        self.params_cfg = model.params
        self.B = int(batch_size)
        self.dev = model.device
        # ---- switches: every environment read of the engine, once.  (GradientOverlap reads its own; RNET_C1_OVERLAP at the head
        # of every backward pass: bench.py and the data-parallel tests flip it on a live engine.)
        env = os.environ.get
        if force_dp is None:
            force_dp = env("RNET_FORCE_DP", "0") == "1"
        if wide_pred_terms is None:
            wide_pred_terms = env("RNET_TRAIN_PRED_W_TERMS") or \
                getattr(getattr(model.params, "training", None), "prediction_weight_planes", None) or 2
        comm_cus = int(env("RNET_COMM_CUS", "8"))
        self.fuse_bn_stats = env("RNET_FUSE_BN_STATS", "1") != "0"   # conv epilogue writes BN partial sums
        # data-gradient epilogue writes stage 1 of the BatchNorm backward reduction of the layer it produces dz for
        self.fuse_bn_bwd = env("RNET_FUSE_BN_BWD", "1") != "0"
        # =2: also the multi-segment groups (the four head-tower depths).  Measured same-box: 3-4 more 122 us reduction
        # launches go, the eight 550 us tower data gradients get ~15 us longer each in the step: +0.25 % on the step
        # (round 3, with the weight-gradient CU cap: 31.06 -> 30.92 ms, +0.45 %, tools/probes/ab_env.sh) for -0.026 on the
        # dominant kernel's MFMA fraction, the figure bench.py's roofline reports — off by default, the capability stays tested
        self.fuse_bn_bwd_groups = env("RNET_FUSE_BN_BWD", "1") == "2"
        # weight / bias gradient launches on a second HIP stream: nothing in the backward pass reads them, so they
        # run beside the data-gradient chain (MFMA-bound wgrad next to the HBM-bound BatchNorm backward kernels)
        self.side_stream_on = env("RNET_WGRAD_STREAM", "1") != "0"
        cus = env("RNET_WGRAD_CUS", "160,208")   # round 6, same-box A/B (profiles/r06_ab/wgrad_cus.txt): 176,256 28.23, 160,208 28.01, 144,192 28.02, 112,192 30.3 ms
        self._wgrad_cap = tuple(int(v) for v in cus.split(",")) if cus not in ("0", "") else None
        if not self.side_stream_on:
            self._wgrad_cap = None      # one-stream backward: nothing to leave CUs to
        if self._wgrad_cap and len(self._wgrad_cap) == 1:
            self._wgrad_cap = (self._wgrad_cap[0], 2 * self._wgrad_cap[0])
        self._wgrad_group_mode = env("RNET_WGRAD_GROUP", "halo")   # "0" | "halo" | "all": see _group_wgrad_steps
        self._ab_workspaces = env("RNET_AB_WORKSPACES") == "1"     # tools/ab_step.py switches kernel families between rounds
        # ---- configuration
        self.f16 = half_activations(model.params)    # (+ the LossScaleOptimizer arithmetic of optimizer_step)
        self.h16 = torch.float16 if self.f16 else torch.bfloat16
        self._DT = {"bf16": self.h16, "f32": torch.float32}
        self.lib = _C.lib(self.f16)
        self.pg = process_group
        if world_size is None:   # one source of truth with RetinaNetLoss, which asks torch.distributed
            import torch.distributed as dist
            world_size = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.world = int(world_size)
        bn = self.params_cfg.architecture.batch_norm
        self.eps, self.momentum_bn = float(bn.epsilon), float(bn.momentum)
        self.dp_active = self.world > 1 or bool(force_dp)    # collectives are issued (over 1 rank when forced)
        self.sync_bn = bool(bn.use_sync) and self.dp_active
        if isinstance(launch_opts, dict):
            launch_opts = _C.LaunchOpts(**launch_opts)
        self.launch_opts = launch_opts.copy() if launch_opts is not None else _C.LaunchOpts()
        # data parallel: the persistent kernels leave a few CUs to RCCL (rn_launch_opts.reserved_cus)
        if self.dp_active and not self.launch_opts.reserved_cus:
            self.launch_opts.reserved_cus = comm_cus
        # the per-device handle (rn_create): device, CU count, this engine's launch defaults; owns the native communicators
        self.handle = _C.Handle(self.lib, self.dev.index if self.dev.index is not None else torch.cuda.current_device(),
                                self.launch_opts)
        self.wide_pred_terms = max(1, min(int(wide_pred_terms), _C.PRED_W_TERMS))
        self.frozen = set(frozen_names)
        for k in model.variables:
            if any(rx.search(k) for rx in frozen_regexes):
                self.frozen.add(k)
        self._check_frozen_layers()
        # ---- what the build records
        self._keep = []
        self._algo = {}           # id(rn_conv_problem) -> (algorithmic FLOPs, algorithmic bytes) where the launch executes more
        self.conv_launches = []   # (name, rn_conv_problem) of every implicit-GEMM launch: lib.rn_conv_kernel_id(byref(p))
        self._launch_names = {}   # id(rn_conv_problem) -> that name (bench.py's layer_profile rows)
        self.wgrad_launches = []  # (name, rn_wgrad_problem) of every weight-gradient launch
        # (name, "fwd" | "dgrad", rn_dw_problem, rn_upsample_zero2x arguments run before it) of every depthwise launch
        self.dw_launches = []
        self.dw_wgrad_launches = []   # (name, rn_dw_problem) of every depthwise weight-gradient launch
        self.se_launches = []     # (name, "fwd" | "bwd", N, HW, C, se) of every squeeze-excite launch
        self._wgrad_capped = []   # (problem, capped target): set_wgrad_cap(False) lifts the cap (bench.py's exclusive step)
        self.stem_packed = None   # live first-layer conv: its kernel as [Cout_pad][R rows][8 taps x 4 ch], repacked per step
        self._bn_of_tensor = {}   # output of a live-BatchNorm layer -> (rn_bn_problem, segment, op, segments of the problem)
        self.bn_bwd_ws = {}       # id(rn_bn_problem) -> workspace that holds the externally written backward partials
        self._bn_bwd_pending = {}  # id(rn_bn_problem) -> segments whose dz-writing launch is planned (see _fuse_bn_bwd)
        self.bn_bwd_fused = []    # tensor names whose BatchNorm backward reduction runs in a dgrad epilogue
        self.dy_of = {}           # conv output -> gradient at the conv's own (pre-BatchNorm) output, what wgrad / dgrad read
        self._loss_dy = None      # loss_grad_buffers(): the prediction convs' entries of dy_of
        self._dgrad_pack_items = None   # rn_dgrad_pack array over dgrad_packs
        self.frozen_dgrad_packs = []    # (kernel variable, conv dims, packed buffer, mode) of frozen convs: packed on load
        self.frozen_dw_flip_packs = []  # (kernel variable, k, C, packed buffer) of frozen depthwise layers: packed on load
        self._frozen_folded = False     # _fold_frozen has run: load_from_model re-enters it
        self.drop_connect = True     # stochastic depth of the EfficientNet skip blocks (efficientnet.py:97-113)
        self.fusion_state = {}       # id(weighted top-down op) -> forward.FusionState (weights, coefficient blocks)
        self.dc_masks = {}           # project conv output -> (f32[B] factors, survival_prob)
        self.dc_all = self.dc_p = None
        self.dc_generator = torch.Generator(device=self.dev)
        self.dc_generator.manual_seed(1337)
        # ---- state of the steps
        self.step_count = 0
        self.loss_scale = None    # LossScaleOptimizer state (mixed_float16 configs): see optimizer_step
        self._ls_host = self._ls_event = None   # pinned copy of the "gradients not finite" flag and its event
        self._ls_pending = False  # that copy has not been looked at yet (_resolve_loss_scale)
        self._wi = None           # weights_info(): workspace, device results, pinned results — made on first use
        self._train_step_active = False
        self._micro_next = 0      # the micro-step accumulate_micro_step expects next (accumulation_steps > 1)
        self._micro_scale = 1.0   # the loss scale of the optimizer step under way: one for all its micro-steps
        self._micro_messages = 0  # SyncBN messages of the micro-steps so far
        self._images_ref = None   # the caller's batch while forward() reads it in place
        self._step_args = dict(wdc=0.0, alpha=0.0, unscale=1.0, clip=0.0)
        self._side_stream = None
        self._side_events = []
        self.side_stream_probed = None
        self._dgrad_prepacked = False   # train_step repacked the data-gradient weights beside the forward pass
        self.conv_profile = None
        self.wgrad_profile = None   # bench.py: list that collects (event0, event1, algorithmic FLOPs, kernel) per wgrad launch
        # bench.py `roofline.layers`: list that collects (event0, event1, launch name, algorithmic FLOPs, algorithmic bytes,
        # kernel) for EVERY implicit-GEMM launch of the step — forward, data gradient, weight gradient
        self.layer_profile = None
        self.hbm_profile = None   # bench.py: list that collects (event0, event1, kernel name, algorithmic bytes)
        # ---- data parallel (self.overlap follows the arenas it works on)
        self.small = SmallMessages(self.lib, self.dev, self.pg, self.world, self.sync_bn)
        self.syncbn_messages_per_step = None   # their count in the last train_step (bench.py: config.syncbn_messages)
        self.price_without_flag_read = False   # bench.py's extra.dp_overhead sets it: see GradientOverlap.finish
        self._prepare_graph()
        with torch.cuda.device(self.dev):
            # split-K of the persistent conv kernels' last round (rn_conv_problem.splitk_ws): every forward / data-gradient
            # launch runs on the main stream, in order, so one workspace serves them all; attached at creation because the
            # dispatcher looks at it
            self.splitk_ws = _C.new_splitk_workspace(self.lib, self.dev)
            # inference form (frozen conv and BatchNorm, no gradient needed at the input): packed weights and folded
            # BatchNorm at stable addresses; the same rule decides the pixel-pair form, so a raw (pre-BN) launch never
            # sees pair-packed weights
            self.folded = FoldedConvs(self.lib, self.g, self.B, self.dev, self.h16, self.launch_opts, self.splitk_ws,
                                      self.eps, eligible=self._inference_form)
            self._analyse()
            self._alloc_params()
            self._alloc_tensors()
            self._fold_frozen()
            self._build_forward()
            self._build_backward()
            self._group_wgrad_steps()
            self.overlap = GradientOverlap(
                self.lib, self.dev, G=self.G, P=self.P, metrics=self.metrics, segs_dev=self.segs_dev,
                block_seg_dev=self.block_seg_dev, n_blocks=self.n_blocks, n_segs=self.n_segs, opt_ws=self.opt_ws,
                train_names=self.train_names, p_off=self.p_off, seg_blocks=self._seg_blocks, ready_steps=self._ready_steps,
                small=self.small, pg=self.pg, world=self.world, dp_active=self.dp_active,
                side_stream=lambda: self._side_stream, accumulation_steps=self.accumulation_steps)
            for name, cp in self.conv_launches:   # a launch writes stage-1 BatchNorm partials for all its segments or none
                marks = {bool(cp.seg[i].bn_bwd_y) for i in range(cp.num_segments)}
                if name.startswith("dgrad:") and len(marks) != 1:
                    raise RuntimeError(f"{name}: BatchNorm backward fusion covers only part of the launch's segments")

    # ------------------------------------------------------------------------------------------
    def _prepare_graph(self):
        """Engine-local copy of the op list: a trainable squeeze-excite runs out of place in training (its backward
        needs the un-gated input), so such `se` ops get an output tensor `<t>:se` and later readers of `<t>` are
        redirected to it; a frozen one gates `<t>` in place as the serving engine does (inp = out = `<t>`).  Also
        classifies every variable (compute layout, weight decay)."""
        g = self.g
        self.tensors = dict(g.tensors)
        self.ops = []
        alias = {}
        for op in g.ops:
            o = dict(op)
            for key in ("inp", "residual"):
                if o.get(key) in alias:
                    o[key] = alias[o[key]]
            if o["op"] == "se" and not self._se_trainable(o):
                o["inp"] = o["out"] = alias.get(o["tensor"], o["tensor"])
            elif o["op"] == "se":
                t = o["tensor"]
                o["inp"], o["out"] = alias.get(t, t), t + ":se"
                self.tensors[o["out"]] = g.tensors[t]
                alias[t] = o["out"]
            if o["op"] in ("topdown",):
                o["ins"] = [alias.get(n, n) for n in o["ins"]]
            self.ops.append(o)
        self.readers = tensor_readers(self.ops)
        # variable name -> (kind, layer): conv / dw / se1 / se2 kernels are weight-decayed
        # (executor.py:308-327: every trainable variable with 'kernel' in its name)
        self.var_kind = {}
        for cname, c in g.convs.items():
            self.var_kind[c.get("kvar", cname + "/kernel")] = ("conv", cname)
        for dname, d in getattr(g, "dws", {}).items():
            self.var_kind[d["kvar"]] = ("dw", dname)
        for sname in getattr(g, "ses", {}):
            self.var_kind[sname + "/conv2d/kernel"] = ("se1", sname)
            self.var_kind[sname + "/conv2d_1/kernel"] = ("se2", sname)
        # FeatureFusion's weights are decayed too: the reference decays every trainable variable of a layer that is no
        # conv layer whose name contains 'kernel' or 'weight' (executor.py:320-323)
        for o in self.ops:
            if o["op"] == "topdown" and o.get("fusion"):
                for j, pair in enumerate(o["fusion_vars"]):
                    for name in pair:
                        self.var_kind[name] = ("fusion", j)

    def _kvar(self, op):
        if op["op"] == "dwconv":
            return self.g.dws[op["dw"]]["kvar"]
        c = self.g.convs[op["conv"]]
        return c.get("kvar", op["conv"] + "/kernel")

    def _conv_trainable(self, op):
        return self._kvar(op) not in self.frozen

    def _bn_trainable(self, op):
        return op.get("bn") and (op["bn"] + "/gamma") not in self.frozen

    def _bn_frozen(self, op):
        """BatchNorm in inference mode under a trainable conv (the `bn` / `*-bn` freeze patterns)"""
        return bool(op.get("bn")) and self._conv_trainable(op) and not self._bn_trainable(op)

    _SE_VARS = ("/conv2d/kernel", "/conv2d/bias", "/conv2d_1/kernel", "/conv2d_1/bias")

    def _se_trainable(self, op):
        return (op["se"] + self._SE_VARS[0]) not in self.frozen

    def _launch_of(self, op):
        """the ops of the launch conv / depthwise `op` runs in: its group, or the op alone"""
        return [op] if op.get("group") is None else self._group_ops(op["op"], op["group"])

    def _passes_gradient(self, op):
        """the launch of frozen conv / depthwise `op` hands a gradient down: an input or residual of one of its ops needs one"""
        return any(self.requires.get(i) for o in self._launch_of(op) for i in (o["inp"], o.get("residual")) if i)

    def _bn_apart(self, op):
        """BatchNorm in inference mode as a step of its own — the raw conv output, then rn_bn_apply on the constant scale /
        shift table: under a trainable conv (_bn_frozen); under a frozen conv whose launch hands a gradient down (the gate
        bits and rn_bn_frozen_bwd need the step); under the frozen project conv of a drop_connect block, whose per-image
        factor stands between the BatchNorm and the residual add where the folded conv epilogue has no place for it."""
        if not op.get("bn") or self._bn_trainable(op):
            return False
        if self._conv_trainable(op):
            return True
        return self._passes_gradient(op) or (self.drop_connect and any(o.get("survival") is not None
                                                                      for o in self._launch_of(op)))

    def _inference_form(self, op):
        return not self._conv_trainable(op) and not self._bn_trainable(op) and not self.requires.get(op["inp"])

    def _check_frozen_layers(self):
        """The reference freezes per Keras layer (executor.py:168-175), this engine per variable name: the two agree when
        every layer's variables are frozen together, which the eight FREEZE_VARS_REGEX patterns guarantee."""
        g = self.g
        layers = [[b + sfx for sfx in ("/gamma", "/beta", "/moving_mean", "/moving_variance")] for b in g.bns]
        layers += [[s + sfx for sfx in self._SE_VARS] for s in getattr(g, "ses", {})]
        dws = getattr(g, "dws", {})
        for cname, c in g.convs.items():
            names = [c.get("kvar", cname + "/kernel")] + ([cname + "/bias"] if c["bias"] else [])
            if cname + ":dw" in dws:      # SeparableConv2D: depthwise_kernel, pointwise_kernel and bias are one layer
                names.append(dws[cname + ":dw"]["kvar"])
            layers.append(names)
        for names in layers:
            n = sum(k in self.frozen for k in names)
            if 0 < n < len(names):
                raise ValueError(f"freeze patterns split a layer: {[k for k in names if k in self.frozen]} frozen, "
                                 f"{[k for k in names if k not in self.frozen]} not (the reference freezes whole layers)")

    def _analyse(self):
        self.requires = {"images": False}
        for op in self.ops:
            kind = op["op"]
            if kind in ("conv", "stem", "dwconv"):
                # a grouped launch stands where its first op does and has one form: a frozen one hands a gradient down
                # when any of its ops' inputs needs one
                if op["out"] in self.requires:
                    continue
                launch = self._launch_of(op)
                below = any(self.requires[i] for o in launch for i in (o["inp"], o.get("residual")) if i)
                for o in launch:
                    self.requires[o["out"]] = self._conv_trainable(o) or bool(self._bn_trainable(o)) or below
            elif kind == "maxpool":
                self.requires[op["out"]] = self.requires[op["inp"]]
            elif kind == "topdown":
                live = [n for pair in op.get("fusion_vars", ()) for n in pair if n not in self.frozen]
                dead = [i for i in op["ins"] if not self.requires[i]]
                if live and dead:   # the weighted backward level writes din of every level: such an input has no buffer
                    raise NotImplementedError(f"fusion weights {live[0]} .. train while the top-down inputs {dead} are "
                                              "frozen down to the image: freeze the fusion weights with them")
                r = any(self.requires[i] for i in op["ins"]) or bool(live)
                for o in op["outs"]:
                    self.requires[o] = r or self.requires.get(o, False)
            elif kind == "balance":
                pass
            elif kind == "se":
                if not self._se_trainable(op) and self.requires[op["inp"]]:
                    # squeeze-excite sits in the backbone, the bottom of the model: no freeze pattern leaves a frozen one
                    # above a trainable layer, and there is no backward of it without its weight gradients
                    raise NotImplementedError(f"squeeze-excite {op['se']} is frozen while layers below it train: its "
                                              "backward without weight gradients is not built (no freeze pattern "
                                              "produces it)")
                self.requires[op["out"]] = self._se_trainable(op)
            else:
                raise NotImplementedError(f"training through '{kind}' ops is not built")
        # The reference's `backbone` / `resnet_initial` freeze patterns exclude fpn, box-head and class-head by name, not
        # the auxiliary head (model/builder.py FREEZE_VARS_REGEX), so they freeze it; its loss gradient would then have
        # to cross frozen convs into the trainable FPN, a backward form this engine does not have
        for op in self.ops:
            if op["op"] in ("conv", "dwconv") and op["out"].startswith("auxillary-head") and \
                    not self._conv_trainable(op) and self.requires.get(op["inp"]):
                raise NotImplementedError(f"auxillary-head: {self._kvar(op)} is frozen while the layers below it train "
                                          "(the reference's `backbone` and `resnet_initial` freeze patterns match the "
                                          "auxillary head): backward through a frozen head is not built — freeze "
                                          "by patterns that leave `auxillary-head` trainable")
        # a conv layer is "live" when its kernel trains.  Live conv + frozen BatchNorm is what the `bn` / `*-bn` freeze
        # patterns produce (_bn_frozen); a frozen conv under a live BatchNorm comes out of none of the eight patterns
        for op in self.ops:
            if op["op"] in ("conv", "stem", "dwconv") and op.get("bn") and \
                    not self._conv_trainable(op) and self._bn_trainable(op):
                raise NotImplementedError(f"{self._kvar(op)}: a frozen conv under a trainable BatchNorm is not built "
                                          "(no freeze pattern produces it)")

    # ---- flat parameter arenas ---------------------------------------------------------------------
    def _alloc_params(self):
        lib = self.lib
        chunk = lib.rn_optim_chunk()
        v = self.model.variables
        names = [k for k in v if self.g.var_specs[k].get("trainable", True) and k not in self.frozen]
        self.train_names = names
        segs, block_seg = [], []
        # the first 4 floats of every arena are reserved: G[0] / G[1] are the "a clip factor != 1 on some rank" /
        # "gradients not finite on some rank" slots that ride in the LAST gradient bucket's all-reduce (the bucket
        # at the front of the arena completes last in the backward pass)
        off, bf_off, nblk = 4, 0, 0
        self.p_off, self.bf_off = {}, {}     # bf_off: conv name | "dw:<name>" | "<se>:w1" / "<se>:w2" -> offset in Pbf
        self.fwd_packs = []                  # live convs whose Cin is not its own K-step padding: repacked per step
        self.fwd_pack_of = {}
        self.split_packs = []                # live f32 convs (prediction layers): split-bf16 planes, repacked per step
        self.split_pack_of = {}
        self.pair_packs = set()              # ... those of them whose two planes are stacked along Cout (w_pair)
        f32_convs = {o["conv"] for o in self.ops if o["op"] == "conv" and o.get("out_dtype") == "f32"}
        for i, k in enumerate(names):
            n = v[k].numel()
            kind, layer = self.var_kind.get(k, ("other", None))
            bfo = -1
            if kind == "conv":
                c = self.g.convs[layer]
                if c["cin"] == 3:
                    pass                                        # first-layer conv: its own packed form
                elif layer in f32_convs and self._f32_terms(layer) > 1:
                    cinp = lib.rn_conv_cin_pad(c["cin"])        # detection_head.py:80-88: the layer keeps its f32 kernel
                    if self.folded.w_pair(layer):               # narrow layer (box prediction): the planes along Cout
                        buf = torch.zeros((lib.rn_conv_pair_rows(c["cout"]), c["k"], c["k"], cinp), dtype=self.h16,
                                          device=self.dev)
                        self.pair_packs.add(layer)
                    else:
                        buf = torch.zeros((lib.rn_conv_cout_pad(c["cout"]), c["k"], c["k"], self._f32_terms(layer) * cinp),
                                          dtype=self.h16, device=self.dev)
                    self.split_packs.append((k, c, cinp, buf))
                    self.split_pack_of[layer] = buf
                elif lib.rn_conv_cin_pad(c["cin"]) == c["cin"]:
                    bfo = bf_off                                # plain cast of the master = the compute layout
                    self.bf_off[layer] = bf_off
                    bf_off += lib.rn_conv_cout_pad(c["cout"]) * c["k"] * c["k"] * c["cin"]
                else:
                    cinp = lib.rn_conv_cin_pad(c["cin"])
                    buf = torch.zeros((lib.rn_conv_cout_pad(c["cout"]), c["k"], c["k"], cinp), dtype=self.h16,
                                      device=self.dev)
                    self.fwd_packs.append((k, c, cinp, buf))
                    self.fwd_pack_of[layer] = buf
            elif kind == "dw":
                bfo = bf_off
                self.bf_off["dw:" + layer] = bf_off
                bf_off += n
            elif kind in ("se1", "se2"):
                bfo = bf_off
                self.bf_off[layer + (":w1" if kind == "se1" else ":w2")] = bf_off
                bf_off += n
            bf_off = (bf_off + 7) // 8 * 8
            nb = (n + chunk - 1) // chunk
            segs.append((off, n, 1 if kind != "other" else 0, nblk, nb, 0, bfo))   # executor.py:308-327: kernels only
            block_seg += [i] * nb
            self.p_off[k] = (off, n)
            off += (n + 3) // 4 * 4
            nblk += nb
        self.n_params = off
        self.P = torch.zeros((off,), dtype=torch.float32, device=self.dev)
        self.G = torch.zeros_like(self.P)
        # gradient accumulation: sum over the micro-steps of factor * t, layout of G (A[0:2]: the flags; rn_optim_clip_accumulate)
        self.A = torch.zeros_like(self.P) if self.accumulation_steps > 1 else None
        # optimizer slots: V is the step kernel's slot 0 (SGD `momentum`, Adam `m`, RMSprop `rms`, Adagrad `accumulator`);
        # S1 / S2 exist only while the configured rule has a second / third slot (_bind_optimizer)
        self.V = torch.zeros_like(self.P)
        self.S1 = self.S2 = None
        self._slot_spec = [("momentum", 0.0), None, None]
        self._slot_owner = "sgd"
        self.E = torch.zeros_like(self.P)
        self.Pbf = torch.zeros((max(bf_off, 8),), dtype=self.h16, device=self.dev)
        self._bf_copies = [(self.p_off[k], s[6]) for k, s in zip(names, segs) if s[6] >= 0]
        seg_np = np.zeros((len(segs),), dtype=_SEG_DTYPE)
        for i, s in enumerate(segs):
            seg_np[i] = s
        self.segs_dev = torch.from_numpy(seg_np.view(np.uint8).copy()).to(self.dev)
        self.block_seg_dev = torch.tensor(block_seg, dtype=torch.int32, device=self.dev)
        self.n_blocks, self.n_segs = len(block_seg), len(segs)
        self.opt_ws = torch.empty((lib.rn_optim_workspace_bytes(self.n_blocks, self.n_segs),), dtype=torch.uint8,
                                  device=self.dev)
        self.metrics = torch.zeros((8,), dtype=torch.float32, device=self.dev)
        self._block_elems = [(segs[si][0] + (bi - segs[si][3]) * chunk, min(chunk, segs[si][1] - (bi - segs[si][3]) * chunk))
                             for bi, si in enumerate(block_seg)]   # (arena offset, elements) of every optimizer block
        self._seg_blocks = {k: (s[3], s[4]) for k, s in zip(names, segs)}   # variable -> (first block, blocks)
        stem = self._stem_op()
        if self._conv_trainable(stem):
            c = self.g.convs[stem["conv"]]
            self.stem_packed = torch.zeros((lib.rn_conv_cout_pad(c["cout"]), c["k"], 32), dtype=self.h16, device=self.dev)
        self.load_from_model()

    def _pview(self, name, arena=None):
        off, n = self.p_off[name]
        return (self.P if arena is None else arena)[off:off + n]

    def _to_compute_layout(self, k, t):
        kind = self.var_kind.get(k, ("other", None))[0]
        return _hwio_to_ohwi(t) if kind in ("conv", "se1", "se2") else t

    def load_from_model(self):
        """model.variables (Keras layouts) -> flat arenas (conv / SE kernels as [Cout][R][S][Cin], depthwise
        kernels as [k*k][C]) + bf16 compute copies."""
        v = self.model.variables
        for k in self.train_names:
            t = self._to_compute_layout(k, v[k].to(self.dev, torch.float32))
            self._pview(k).copy_(t.reshape(-1))
        self.E.copy_(self.P)
        self._bind_optimizer(reset=True)
        for (off, n), bfo in self._bf_copies:
            self.Pbf[bfo:bfo + n].copy_(self.P[off:off + n])
        self.refresh_packs()
        if self._frozen_folded:     # a reload: the frozen layers' packed weights, folded BatchNorm and data-gradient packs
            self._fold_frozen()
        else:
            self._fill_frozen_bn()

    def _bind_optimizer(self, reset=False):
        """Slot arenas for the optimizer the model holds NOW (tests and tools replace `model.optimizer` after the engine
        is built): one arena per slot of its rule and no more — SGD keeps exactly V.  A rule or slot set other than the
        bound one (re)allocates and starts every slot at its initial value (Adagrad's accumulator: 0.1); reset=True
        does the latter on its own."""
        opt = getattr(self.model, "optimizer", None)
        owner = opt.name if opt is not None else "sgd"
        spec = list(opt.slots()) if opt is not None else [("momentum", 0.0)]
        spec += [None] * (3 - len(spec))
        changed = (owner, spec) != (self._slot_owner, self._slot_spec)
        if changed:
            self._slot_owner, self._slot_spec = owner, spec
            self.S1 = (self.S1 if self.S1 is not None else torch.zeros_like(self.P)) if spec[1] else None
            self.S2 = (self.S2 if self.S2 is not None else torch.zeros_like(self.P)) if spec[2] else None
        if changed or reset:
            for arena, s in zip((self.V, self.S1, self.S2), self._slot_spec):
                if s is not None:
                    arena.fill_(s[1])
        return opt

    def _slot_arena(self, slot):
        """the arena that holds Keras slot `slot` of the bound optimizer (`average`: the moving average), or None"""
        if slot == "average":
            return self.E
        for arena, s in zip((self.V, self.S1, self.S2), self._slot_spec):
            if s is not None and s[0] == slot:
                return arena
        return None

    def _stem_op(self):
        return next(o for o in self.ops if o["op"] == "stem")

    def refresh_packs(self):
        """per-step repacks from the f32 masters: the live first-layer conv ([Cout][R][S][3] ->
        bf16 [Cout_pad][R rows][8 taps x 4 ch]) and live convs whose Cin is zero-padded to the K step."""
        st = _C.current_stream()
        op = self._stem_op()
        if self._conv_trainable(op):
            c = self.g.convs[op["conv"]]
            k = c["k"]
            w = _ohwi_to_hwio(self._pview(self._kvar(op)).reshape(c["cout"], k, k, 3))
            _C.check(self.lib.rn_pack_stem_weight_rs(_C.ptr(w), k, k, c["cout"], _C.ptr(self.stem_packed), st),
                     "rn_pack_stem_weight_rs")
        for (kname, c, cinp, buf) in self.fwd_packs:
            off, _ = self.p_off[kname]
            _C.check(self.lib.rn_pack_conv_weight_ohwi(self.P.data_ptr() + 4 * off, c["k"], c["k"], c["cin"], c["cout"],
                                                       cinp, buf.data_ptr(), st), "rn_pack_conv_weight_ohwi")
        for (kname, c, cinp, buf) in self.split_packs:
            off, _ = self.p_off[kname]
            if self.var_kind[kname][1] in self.pair_packs:
                _C.check(self.lib.rn_pack_conv_weight_pair(self.P.data_ptr() + 4 * off, 1, c["k"], c["k"], c["cin"],
                                                           c["cout"], cinp, buf.data_ptr(), st), "rn_pack_conv_weight_pair")
                continue
            _C.check(self.lib.rn_pack_conv_weight_split(self.P.data_ptr() + 4 * off, 1, c["k"], c["k"], c["cin"],
                                                        c["cout"], cinp, self._f32_terms(self.var_kind[kname][1]),
                                                        buf.data_ptr(), st), "rn_pack_conv_weight_split")

    def _keras_layout(self, k, arena):
        """Variable `k` of a flat arena in the layout Keras holds it (conv / SE kernels HWIO)."""
        v = self.model.variables[k]
        t = self._pview(k, arena)
        if self.var_kind.get(k, ("other", None))[0] in ("conv", "se1", "se2"):
            kh, kw, ci, co = v.shape
            t = _ohwi_to_hwio(t.reshape(co, kh, kw, ci))
        return t.reshape(v.shape)

    def optimizer_slots(self):
        """{(variable, slot): f32 array}: the optimizer's slots under their Keras names (SGD `momentum`; Adam `m`, `v`,
        `vhat`; RMSprop `rms`, `momentum`, `mg`; Adagrad `accumulator`) and the moving-average `average` copies
        (optimizers/builder.py:27-71 — what `save_weights` stores next to the weights for a resume)."""
        self._bind_optimizer()
        out = {}
        for k in self.train_names:
            for arena, s in zip((self.V, self.S1, self.S2), self._slot_spec):
                if s is not None:
                    out[(k, s[0])] = self._keras_layout(k, arena).detach().cpu().numpy().copy()
            out[(k, "average")] = self._keras_layout(k, self.E).detach().cpu().numpy().copy()
        return out

    def load_optimizer_slots(self, slots, only=None):
        """Inverse of `optimizer_slots`; variables without a stored slot keep their current state, and so do slots the
        bound optimizer does not have.  only: restrict to these slot names."""
        self._bind_optimizer()
        for (k, slot), arr in slots.items():
            arena = self._slot_arena(slot)
            if k not in self.p_off or arena is None or (only is not None and slot not in only):
                continue
            t = self._to_compute_layout(k, torch.as_tensor(np.asarray(arr), dtype=torch.float32).to(self.dev))
            self._pview(k, arena).copy_(t.reshape(-1))

    def save_checkpoint(self, prefix):
        """Weights + BN moving statistics + optimizer slots (SGD `momentum`, Adam `m` / `v` / `vhat`, RMSprop `rms` /
        `momentum` / `mg`, Adagrad `accumulator`; `average`) + the step counter (`<Class>/iter`), in
        TensorFlow's checkpoint FILE format (where executor.py:652-654 / 695-697 call `model.save_weights`).  Interop
        is one-way: this build reads what the reference wrote (by variable name through the object graph); the
        reference's Keras `load_weights` matches structurally and will not consume the flat object graph written
        here (retinanet/tf_checkpoint.py::save_weights).  Written between optimizer steps: the accumulator of a
        step under way (accumulation_steps > 1) is no part of it."""
        if self._micro_next != 0:
            raise RuntimeError(f"save_checkpoint inside an optimizer step: {self._micro_next} of "
                               f"{self.accumulation_steps} micro-steps accumulated")
        with torch.cuda.device(self.dev):
            self.store_to_model(use_ema=False)
            torch.cuda.synchronize()
        self.finish_step()
        from retinanet.optimizers.builder import iter_key
        extra = {iter_key(self.model.optimizer): np.asarray(self.step_count, dtype=np.int64)}   # SGD/iter, Adam/iter, ...
        if self.loss_scale:   # Keras' LossScaleOptimizer checkpoints its dynamic state the same way
            extra["loss_scale/current_loss_scale"] = np.asarray(self.loss_scale["scale"], dtype=np.float32)
            extra["loss_scale/good_steps"] = np.asarray(self.loss_scale["good"], dtype=np.int64)
        loss = self.model.loss
        if loss is not None and loss.use_moving_average_normalizer:
            # this rank's value (only the chief writes checkpoints; the reference reads the ON_READ variable as the
            # mean over the replicas: DESIGN 7c)
            state = loss.moving_average_normalizer   # None before the first loss call: the initial 0.0
            extra["loss/moving_average_normalizer"] = (np.zeros((), np.float32) if state is None
                                                       else state.cpu().numpy().reshape(()).copy())
        self.model.save_weights(prefix, slots=self.optimizer_slots(), extra=extra)

    def restore_checkpoint(self, prefix):
        """executor.py:221-244: load the latest weights and continue from their step."""
        with torch.cuda.device(self.dev):
            slots = self.model.load_weights(prefix)
            self.load_from_model()
            for bn, d in self.bn_state.items():
                d["mm"].copy_(self.model.variables[bn + "/moving_mean"])
                d["mv"].copy_(self.model.variables[bn + "/moving_variance"])
            self._fold_frozen()
            from retinanet.optimizers.builder import iter_key, read_iterations
            it, wrote = read_iterations(self.model.loaded_extras, self.model.optimizer)
            mine = iter_key(self.model.optimizer)[:-len("/iter")]
            if wrote in (None, mine):
                self.load_optimizer_slots(slots)
            else:   # another optimizer wrote the file: its slots mean nothing to this one (and may share a name)
                import logging
                logging.warning("checkpoint %s was written by %s, the configured optimizer is %s: weights, moving "
                                "averages and the step counter are restored, %s starts with fresh slots", prefix, wrote,
                                mine, mine)
                self.load_optimizer_slots(slots, only=("average",))
            self._ls_pending = False
            self.step_count = it
            if self.model.optimizer is not None:
                self.model.optimizer.iterations = self.step_count
            ls = self.model.loaded_extras.get("loss_scale/current_loss_scale")
            opt = self.model.optimizer
            if ls is not None and opt is not None and opt.dynamic_loss_scale:   # a resumed mixed_float16 run keeps its scale
                good = self.model.loaded_extras.get("loss_scale/good_steps")
                self.loss_scale = dict(scale=float(ls), good=int(good) if good is not None else 0,
                                       growth_steps=int(opt.loss_scale_growth_steps), skipped=False)
            man = self.model.loaded_extras.get("loss/moving_average_normalizer")
            loss = self.model.loss
            if man is not None and loss is not None and loss.use_moving_average_normalizer:
                # a file without the key leaves the state as it is (0.0 in a fresh engine, the reference's initial value)
                loss.moving_average_normalizer = torch.from_numpy(
                    np.asarray(man, dtype=np.float32).reshape(1).copy()).to(self.dev)

    def store_to_model(self, use_ema=False):
        """flat arenas -> model.variables (executor.assign_moving_averaged_weights when use_ema)."""
        v = self.model.variables
        src = self.E if use_ema else self.P
        for k in self.train_names:
            v[k].copy_(self._keras_layout(k, src))
        for bn, d in self.bn_state.items():
            v[bn + "/moving_mean"].copy_(d["mm"])
            v[bn + "/moving_variance"].copy_(d["mv"])
        self.model._refresh()

    # ---- activations / gradients ---------------------------------------------------------------------
    def _alloc_tensors(self):
        B, dev = self.B, self.dev
        self.t, self.raw, self.grad = {}, {}, {}
        # frozen ResNet stage-1 bottleneck blocks as ONE launch each (retinanet/model/bottleneck.py): every layer of the
        # block frozen with its BatchNorm, nothing below it needs a gradient; their inner tensors get no buffer
        mine = {o["out"]: o for o in self.ops if "out" in o}
        blocks = fused_blocks(self.lib, self.g, B, lambda blk: not self.requires.get(blk["x"]) and all(
            o["out"] in mine and self._inference_form(mine[o["out"]]) and not self.requires.get(o["out"])
            for o in blk["ops"]))
        self._bneck_skip = {o["out"] for blk in blocks for o in blk["ops"]}
        inner = self._bneck_skip - {blk["name"] for blk in blocks}
        padded = padded_outputs(self.g)
        for name, (H, W, C, dt) in self.tensors.items():
            if name not in inner:
                self.t[name] = torch.empty((B, H, W, padded.get(name, C)), dtype=self._DT[dt], device=dev)
        self.bneck = {blk["ops"][0]["out"]: Bottleneck64(self.lib, self.g, blk, B, dev, self.launch_opts, self.t[blk["x"]],
                                                         self.t[blk["name"]]) for blk in blocks}
        self.stem_k, self.stem_pad, self.Hp, self.Wp, self.stem_in = stem_input(self.tensors, self._stem_op(), B, self.h16,
                                                                                dev)
        for op in self.ops:
            if op["op"] in ("conv", "stem", "dwconv") and (self._bn_trainable(op) or self._bn_apart(op)):
                self.raw[op["out"]] = torch.empty_like(self.t[op["out"]])
        # squeeze-excite: saved forward state per trainable op + one shared workspace (a frozen one keeps no state)
        self.se_state = {}
        se_bytes = 0
        for op in self.ops:
            if op["op"] == "se":
                nb = self.lib.rn_se_workspace_bytes(B, self.g.ses[op["se"]]["C"])
                if self._se_trainable(op):
                    self.se_state[op["out"]] = torch.empty((nb,), dtype=torch.uint8, device=dev)
                se_bytes = max(se_bytes, nb)
        self.se_ws = torch.empty((max(se_bytes, 16),), dtype=torch.uint8, device=dev)
        # balance features runs out of place in training (its backward needs the inputs)
        self.bal_out = {}
        for op in self.ops:
            if op["op"] == "balance":
                for n in op["tensors"]:
                    self.bal_out[n] = torch.empty_like(self.t[n])
        # gradient buffers (bf16) for every tensor that needs one
        need = set()
        for op in self.ops:
            if op["op"] in ("conv", "dwconv", "se") and self.requires.get(op["out"]):
                need.add(op["out"])
                for i in [op["inp"]] + ([op["residual"]] if op.get("residual") else []):
                    if self.requires.get(i):
                        need.add(i)
            elif op["op"] in ("maxpool",) and self.requires.get(op["out"]):
                need.add(op["out"])
                if self.requires.get(op["inp"]):
                    need.add(op["inp"])
            elif op["op"] == "topdown":
                for n in op["ins"] + op["outs"]:
                    if self.requires.get(n):
                        need.add(n)
        for n in need:
            H, W, C, _ = self.tensors[n]
            self.grad[n] = torch.zeros((B, H, W, C), dtype=self.h16, device=dev)
        for n, t in self.bal_out.items():
            if self.requires.get(n):
                self.grad["bal:" + n] = torch.zeros_like(t)
        self.bn_state = {}
        for op in self.ops:
            if op["op"] in ("conv", "stem", "dwconv") and self._bn_trainable(op):
                bn = op["bn"]
                self.bn_state[bn] = {"mm": self.model.variables[bn + "/moving_mean"].to(dev, torch.float32).clone(),
                                     "mv": self.model.variables[bn + "/moving_variance"].to(dev, torch.float32).clone()}

    def _fold_frozen(self):
        """inference-mode scale/shift + packed weights for frozen conv / depthwise (+BN) and squeeze-excite layers, and
        the data-gradient weight packs of those that hand a gradient down (in place after the first call)."""
        for op in self.ops:
            if op["op"] in ("conv", "stem") and not self._conv_trainable(op) and op["out"] not in self._bneck_skip:
                self.folded.load(self.model.variables, op)
            elif op["op"] == "dwconv" and not self._conv_trainable(op):
                self.folded.load_dw(self.model.variables, op)
            elif op["op"] == "se" and not self._se_trainable(op):
                self.folded.load_se(self.model.variables, op)
            elif op["op"] == "topdown" and op.get("fusion"):   # frozen fusion weights: f32 copies at stable addresses
                for name in (n for pair in op["fusion_vars"] for n in pair if n in self.frozen):
                    self.folded.stable(name, self.model.variables[name].to(self.dev, torch.float32).reshape(-1).clone())
        for fb in self.bneck.values():
            fb.load(self.model.variables, self.eps)
        self._fill_frozen_bn()
        self._pack_frozen_dgrad_weights()
        self._frozen_folded = True

    def _pack_frozen_dgrad_weights(self):
        """The data-gradient weight layouts of frozen layers (rn_pack_conv_weight_dgrad_batch, rn_pack_depthwise_weight_flip)
        are constants: packed here, when weights are loaded, from f32 copies of the model's variables in the compute
        layout — frozen variables have no slice of the arenas — and never by refresh_dgrad_weights."""
        lib, st, v = self.lib, _C.current_stream(), self.model.variables
        if self.frozen_dgrad_packs:
            arr = (_C.DgradPack * len(self.frozen_dgrad_packs))()
            masters = []
            for i, (kvar, k, cin, cout, cw, buf, mode) in enumerate(self.frozen_dgrad_packs):
                masters.append(_hwio_to_ohwi(v[kvar].to(self.dev, torch.float32)))
                arr[i].w_ohwi, arr[i].w_packed = masters[-1].data_ptr(), buf.data_ptr()
                arr[i].R, arr[i].S, arr[i].Cin, arr[i].Cout, arr[i].Cout_pad, arr[i].pad_ = k, k, cin, cout, cw, mode
            _C.check(lib.rn_pack_conv_weight_dgrad_batch(arr, len(self.frozen_dgrad_packs), st), "pack dgrad (frozen)")
        for (kvar, k, C, buf) in self.frozen_dw_flip_packs:
            w = v[kvar].to(self.dev, torch.float32).reshape(k * k, C).contiguous()
            _C.check(lib.rn_pack_depthwise_weight_flip(w.data_ptr(), k, C, buf.data_ptr(), st), "pack dw flip (frozen)")

    def _fill_frozen_bn(self, groups=None):
        """(scale, shift) of the frozen BatchNorm layers under trainable convs, from the model's moving statistics by the
        inference engine's arithmetic (forward.fold_bn), into fwd[2C..4C) of their rn_bn_problem segments: constant until
        weights are loaded again.  The mean / invstd rows stay zero: nothing reads them."""
        for grp in (getattr(self, "bn_groups", {}).values() if groups is None else groups):
            if not grp.frozen:
                continue
            off = 0
            for op in grp.ops:
                C = self.tensors[op["out"]][2]
                scale, shift, _ = fold_bn(self.model.variables, op["bn"], None, self.eps, self.dev)
                grp.fwd[4 * off + 2 * C:4 * off + 3 * C].copy_(scale)
                grp.fwd[4 * off + 3 * C:4 * off + 4 * C].copy_(shift)
                off += C

    # ---- helpers to build launches ---------------------------------------------------------------------
    def _conv_meta(self, p):
        """(ALGORITHMIC FLOPs, algorithmic HBM bytes, kernel variant or None) of a launch — SURVEY 8(d): FLOPs =
        2 * Ho*Wo*k*k*Cin*Cout of the LAYER per image (a data-gradient launch counts its layer's forward MACs, not the
        zero-upsampled or channel-padded GEMM it executes; split-bf16 weight planes count once); bytes = every input
        pixel read once + every output written once (+ residual read) + weights.  Variants bench.py tracks: the
        256x256x32 kernels and the 128x128x64 kernel, bf16 output."""
        osz = 4 if p.out_dtype == _C.RN_DT_F32 else 2
        dom = True
        for i in range(p.num_segments):
            s = p.seg[i]
            dom = dom and s.Cout > 64 and s.Cin % 64 == 0 and p.out_dtype == _C.RN_DT_BF16
        if id(p) in self._algo:
            flops, byts = self._algo[id(p)]
        else:
            flops = byts = 0
            for i in range(p.num_segments):
                s = p.seg[i]
                flops += 2 * s.N * s.Ho * s.Wo * p.R * p.S * s.Cin * s.Cout
                byts += 2 * s.N * s.H * s.W * s.pix_stride + osz * s.N * s.Ho * s.Wo * s.Cout + 2 * p.R * p.S * s.Cin * s.Cout
                if s.residual:
                    byts += 2 * s.N * s.Ho * s.Wo * s.Cout
        # one name per device symbol, so that a bench line and a rocprof kernel-stats row can be matched
        variant = None
        kid = self.lib.rn_conv_kernel_id(ctypes.byref(p))
        has_res = any(p.seg[i].residual for i in range(p.num_segments))
        bnb = bool(p.seg[0].bn_bwd_y)   # the BN_BWD variants (stage 1 of a BatchNorm backward reduction in the epilogue)
        tmpl = (f"<{'true' if p.out_dtype == _C.RN_DT_F32 else 'false'}, {'true' if has_res else 'false'}, "
                f"{'true' if bnb else 'false'}>")
        # (device symbols: conv_halo_kernel<f32 out, residual, BN_BWD, SPLIT, waves along the pixels>)
        if kid == 2:
            variant = "conv_halo_kernel" + tmpl[:-1] + ", false, 2> (256x256x32, 3x3 halo patch)"
        elif kid == 3:     # the same kernel template with 4 x 2 waves: 512 x 128 tiles (64 < Cout <= 128)
            variant = "conv_halo_kernel" + tmpl[:-1] + ", false, 4> (512x128x32, 3x3 halo patch)"
        elif kid == 1:
            variant = "conv_big_kernel" + tmpl + " (256x256x32)"
        elif dom:
            variant = "conv_fwd_kernel<128,128,64,bf16>"
        return flops, byts, variant

    def _timed(self, launch, *sinks):
        """launch() between two timing events on the current stream (bench.py's profiles): (e0, e1, *row) goes to every
        (list, row) of `sinks` whose list is not None"""
        cur = torch.cuda.current_stream(self.dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        launch()
        e1.record(cur)
        for lst, row in sinks:
            if lst is not None:
                lst.append((e0, e1) + row)

    def _launch_conv(self, p, st, what):
        """All implicit-GEMM launches (forward and dgrad) go through here so bench.py can bracket the
        dominant kernel variant with HIP events on the launch stream."""
        prof, lprof = self.conv_profile, self.layer_profile
        if prof is not None or lprof is not None:
            flops, byts, variant = self._conv_meta(p)
            if variant or lprof is not None:
                lrow = None
                if lprof is not None:
                    kid = self.lib.rn_conv_kernel_id(ctypes.byref(p))
                    kname = variant or ("conv_fwd_kernel (128-row tiles)" if kid == 0 else f"kernel id {kid}")
                    lrow = (self._launch_names.get(id(p), what), flops, byts, kname)
                self._timed(lambda: _C.check(self.lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), st), what),
                            (prof if variant else None, (flops, byts, variant)), (lprof, lrow))
                return
        _C.check(self.lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), st), what)

    def _weight_ptr(self, cname):
        """compute copy of the kernel of a live conv"""
        if cname in self.fwd_pack_of:
            return self.fwd_pack_of[cname].data_ptr()
        if cname in self.split_pack_of:
            return self.split_pack_of[cname].data_ptr()
        return self.Pbf.data_ptr() + 2 * self.bf_off[cname]

    def _f32_terms(self, layer):
        """bf16 weight planes of the dtype=float32 conv `layer` in THIS engine's forward pass: the narrow (pair-form)
        layers always carry both planes, the wide one `wide_pred_terms`"""
        if _C.PRED_W_TERMS <= 1:
            return 1
        return _C.PRED_W_TERMS if self.folded.w_pair(layer) else self.wide_pred_terms

    def _group_ops(self, kind, grp):
        """The ops of one grouped launch, in graph order.  (The one group that mixes K depths — the FPN lateral 1x1 convs with
        512 / 1024 / 2048 input channels — is balanced inside rn_conv2d_nhwc_fwd: tiles numbered deepest segment first and
        dealt to the workgroups round-robin; sorting the list here alone made that launch slower)"""
        return [o for o in self.ops if o["op"] == kind and o.get("group") == grp]

    def _conv_problem(self, ops, dst_of, raw_mode):
        """forward conv launch over `ops`; raw_mode: write pre-BN output (+bias) without activation."""
        p = conv_problem(self.g, ops, self.B, self.launch_opts, self.splitk_ws, lambda o: self._src(o["inp"]), dst_of,
                         self.folded.pixel_pair, _C.RN_ACT_NONE if raw_mode else None)
        for i, op in enumerate(ops):
            s = p.seg[i]
            if not self._conv_trainable(op):
                self.folded.fill(s, op, self.t)
                if raw_mode:     # frozen conv in front of a BatchNorm step (_bn_apart): weights and bias only
                    s.scale = s.shift = s.residual = None
            else:                # live conv: raw pre-BN output, or without BN (prediction convs)
                s.w = self._weight_ptr(op["conv"])
                s.bias = self._pview(op["conv"] + "/bias").data_ptr() if self.g.convs[op["conv"]]["bias"] else None
                if not raw_mode:
                    s.residual = self.t[op["residual"]].data_ptr() if op.get("residual") else None
                s.w_terms = self._f32_terms(op["conv"]) if op["conv"] in self.split_pack_of and op["conv"] not in self.pair_packs else 1
                s.w_pair = 1 if op["conv"] in self.pair_packs else 0
            if self.folded.pixel_pair(op):      # algorithmic work: the layer's own
                c, x, y = self.g.convs[op["conv"]], self._src(op["inp"]), dst_of(op)
                self._algo[id(p)] = (2 * self.B * y.shape[1] * y.shape[2] * 9 * c["cin"] * c["cout"],
                                     2 * x.numel() + 2 * y.numel() + 2 * 9 * c["cin"] * c["cout"])
        self._keep.append(p)
        self.conv_launches.append((conv_launch_name("fwd:", ops, {n for n, _ in self.conv_launches}), p))
        return p

    def _dw_problem(self, ops, dst_of, folded=False):
        """forward depthwise launch over `ops` writing the raw (pre-BN) or final output; bf16 weights are
        the plain-cast copies of the [k*k][C] masters, those of frozen layers the packed copies of _fold_frozen.
        folded: frozen layers in inference form, BatchNorm and activation in the epilogue."""
        live = self._conv_trainable(ops[0])
        p = dw_problem(self.g, ops, self.B, lambda o: self._src(o["inp"]), dst_of,
                       (lambda o: self.Pbf.data_ptr() + 2 * self.bf_off["dw:" + o["dw"]]) if live else
                       (lambda o: self.folded.packed[o["dw"]].data_ptr()),
                       _C.ACT_IDS[ops[0]["act"]] if folded else _C.RN_ACT_NONE)
        if folded:
            for i, op in enumerate(ops):
                self.folded.fill_dw(p.seg[i], op)
        self._keep.append(p)
        return p

    def _bn_pass(self, kind, pb, fn):
        """BatchNorm elementwise / reduction passes (HBM-bound): bench.py brackets them with events on the launch stream.
        Algorithmic bytes: apply = read y + write z (+ residual); bwd_reduce = read y + dz (+ z for the residual
        layers' gate); bwd_apply = the same reads + write dy (+ dres, + its old value when accumulating); frozen_bwd =
        read dz + the gate source rn_bn_frozen_bwd actually reads (the bits, else z behind a relu / relu6 residual add, y
        for the other relu / relu6 / swish layers + the residual re-read of swish, nothing without an activation) + write
        dy (+ dres as for bwd_apply)."""
        prof = self.hbm_profile
        if prof is None or (kind == "bn_bwd_reduce" and pb.seg[0].ext_chunks_bwd > 0):   # only the final pass is left
            return fn()
        byts = 0
        for i in range(pb.num_segments):
            s = pb.seg[i]
            n = int(s.P) * int(s.C) * 2
            gate = (n // 16 if s.act_mask else n) if (s.residual and pb.act) else 0   # z, or its one-bit gate
            if kind == "bn_frozen_bwd":
                relu = pb.act in (_C.ACT_IDS["relu"], _C.ACT_IDS["relu6"])
                if relu and all(pb.seg[j].act_mask for j in range(pb.num_segments)):
                    gate = n // 16
                elif relu:
                    gate = n
                else:
                    gate = (n * (2 if s.residual else 1)) if pb.act else 0
                byts += n + gate + n * (1 + ((2 if s.dres_accumulate else 1) if s.dres else 0))
            elif kind == "bn_apply":
                byts += n * (3 if s.residual else 2) + (n // 16 if s.act_mask else 0)
            elif kind == "bn_bwd_reduce":
                byts += n * 2 + gate
            else:
                byts += n * 2 + gate + n * (1 + ((2 if s.dres_accumulate else 1) if s.dres else 0))
        self._timed(fn, (prof, (kind, byts)))

    def _bn_stats_finalize(self, prb, ws, sums, st):
        """Batch statistics -> (mean, invstd, scale, shift) + moving statistics.  One replica: the final reduction
        kernel also finalizes; SyncBN: the [2][C] sums are all-reduced between the two."""
        lib = self.lib
        if not self.sync_bn:
            _C.check(lib.rn_bn_stats_finalize(prb, _C.ptr(ws), ws.numel(), st), "rn_bn_stats_finalize")
            return
        _C.check(lib.rn_bn_stats(prb, _C.ptr(ws), ws.numel(), st), "rn_bn_stats")
        self.small.merge_stats(sums)
        _C.check(lib.rn_bn_finalize(prb, st), "rn_bn_finalize")

    def _bn_problem(self, ops, conv_problem=None):
        """BatchNorm problem over `ops` and its buffers (BnGroup).  With `conv_problem` (the launch that produces the raw outputs): the forward
        statistics' stage-1 partial sums are written by the conv epilogue (rn_conv_segment.bn_partial, one row per
        128 output pixels) and rn_bn_stats only does the final ordered reduction.
        A BatchNorm in inference mode (_bn_apart) gets the same problem without anything the statistics, the
        reductions or the gamma / beta gradients touch: y, z, residual, dz, dy, the gate bits and the constant fwd table —
        and without dy and the gate bits where nothing below the layer needs a gradient (the frozen project conv of a
        drop_connect block: only its forward step runs)."""
        frozen = self._bn_apart(ops[0])
        p = _C.BnProblem()
        p.num_segments = len(ops)
        p.act = _C.ACT_IDS[ops[0]["act"]]
        p.bessel = 0 if self.sync_bn else 1
        p.eps, p.momentum, p.count_scale = self.eps, self.momentum_bn, float(self.world if self.sync_bn else 1)
        csum = sum(self.tensors[o["out"]][2] for o in ops)
        sums = bsums = None
        if not frozen:
            sums = torch.zeros((2 * csum + 1,), dtype=torch.float32, device=self.dev)   # + the slot C2 rides in
            bsums = torch.zeros((2 * csum,), dtype=torch.float32, device=self.dev)
        fwd = torch.zeros((4 * csum,), dtype=torch.float32, device=self.dev)
        off = 0
        dys = []
        for i, op in enumerate(ops):
            C = self.tensors[op["out"]][2]
            bn = op["bn"]
            y, z = self.raw[op["out"]], self.t[op["out"]]
            backward = bool(self.requires.get(op["out"]))    # (always, but for a frozen layer above nothing that trains)
            dy = torch.empty_like(y) if backward else None
            dys.append(dy)
            s = p.seg[i]
            s.y, s.z, s.dy = y.data_ptr(), z.data_ptr(), dy.data_ptr() if backward else None
            s.residual = self.t[op["residual"]].data_ptr() if op.get("residual") else None
            s.dz = self.grad[op["out"]].data_ptr() if op["out"] in self.grad else None
            s.dres = None
            s.fwd = fwd.data_ptr() + 4 * 4 * off
            if not frozen:
                s.sums = sums.data_ptr() + 4 * 2 * off
                s.bsums = bsums.data_ptr() + 4 * 2 * off
                s.gamma = self._pview(bn + "/gamma").data_ptr()
                s.beta = self._pview(bn + "/beta").data_ptr()
                s.moving_mean = self.bn_state[bn]["mm"].data_ptr()
                s.moving_var = self.bn_state[bn]["mv"].data_ptr()
                s.dgamma = self._pview(bn + "/gamma", self.G).data_ptr()
                s.dbeta = self._pview(bn + "/beta", self.G).data_ptr()
            s.P, s.C, s.dres_accumulate = y.shape[0] * y.shape[1] * y.shape[2], C, 0
            if (s.residual or frozen) and op["act"] in ("relu", "relu6") and backward:
                # relu behind the residual add: the forward stores the gate as one bit per element, the two backward
                # passes read P*C/8 bytes instead of z (rn_bn_segment.act_mask).  Every relu / relu6 layer of a frozen
                # BatchNorm: rn_bn_frozen_bwd then reads the bits instead of y or z
                mk = torch.empty((int(s.P) * C // 8,), dtype=torch.uint8, device=self.dev)
                self._keep.append(mk)
                s.act_mask = mk.data_ptr()
            if op.get("survival") is not None and self.drop_connect:
                if self.dc_all is None:     # one [blocks, B] tensor so that a step draws every factor at once
                    nsurv = sum(1 for o in self.ops if o.get("survival") is not None)
                    self.dc_all = torch.ones((nsurv, self.B), dtype=torch.float32, device=self.dev)
                    self.dc_p = torch.ones((nsurv, 1), dtype=torch.float32, device=self.dev)
                j = len(self.dc_masks)
                m = self.dc_all[j]
                self.dc_p[j, 0] = float(op["survival"])
                self.dc_masks[op["out"]] = (m, float(op["survival"]))
                s.sample_scale, s.rows_per_sample = m.data_ptr(), y.shape[1] * y.shape[2]
            off += C
        if frozen:
            grp = BnGroup(p, None, None, None, dys, ops, fwd, True)
            self._fill_frozen_bn([grp])
            self._keep += [p, fwd] + [dy for dy in dys if dy is not None]
            return grp
        fused = conv_problem is not None and self.fuse_bn_stats and conv_problem.out_dtype == _C.RN_DT_BF16
        if fused:
            for i in range(len(ops)):   # one row of partial sums per 128 output pixels of the kernel the dispatcher will run
                p.seg[i].ext_chunks = self.lib.rn_conv_bn_row_blocks(ctypes.byref(conv_problem), i)
        # (zeros: the ticket counters in the workspace tail start at zero, rnet_hip.h: rn_bn_workspace_bytes)
        ws = torch.zeros((max(self.lib.rn_bn_workspace_bytes(ctypes.byref(p)), 256),), dtype=torch.uint8,
                         device=self.dev)
        if fused:
            for i in range(len(ops)):
                conv_problem.seg[i].bn_partial = ws.data_ptr() + self.lib.rn_bn_partial_offset_bytes(ctypes.byref(p), i)
        self._keep += [p, sums, bsums, fwd, ws] + dys
        return BnGroup(p, sums, bsums, ws, dys, ops, fwd)

    # ---- forward --------------------------------------------------------------------------------------
    def _launch_ops(self, op, done):
        """The ops of the launch that conv / depthwise `op` belongs to: the op itself, or its whole group when `op` is the
        first of the group to turn up (`done`: the groups seen so far); [] when the group's launch was already built."""
        grp = op.get("group")
        if grp is None:
            return [op]
        if (op["op"], grp) in done:
            return []
        done.add((op["op"], grp))
        return self._group_ops(op["op"], grp)

    def _launch_ops_bn(self, op, done):
        """(_launch_ops(op, done), whether the launch's BatchNorm trains): one launch has one BatchNorm form"""
        ops = self._launch_ops(op, done)
        live_bn = bool(ops) and bool(self._bn_trainable(ops[0]))
        if any(bool(self._bn_trainable(o)) != live_bn for o in ops):
            raise NotImplementedError("a conv group mixes frozen and live BatchNorm")
        if any(self._conv_trainable(o) != self._conv_trainable(ops[0]) for o in ops):
            raise NotImplementedError(f"the {op['op']} group {op.get('group')} mixes frozen and live kernels: one launch "
                                      "has one form, and no freeze pattern splits a group")
        return ops, live_bn

    def _bn_train_step(self, launch, ops, conv_problem=None):
        """Forward step of live convs with a BatchNorm: launch(st) writes the raw outputs -> batch statistics and
        finalize (live BatchNorm only) -> rn_bn_apply (bracketed for bench.py's hbm_profile); registers the launch's
        BnGroup."""
        grp = self.bn_groups[ops[0]["out"]] = self._bn_problem(ops, conv_problem)
        lib, pb, prb = self.lib, grp.problem, ctypes.byref(grp.problem)

        def run(st):
            launch(st)
            if not grp.frozen:   # (frozen: scale / shift are the constants _fill_frozen_bn wrote)
                self._bn_stats_finalize(prb, grp.ws, grp.sums, st)
            self._bn_pass("bn_apply", pb, lambda: _C.check(lib.rn_bn_apply(prb, st), "rn_bn_apply"))
        return run

    def _build_forward(self):
        lib, B = self.lib, self.B
        self.fwd_steps = []
        self.fused_pools = set()   # MaxPool outputs written by rn_stem_conv_bn_relu_pool
        self.bn_groups = {}   # first op out -> BnGroup
        self.bal_src = {}     # tensor name -> balance output tensor (consumers read the balanced copy)
        done = set()
        for op in self.ops:
            kind = op["op"]
            if kind == "stem":
                img, y = self.t["images"], self.t[op["out"]]
                H, W = img.shape[1], img.shape[2]
                cout = self.g.convs[op["conv"]]["cout"]
                pin = self.stem_in.data_ptr()
                self._images_ptr = img.data_ptr()   # forward() points this at the caller's batch when it can be read in place
                self.fwd_steps.append(lambda st, pin=pin, H=H, W=W: _C.check(
                    lib.rn_pack_image_nhwc4(self._images_ptr, B, H, W, self.stem_pad[0], self.stem_pad[1], self.Hp, self.Wp,
                                            pin, st), "rn_pack_image_nhwc4"))
                if self._conv_trainable(op):
                    p = stem_problem(self, self.raw[op["out"]], cout, self.stem_packed.data_ptr(), _C.RN_ACT_NONE)
                    self._keep.append(p)
                    self.fwd_steps.append(self._bn_train_step(lambda st, p=p: self._launch_conv(p, st, "stem(train)"), [op]))
                    continue
                sc, sh, _ = self.folded.fold[op["out"]]
                p = stem_problem(self, y, cout, self.folded.packed[op["conv"]].data_ptr(), _C.ACT_IDS[op["act"]],
                                 sc.data_ptr(), sh.data_ptr())
                self._keep.append(p)
                pool = stem_pool_partner(self.g, op, self.readers)
                if pool is not None and not self.requires.get(op["out"]):
                    # frozen stem (`resnet_initial`): conv + folded BatchNorm + relu + MaxPool in one launch
                    self.fused_pools.add(pool["out"])
                    self.fwd_steps.append(stem_pool_step(lib, p, pool, self.t[pool["out"]]))
                else:
                    self.fwd_steps.append(lambda st, p=p: self._launch_conv(p, st, "stem"))
            elif kind == "conv" and op["out"] in self._bneck_skip:
                fb = self.bneck.get(op["out"])
                if fb is not None:                 # the block's first op in graph order carries the launch
                    def run_block(st, fb=fb):
                        lprof = self.layer_profile
                        if lprof is None:
                            fb.launch(st)
                            return
                        self._timed(lambda: fb.launch(st),
                                    (lprof, ("fwd:" + fb.name, fb.flops, fb.bytes, "bneck64_kernel (one launch per block)")))
                    self.fwd_steps.append(run_block)
            elif kind == "conv":
                ops, live_bn = self._launch_ops_bn(op, done)
                if not ops:
                    continue
                if live_bn or self._bn_apart(ops[0]):   # (BatchNorm in inference mode: no bn_partial epilogue in the conv)
                    pc = self._conv_problem(ops, lambda o: self.raw[o["out"]], raw_mode=True)
                    self.fwd_steps.append(self._bn_train_step(lambda st, pc=pc: self._launch_conv(pc, st, "conv(train)"),
                                                              ops, conv_problem=pc if live_bn else None))
                else:
                    for sub in split_by_depth(self.g, ops):
                        pc = self._conv_problem(sub, lambda o: self.t[o["out"]], raw_mode=False)
                        self.fwd_steps.append(lambda st, pc=pc: self._launch_conv(pc, st, "conv"))
            elif kind == "dwconv":
                ops, live_bn = self._launch_ops_bn(op, done)
                if not ops:
                    continue
                live_bn = live_bn or self._bn_apart(ops[0])   # either way: raw output, then the BatchNorm step
                # a frozen layer that hands no gradient down: BatchNorm and activation in the epilogue, as when serving
                folded = not live_bn and not self._conv_trainable(ops[0]) and not self._passes_gradient(ops[0])
                pd = self._dw_problem(ops, (lambda o: self.raw[o["out"]]) if live_bn else (lambda o: self.t[o["out"]]),
                                      folded=folded)
                self.dw_launches.append(("dw:" + (ops[0].get("group") or ops[0]["out"]), "fwd", pd, []))
                prd = ctypes.byref(pd)
                if live_bn:
                    self.fwd_steps.append(self._bn_train_step(
                        lambda st, prd=prd: _C.check(lib.rn_depthwise_conv2d_nhwc_fwd(prd, st), "depthwise(train)"), ops))
                else:
                    if not folded and ops[0].get("act") not in (None, "none"):
                        raise NotImplementedError("depthwise conv with an activation but no BatchNorm")
                    self.fwd_steps.append(lambda st, prd=prd: _C.check(lib.rn_depthwise_conv2d_nhwc_fwd(prd, st),
                                                                       "depthwise"))
            elif kind == "se" and not self._se_trainable(op):
                # frozen, nothing below it trains (_analyse): the serving engine's in-place launch — no second tensor, no
                # saved state; the out-of-place forward would write both only for a backward that never runs
                x, se = self.t[op["inp"]], self.g.ses[op["se"]]
                a = self.folded.se_args(op, x, B, self.se_ws)
                self.se_launches.append(("se:" + op["out"], "fwd", B, x.shape[1] * x.shape[2], se["C"], se["se"]))
                self.fwd_steps.append(lambda st, a=a: _C.check(lib.rn_squeeze_excite_inplace(*a, st),
                                                               "rn_squeeze_excite_inplace"))
            elif kind == "se":
                x, y = self.t[op["inp"]], self.t[op["out"]]
                name, se = op["se"], self.g.ses[op["se"]]
                state = self.se_state[op["out"]]
                a = (x.data_ptr(), y.data_ptr(), B, x.shape[1] * x.shape[2], se["C"],
                     self.Pbf.data_ptr() + 2 * self.bf_off[name + ":w1"], self._pview(name + "/conv2d/bias").data_ptr(),
                     self.Pbf.data_ptr() + 2 * self.bf_off[name + ":w2"], self._pview(name + "/conv2d_1/bias").data_ptr(),
                     se["se"], state.data_ptr(), state.numel())
                self.se_launches.append(("se:" + op["out"], "fwd", B, x.shape[1] * x.shape[2], se["C"], se["se"]))
                self.fwd_steps.append(lambda st, a=a: _C.check(lib.rn_squeeze_excite_fwd(*a, st), "rn_squeeze_excite_fwd"))
            elif kind == "maxpool":
                if op["out"] in self.fused_pools:   # written by the fused stem launch
                    continue
                self.fwd_steps.append(maxpool_step(lib, op, self.t, B))
            elif kind == "topdown":
                fusion = None
                if op.get("fusion"):   # live weights are read where they live: the flat parameter arena
                    fusion = self.fusion_state[id(op)] = FusionState(
                        lib, op, self.t[op["ins"][0]].shape[3], self.dev,
                        lambda n: self._pview(n).data_ptr() if n in self.p_off else self.folded.packed[n].data_ptr())
                self.fwd_steps.append(topdown_step(lib, op, self.t, B, self._keep, fusion))
            elif kind == "balance":
                ts = [self.t[n] for n in op["tensors"]]
                outs = [self.bal_out[n] for n in op["tensors"]]
                for n in op["tensors"]:
                    self.bal_src[n] = self.bal_out[n]
                pin, pout = _C.ptr_array(ts), _C.ptr_array(outs)
                self.bal_avg = torch.empty_like(ts[op["mid"]])
                self._keep += [pin, pout]
                a = (pin, pout, len(ts), op["mid"], B, ts[0].shape[1], ts[0].shape[2], ts[0].shape[3],
                     self.bal_avg.data_ptr())
                self.fwd_steps.append(lambda st, a=a: _C.check(lib.rn_balance_features(*a, st), "rn_balance_features"))
        self.outputs = {k: {lv: output_view(self.t[n], self.tensors[n][2]) for lv, n in d.items()}
                        for k, d in self.g.outputs.items()}
        self._bn_of_tensor = {o["out"]: (grp.problem, i, o, len(grp.ops))
                              for grp in self.bn_groups.values() for i, o in enumerate(grp.ops)}
        # the loss normaliser (C2) rides in the step's first SyncBN forward message: only a live BatchNorm sends one
        self.small.has_carrier = any(not grp.frozen for grp in self.bn_groups.values())

    def _src(self, name):
        return self.bal_src.get(name, self.t[name])

    def _zero_upsampled(self, dy, H, W, ups):
        """dy of a stride-2 layer with zeros between its pixels, at the layer input's H x W, for the stride-1 form of the
        data gradient to run on.  The rn_upsample_zero2x arguments that fill the buffer join `ups`, which _dgrad_step runs."""
        up = torch.empty((self.B, H, W, dy.shape[3]), dtype=self.h16, device=self.dev)
        self._keep.append(up)
        ups.append((dy.data_ptr(), up.data_ptr(), self.B, dy.shape[1], dy.shape[2], dy.shape[3], H, W))
        return up

    def _dgrad_step(self, ups, launch, post_op=None, post=(), what="dgrad"):
        """Data-gradient step: rn_upsample_zero2x over the argument tuples `ups` (_zero_upsampled), launch(st), then
        post_op = (library function, its name) over the argument tuples `post`.  launch(st) returns the library's status, or
        None where it has checked it itself (_launch_conv)."""
        lib = self.lib

        def dgrad(st):
            for u in ups:
                _C.check(lib.rn_upsample_zero2x(*u, st), "rn_upsample_zero2x")
            status = launch(st)
            if status:
                _C.check(status, what)
            for a in post:
                _C.check(post_op[0](*a, st), post_op[1])
        return BackwardStep(dgrad)

    # ---- backward ---------------------------------------------------------------------------------------
    def _build_backward(self):
        self.bwd_steps = []
        self.dgrad_packs = []     # (master offset, conv dims, packed buffer)
        self.dw_flip_packs = []   # (master offset, k, C, packed bf16 tap-reversed filter)
        plan, done = [], set()
        for op in self.ops:     # the forward launches; a group stands where its first op does
            if op["op"] in ("conv", "dwconv"):
                launch = self._launch_ops(op, done)
                if launch:
                    plan.append((op["op"], launch))
            elif op["op"] in self._backward_planners:
                plan.append((op["op"], op))
        # which tensor gradients get more than one contribution is decided here, by the order the steps are planned in
        self.joins = joins = GradientJoins(self.grad, self.bal_src)
        for kind, item in reversed(plan):
            self._backward_planners[kind](self, item, joins)
        # what the steps look up, static from here on
        self._launch_names = {id(q): n for n, q in self.conv_launches}
        # (a frozen prediction conv has no dy: such an engine serves forward() only)
        self._loss_dy = {k: {lv: self.dy_of[name] for lv, name in self.g.outputs[k].items() if name in self.dy_of}
                         for k in self.g.outputs}
        if self.dgrad_packs:
            arr = (_C.DgradPack * len(self.dgrad_packs))()
            for i, (mptr, k, cin, cout, cw, buf, mode) in enumerate(self.dgrad_packs):
                arr[i].w_ohwi, arr[i].w_packed = mptr, buf.data_ptr()
                arr[i].R, arr[i].S, arr[i].Cin, arr[i].Cout, arr[i].Cout_pad, arr[i].pad_ = k, k, cin, cout, cw, mode
            self._dgrad_pack_items = arr
        self._pack_frozen_dgrad_weights()    # (every later load re-enters it through _fold_frozen)

    def _plan_se_backward(self, op, joins):
        lib, B = self.lib, self.B
        if not self._se_trainable(op):    # (frozen: in place in the forward pass, nothing below it trains)
            return
        x, dy = self.t[op["inp"]], self.grad[op["out"]]
        dx = joins.sole(op["inp"], "se:" + op["out"])
        name, se = op["se"], self.g.ses[op["se"]]
        a = (x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, x.shape[1] * x.shape[2], se["C"],
             self.Pbf.data_ptr() + 2 * self.bf_off[name + ":w1"],
             self.Pbf.data_ptr() + 2 * self.bf_off[name + ":w2"], se["se"], self.se_state[op["out"]].data_ptr(),
             self._pview(name + "/conv2d/kernel", self.G).data_ptr(),
             self._pview(name + "/conv2d/bias", self.G).data_ptr(),
             self._pview(name + "/conv2d_1/kernel", self.G).data_ptr(),
             self._pview(name + "/conv2d_1/bias", self.G).data_ptr(), self.se_ws.data_ptr(), self.se_ws.numel())
        self.se_launches.append(("se:" + op["out"], "bwd", B, x.shape[1] * x.shape[2], se["C"], se["se"]))
        self.bwd_steps.append(BackwardStep(
            lambda st, a=a: _C.check(lib.rn_squeeze_excite_bwd(*a, st), "rn_squeeze_excite_bwd"),
            writes=[name + sfx for sfx in self._SE_VARS]))

    def _plan_maxpool_backward(self, op, joins):
        lib, B = self.lib, self.B
        if not self.requires.get(op["inp"]):
            return
        x, dy = self.t[op["inp"]], self.grad[op["out"]]
        dx, accumulate = joins.add(op["inp"], "maxpool:" + op["out"], balanced=False)
        a = (x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, x.shape[1], x.shape[2], x.shape[3], op["k"],
             op["stride"], op["pad_top"], op["pad_left"], dy.shape[1], dy.shape[2], int(accumulate))
        self.bwd_steps.append(BackwardStep(lambda st, a=a: _C.check(lib.rn_maxpool2d_nhwc_bwd(*a, st), "maxpool_bwd")))

    def _plan_stem_backward(self, op, joins):
        lib, B = self.lib, self.B
        if not self._conv_trainable(op):
            return
        # the BatchNorm step runs inside stem_bwd, ahead of the weight gradient (the live form's two passes were never rows
        # of hbm_profile)
        head = []
        dy = self._plan_bn_backward([op], joins, profiled=False, steps=head)[op["out"]]
        bn_bwd = head[0]
        c = self.g.convs[op["conv"]]
        pw = _C.WgradProblem()
        pw.opts = self.launch_opts
        k = self.stem_k
        pw.R, pw.S, pw.stride_h, pw.stride_w, pw.pad_top, pw.pad_left, pw.num_segments = k, 1, 2, 2, 0, 0, 1
        sg = pw.seg[0]
        sg.x, sg.dy = self.stem_in.data_ptr(), dy.data_ptr()
        sg.N, sg.H, sg.W, sg.Cin, sg.Ho, sg.Wo, sg.Cout = B, self.Hp, self.Wp, 32, dy.shape[1], dy.shape[2], c["cout"]
        sg.x_pix_stride = 4
        wsw = torch.empty((max(lib.rn_wgrad_workspace_bytes(ctypes.byref(pw)), 256),), dtype=torch.uint8,
                          device=self.dev)
        dwp = torch.zeros((c["cout"], k, 8, 4), dtype=torch.float32, device=self.dev)
        gview = self._pview(self._kvar(op), self.G).view(c["cout"], k, k, 3)
        self._keep += [pw, wsw, dwp]

        def stem_bwd(st, bn_bwd=bn_bwd.run):
            bn_bwd(st)
            _C.check(lib.rn_conv2d_nhwc_wgrad(ctypes.byref(pw), dwp.data_ptr(), 0.0, wsw.data_ptr(),
                                              wsw.numel(), st), "stem wgrad")
            gview.copy_(dwp[:, :, :k, :3])   # [co][r][8 taps x 4 ch] -> [co][r][s][c]
        self.bwd_steps.append(BackwardStep(stem_bwd, writes=[self._kvar(op)] + bn_bwd.writes))

    def _topdown_din(self, op, l, joins):
        """Gradient buffer of input l of top-down op `op`.  The level kernels overwrite it — except where the level passes
        through (the top one: outs[l] IS ins[l]): there dout and din are one buffer, which the step updates in place on top
        of what the readers of the output have written."""
        name = op["ins"][l]
        if name != op["outs"][l]:
            return joins.sole(name, "topdown")
        din, accumulate = joins.add(name, "topdown", balanced=False)
        if not accumulate:
            raise RuntimeError(f"top-down level {name} passes through, and no reader of it has written its gradient")
        return din

    def _plan_topdown_backward(self, op, joins):
        lib, B = self.lib, self.B
        L = len(op["ins"])
        if not any(self.requires.get(n) for n in op["outs"]):    # frozen inputs, frozen fusion weights: no backward
            return
        if op["act"] == "swish":
            # rn_fpn_topdown_bwd_level refuses it: swish' needs the sum in front of the activation, and the
            # forward pass keeps only its output
            raise NotImplementedError(f"backward of the top-down op {op['outs'][0]} .. {op['outs'][-1]} with "
                                      "activation 'swish' is not built (relu / relu6 / none are)")
        act = _C.ACT_IDS[op["act"]]
        if op.get("fusion"):
            self._plan_fused_topdown_backward(op, act, joins)
            return
        prev = None
        for l in range(L):
            dout = self.grad[op["outs"][l]]
            din = self._topdown_din(op, l, joins)
            outp = self.t[op["outs"][l]].data_ptr() if l < L - 1 else None
            a = (dout.data_ptr(), prev, outp, din.data_ptr(), B, dout.shape[1], dout.shape[2], dout.shape[3],
                 act if l < L - 1 else _C.RN_ACT_NONE)
            self.bwd_steps.append(BackwardStep(lambda st, a=a: _C.check(lib.rn_fpn_topdown_bwd_level(*a, st),
                                                                        "topdown_bwd")))
            prev = din.data_ptr()

    def _plan_balance_backward(self, op, joins):
        lib, B = self.lib, self.B
        names = op["tensors"]
        if not any(self.requires.get(n) for n in names):    # everything below BalanceFeatures is frozen
            return
        dout = [self.grad["bal:" + n] for n in names]
        ins = [self.t[n] for n in names]
        din = [joins.sole(n, "balance") for n in names]
        nsc = lib.rn_balance_features_bwd_scratch_bytes(len(names), op["mid"], B, ins[0].shape[1], ins[0].shape[2],
                                                        ins[0].shape[3])
        scratch = torch.empty((max(int(nsc), 256),), dtype=torch.uint8, device=self.dev)
        pd, pi, pn = _C.ptr_array(dout), _C.ptr_array(ins), _C.ptr_array(din)
        self._keep += [pd, pi, pn, scratch]
        a = (pd, pi, pn, self.bal_avg.data_ptr(), scratch.data_ptr(), scratch.numel(), len(names), op["mid"], B,
             ins[0].shape[1], ins[0].shape[2], ins[0].shape[3])
        self.bwd_steps.append(BackwardStep(lambda st, a=a: _C.check(lib.rn_balance_features_bwd(*a, st), "balance_bwd")))

    def _plan_fused_topdown_backward(self, op, act, joins):
        """Backward of a weighted top-down op, finest level first: per level one rn_fpn_fused_bwd_level (the gated gradient
        g overwrites dout — nothing reads dout afterwards —, din, stage 1 of the two weight-gradient sums) and one
        rn_fpn_fused_bwd_finalize that writes dw_lower / dw_upper into the gradient arena.  Both run on the main stream, in
        order, so the arena is complete before anything that follows the backward pass reads it; `writes` tells the
        bucketed all-reduce which variables the step completes."""
        lib, B, fus = self.lib, self.B, self.fusion_state[id(op)]
        L = len(op["ins"])
        prev_g = prev_coef = None
        for l in range(L):
            dout, din = self.grad[op["outs"][l]], self._topdown_din(op, l, joins)
            _, H, W, C = dout.shape
            if l == L - 1:
                a = (dout.data_ptr(), prev_g, prev_coef, None, None, None, None, None, din.data_ptr(), None, 0, B, H, W, C,
                     _C.RN_ACT_NONE)
                self.bwd_steps.append(BackwardStep(lambda st, a=a: _C.check(lib.rn_fpn_fused_bwd_level(*a, st),
                                                                            "fused_topdown_bwd")))
                break
            ws = torch.empty((lib.rn_fpn_fused_bwd_workspace_bytes(B, H, W, C),), dtype=torch.uint8, device=self.dev)
            coef = fus.coef[l].data_ptr()
            a = (dout.data_ptr(), prev_g, prev_coef, self.t[op["outs"][l]].data_ptr(), self.t[op["ins"][l]].data_ptr(),
                 self.t[op["outs"][l + 1]].data_ptr(), coef, dout.data_ptr(), din.data_ptr(), ws.data_ptr(), ws.numel(),
                 B, H, W, C, act)
            live = [n for n in fus.names[l] if n in self.p_off]
            # a frozen weight's gradient goes to a scratch nobody reads
            dw = [self._pview(n, self.G) if n in self.p_off else torch.empty_like(self.folded.packed[n])
                  for n in fus.names[l]]
            f = (ws.data_ptr(), ws.numel(), B, H, W, C, fus.w[l][0], fus.w[l][1], coef, fus.mode, None,
                 dw[0].data_ptr(), dw[1].data_ptr())
            self._keep += [ws, dw]

            def level(st, a=a, f=f, finalize=bool(live)):
                _C.check(lib.rn_fpn_fused_bwd_level(*a, st), "fused_topdown_bwd")
                if finalize:
                    _C.check(lib.rn_fpn_fused_bwd_finalize(*f, st), "fused_topdown_bwd_finalize")
            self.bwd_steps.append(BackwardStep(level, writes=live))
            prev_g, prev_coef = dout.data_ptr(), coef

    def set_wgrad_cap(self, on):
        """The CU cap of the weight-gradient launches (see _plan_wgrad) on / off: with the chip to themselves
        (bench.py's one-stream `exclusive` step) they run uncapped; the workspaces fit either split-K plan."""
        for p, cap in self._wgrad_capped:
            p.opts.wgrad_target_blocks = cap if on else 0

    @staticmethod
    def _wgrad_bytes(p):
        """algorithmic HBM bytes of a weight-gradient launch: x and dy read once, dW (f32) written once"""
        b = 0
        for i in range(p.num_segments):
            s = p.seg[i]
            b += 2 * s.N * s.H * s.W * s.Cin + 2 * s.N * s.Ho * s.Wo * s.Cout
        return b + 4 * p.R * p.S * p.seg[0].Cin * p.seg[0].Cout

    def _wgrad_kernel_name(self, p):
        return ("wgrad_kernel (128x128 per-tap tiles)", "wgrad_big_kernel (256x256 per-tap tiles)",
                "wgrad_halo_kernel")[max(self.lib.rn_wgrad_kernel_id(ctypes.byref(p)), 0)]

    def _wgrad_workspace(self, problems, size):
        """Split-K workspace of a weight-gradient launch over `problems`; size(): the library's byte count for their options
        as they stand.  It must fit the capped plan, the uncapped one (set_wgrad_cap(False) lifts the cap on a live engine)
        and, under RNET_AB_WORKSPACES=1, the other kernel families (tools/ab_step.py switches them between timed rounds)."""
        def largest(field, values):
            old = [getattr(p.opts, field) for p in problems]
            n = 0
            for v in values:
                for p in problems:
                    setattr(p.opts, field, v)
                n = max(n, size())
            for p, v in zip(problems, old):
                setattr(p.opts, field, v)
            return n
        nws = size()
        if any(p.opts.wgrad_target_blocks for p in problems):
            nws = max(nws, largest("wgrad_target_blocks", (0,)))
        if self._ab_workspaces:
            nws = max(nws, largest("wgrad_kernel", (1, 3)))
        return torch.empty((max(nws, 256),), dtype=torch.uint8, device=self.dev)

    def _wgrad_step(self, call, args, what, flops, byts, kname, lname, writes, item=None):
        """Side-stream step of one weight-gradient library call `call(*args, stream)`, bracketed with events on the stream
        it goes to (the side stream in the two-stream backward) while bench.py collects wgrad_profile / layer_profile."""
        def wgrad(st):
            prof, lprof = self.wgrad_profile, self.layer_profile
            if prof is None and lprof is None:
                _C.check(call(*args, st), what)
                return
            self._timed(lambda: _C.check(call(*args, st), what), (prof, (flops, kname)), (lprof, (lname, flops, byts, kname)))
        return BackwardStep(wgrad, side=True, writes=writes, wgrad=item)

    def _group_wgrad_steps(self):
        """Weight-gradient launches of layers with IDENTICAL geometry become one rn_conv2d_nhwc_wgrad_group call (the
        eight head-tower layers, the 3x3 layers of a ResNet stage: up to 8 per call), issued where the LAST of them
        stood in the backward order — nothing but the optimizer reads a weight gradient, and dy / the saved activation
        of the earlier layers are static buffers nobody writes again.  One launch over (layer, co tile, ci tile) tiles
        needs 1/n of the split-K pixel chunks per layer: every workgroup writes its whole 288 KB accumulator as a partial
        tile, ~75 MB per launch however small the layer.  RNET_WGRAD_GROUP=0 keeps one launch per layer."""
        lib = self.lib
        self.wgrad_groups = []
        if self._wgrad_group_mode == "0":
            return
        by_sig = {}
        for i, step in enumerate(self.bwd_steps):
            if step.wgrad is None:
                continue
            p = step.wgrad[0]
            sig = (p.R, p.S, p.stride_h, p.stride_w, p.pad_top, p.pad_left, p.num_segments, bytes(p.opts),
                   tuple((s.N, s.H, s.W, s.Cin, s.Ho, s.Wo, s.Cout, s.dy_pix_stride, s.x_pix_stride)
                         for s in (p.seg[k] for k in range(p.num_segments))),
                   # the auxiliary head's layers group among themselves: the other layers' groups stay what they are
                   # without the head, whatever width it is given
                   any(w.startswith("auxillary-head") for w in step.writes))
            by_sig.setdefault(sig, []).append(i)
        drop, replace = set(), {}
        for sig, idxs in by_sig.items():
            for lo in range(0, len(idxs), 8):
                grp = idxs[lo:lo + 8]
                if len(grp) < 2:
                    continue
                items = [self.bwd_steps[i].wgrad for i in grp]
                probs = [it[0] for it in items]
                arr = (ctypes.POINTER(_C.WgradProblem) * len(grp))(*[ctypes.pointer(p) for p in probs])
                if lib.rn_wgrad_group_fused(arr, len(grp)) != 1:
                    continue
                # Groups the halo kernel does not serve — the 1x1 layers of a ResNet stage, five / six of one geometry, which
                # rn_conv2d_nhwc_wgrad_group runs as segments of one partial-tile launch since round 6 — are NOT grouped by
                # default: same-box A/B (tools/probes/ab_env_r06.sh, profiles/r06_ab/wgrad_group_1x1.txt) 28.11 / 28.32 / 28.47
                # grouped against 28.10 / 28.14 / 28.22 ms per step.  A group is issued where its LAST layer stood, which
                # moves ~40 small launches' work to the end of the weight-gradient stream — the stream that already ends
                # 0.5 ms after the main one.  RNET_WGRAD_GROUP=all groups them (the library path stays tested).
                if self._wgrad_group_mode != "all" and lib.rn_wgrad_kernel_id(ctypes.byref(probs[0])) != 2:
                    continue
                ws = self._wgrad_workspace(probs, lambda: lib.rn_wgrad_group_workspace_bytes(arr, len(grp)))
                dws = _C.ptr_array([it[1] for it in items])
                wname = f"{self._wgrad_kernel_name(probs[0])} ({len(grp)} layers per launch) + wgrad_reduce_kernel"
                lname = "wgrad:" + "+".join(n[len("wgrad:"):] for n, q in self.wgrad_launches
                                            if any(q is p for p in probs))
                self._keep += [arr, dws, ws]
                old_ws = {id(it[2]) for it in items}
                self._keep = [k for k in self._keep if id(k) not in old_ws]      # the per-layer workspaces are not needed
                replace[grp[-1]] = self._wgrad_step(
                    lib.rn_conv2d_nhwc_wgrad_group, (arr, len(grp), dws, 0.0, ws.data_ptr(), ws.numel()),
                    "rn_conv2d_nhwc_wgrad_group", sum(it[3] for it in items), sum(self._wgrad_bytes(p) for p in probs),
                    wname, lname, [w for i in grp for w in self.bwd_steps[i].writes])
                drop.update(grp[:-1])
                self.wgrad_groups.append(probs)
        self.bwd_steps = [replace.get(i, step) for i, step in enumerate(self.bwd_steps) if i not in drop]

    def _bn_bwd_step(self, grp, ws, profiled=True):
        """BatchNorm backward of the layers of BnGroup `grp`: reduction (over the partials in `ws`) -> SyncBN all-reduce
        of the sums -> apply (dy).  profiled=False keeps the two passes out of bench.py's hbm_profile."""
        lib, pb, prb, bsums = self.lib, grp.problem, ctypes.byref(grp.problem), grp.bsums
        bracket = self._bn_pass if profiled else (lambda kind, pb, fn: fn())

        def run(st):
            bracket("bn_bwd_reduce", pb, lambda: _C.check(lib.rn_bn_bwd_reduce(prb, _C.ptr(ws), ws.numel(), st),
                                                           "rn_bn_bwd_reduce"))
            if self.sync_bn:
                self.small.all_reduce(bsums)
            bracket("bn_bwd_apply", pb, lambda: _C.check(lib.rn_bn_bwd_apply(prb, st), "rn_bn_bwd_apply"))
        return BackwardStep(run, writes=[op["bn"] + sfx for op in grp.ops for sfx in ("/gamma", "/beta")])

    def _bn_frozen_bwd_step(self, grp):
        """Backward of the frozen BatchNorm layers of BnGroup `grp`: one elementwise pass dz -> dy (+ dres).  No
        workspace, no SyncBN message, and no variable's gradient is completed by it."""
        lib, pb, prb = self.lib, grp.problem, ctypes.byref(grp.problem)

        def run(st):
            self._bn_pass("bn_frozen_bwd", pb, lambda: _C.check(lib.rn_bn_frozen_bwd(prb, st), "rn_bn_frozen_bwd"))
        return BackwardStep(run, writes=[])

    @staticmethod
    def _distinct_inputs(ops):
        """the ops whose input needs a gradient, split into launches whose segments read distinct inputs (they write
        distinct gradient buffers: both heads read the same pyramid level)"""
        launches = []
        for op in ops:
            for sub in launches:
                if all(o["inp"] != op["inp"] for o in sub):
                    sub.append(op)
                    break
            else:
                launches.append([op])
        return launches

    def _plan_bn_backward(self, ops, joins, *, profiled=True, steps=None):
        """BatchNorm head of the backward of the launch over `ops` (BnGroup bn_groups[ops[0]["out"]]): dz of every segment
        is the gradient at the layer's output, a residual input that needs a gradient gets it from the same pass (dres),
        and one frozen or live BatchNorm step joins `steps` (default: bwd_steps).  Returns {op out: dy}, the gradients at
        the conv outputs that the step writes."""
        grp = self.bn_groups[ops[0]["out"]]
        pb = grp.problem
        for i, op in enumerate(ops):
            s = pb.seg[i]
            s.dz = self.grad[op["out"]].data_ptr()
            if op.get("residual") and self.requires.get(op["residual"]):
                dres, accumulate = joins.add(op["residual"], "bn:" + ops[0]["out"], balanced=False)
                s.dres, s.dres_accumulate = dres.data_ptr(), int(accumulate)
        if grp.frozen:
            step = self._bn_frozen_bwd_step(grp)
        else:   # (ws: stage 1 already written there by the dgrad launch that produced dz)
            step = self._bn_bwd_step(grp, self.bn_bwd_ws.get(id(pb), grp.ws), profiled)
        (self.bwd_steps if steps is None else steps).append(step)
        return {op["out"]: grp.dys[i] for i, op in enumerate(ops)}

    def _plan_plain_dy(self, ops):
        """{op out: dy} of convs without a BatchNorm: the prediction convs' dy is the buffer the loss gradient is written to,
        the others' comes out of an rn_act_bwd step."""
        lib = self.lib
        dy_of = {}
        for op in ops:
            if op["out_dtype"] == "f32":      # prediction convs: loss gradient arrives in fp32
                shp = list(self.t[op["out"]].shape)
                shp[3] = (shp[3] + 63) // 64 * 64     # K dimension of the dgrad GEMM: pad 36/720 -> 64/768
                dyb = torch.zeros(shp, dtype=self.h16, device=self.dev)
                dy_of[op["out"]] = dyb
            else:
                if op["act"] == "swish":     # rn_act_bwd refuses it: swish' is no function of the stored output
                    raise NotImplementedError(f"backward of the conv op {op['out']} ({op['conv']}): activation "
                                              "'swish' without a BatchNorm in front is not built")
                dyb = torch.empty_like(self.t[op["out"]])
                dy_of[op["out"]] = dyb
                a = (self.grad[op["out"]].data_ptr(), self.t[op["out"]].data_ptr(), dyb.data_ptr(),
                     dyb.numel(), _C.ACT_IDS[op["act"]])
                self.bwd_steps.append(BackwardStep(lambda st, a=a: _C.check(lib.rn_act_bwd(*a, st), "rn_act_bwd")))
        self._keep += list(dy_of.values())
        return dy_of

    def _plan_wgrad(self, cname, cops, dy_of):
        """Weight gradient of conv layer `cname`, one launch over the ops `cops` that share it"""
        lib, B = self.lib, self.B
        c = self.g.convs[cname]
        kvar = c.get("kvar", cname + "/kernel")
        p = _C.WgradProblem()
        p.opts = self.launch_opts
        p.R = p.S = c["k"]
        p.stride_h = p.stride_w = c["stride"]
        p.pad_top = p.pad_left = cops[0]["pad"]
        p.num_segments = len(cops)
        # rn_conv2d_nhwc_wgrad takes Cout % 4 == 0: the auxiliary head's 9-channel prediction conv runs as 12 (dy's pad
        # channels are zero, so rows 9 - 11 of dw are) into a buffer of its own, the live rows are copied to the arena
        cout4 = -(-c["cout"] // 4) * 4
        for i, op in enumerate(cops):
            x, dy = self._src(op["inp"]), dy_of[op["out"]]
            s = p.seg[i]
            s.x, s.dy = x.data_ptr(), dy.data_ptr()
            s.N, s.H, s.W, s.Cin, s.Ho, s.Wo, s.Cout = B, x.shape[1], x.shape[2], c["cin"], dy.shape[1], dy.shape[2], cout4
            s.dy_pix_stride = dy.shape[3]
        # Two-stream backward: a weight-gradient launch is capped to ~2/3 of the CUs (rn_launch_opts.wgrad_target_blocks).
        # Its persistent workgroups own a CU for hundreds of microseconds; when they cover the whole chip every
        # main-stream launch — the critical path — queues behind them.  Measured in one process (tools/ab_step.py):
        # 31.40 -> 30.48 ms and 32.45 -> 31.34 ms per step on two boxes with 176 workgroups for the 256-wide kernels
        # and 256 (two per CU) for the 128-tile kernel; 128 / 192 is already slower again.  RNET_WGRAD_CUS=0: no cap.
        if self._wgrad_cap and not p.opts.wgrad_target_blocks:
            kid = lib.rn_wgrad_kernel_id(ctypes.byref(p))
            p.opts.wgrad_target_blocks = self._wgrad_cap[0] if kid in (1, 2) else self._wgrad_cap[1]
            self._wgrad_capped.append((p, int(p.opts.wgrad_target_blocks)))
        ws = self._wgrad_workspace([p], lambda: lib.rn_wgrad_workspace_bytes(ctypes.byref(p)))
        dw = self._pview(kvar, self.G)
        dw_live = None
        if cout4 != c["cout"]:
            dw_live, dw = dw, torch.zeros((cout4 * c["k"] * c["k"] * c["cin"],), dtype=torch.float32, device=self.dev)
            self._keep.append(dw)
        self._keep += [p, ws]
        self.wgrad_launches.append(("wgrad:" + cname, p))
        # algorithmic FLOPs of the layer's weight gradient: 2 * pixels * k*k * Cin * Cout over the segments
        flw = sum(2 * B * p.seg[i].Ho * p.seg[i].Wo * c["k"] * c["k"] * c["cin"] * c["cout"] for i in range(len(cops)))
        # (a layer with a buffer of its own stays out of _group_wgrad_steps' merge of same-shape layers)
        step = self._wgrad_step(lib.rn_conv2d_nhwc_wgrad, (ctypes.byref(p), dw.data_ptr(), 0.0, ws.data_ptr(), ws.numel()),
                                "rn_conv2d_nhwc_wgrad", flw, self._wgrad_bytes(p),
                                self._wgrad_kernel_name(p) + " + wgrad_reduce_kernel", "wgrad:" + cname, [kvar],
                                item=(p, dw, ws, flw) if dw_live is None else None)
        if dw_live is not None:
            def padded_wgrad(st, wgrad=step.run, src=dw, dst=dw_live):
                wgrad(st)
                _C.check(lib.rn_reduce_rows_f32(_C.ptr(src), 1, dst.numel(), dst.numel(), 0.0, _C.ptr(dst), st),
                         "live rows of a padded weight gradient")
            step = BackwardStep(padded_wgrad, side=True, writes=step.writes)
        self.bwd_steps.append(step)

    def _plan_bias_grad(self, cname, cops, ops, dy_of, grp):
        """Bias gradient of conv layer `cname` = column sums of dy over every segment (two-stage reduction kernel).
        ops: the launch `cops` belong to; grp: its BnGroup when the BatchNorm behind it trains, else None."""
        lib = self.lib
        pb2 = _C.BnProblem()
        pb2.num_segments, pb2.act, pb2.bessel, pb2.eps, pb2.momentum, pb2.count_scale = len(cops), 0, 0, 0.0, 0.0, 1.0
        cw = dy_of[cops[0]["out"]].shape[3]    # channel width of dy (padded for prediction convs)
        bs = torch.zeros((len(cops), 2, cw), dtype=torch.float32, device=self.dev)
        for i, op in enumerate(cops):
            dy = dy_of[op["out"]]
            s = pb2.seg[i]
            s.y, s.sums = dy.data_ptr(), bs[i].data_ptr()
            s.P, s.C = dy.shape[0] * dy.shape[1] * dy.shape[2], cw
        # A conv in front of a live BatchNorm: its dy is written by rn_bn_bwd_apply, which can sum the columns of
        # what it stores on the way out (rn_bn_segment.dy_colsum_partial) — stage 1 of this reduction then never
        # reads the dy tensor again (FPN + head-tower convs: 17 launches, ~1 ms of side-stream HBM reads per step;
        # same-process A/B of the step with / without ANY bias-gradient launch: 29.73 / 29.50 ms).  Where
        # rn_bn_bwd_colsum_chunks refuses a segment, and in front of a frozen BatchNorm (rn_bn_frozen_bwd has no
        # such epilogue), the separate pass stays.
        fused_cs = False
        if grp is not None:
            pb = grp.problem
            seg_of = [ops.index(op) for op in cops]
            chunks = [lib.rn_bn_bwd_colsum_chunks(ctypes.byref(pb), j) for j in seg_of]
            if all(ch > 0 for ch in chunks):
                fused_cs = True
                for i, ch in enumerate(chunks):
                    pb2.seg[i].ext_chunks = ch
        ws2 = torch.zeros((max(lib.rn_bn_workspace_bytes(ctypes.byref(pb2)), 256),), dtype=torch.uint8,
                          device=self.dev)
        if fused_cs:
            for i, j in enumerate(seg_of):
                pb.seg[j].dy_colsum_partial = ws2.data_ptr() + lib.rn_bn_partial_offset_bytes(ctypes.byref(pb2), i)
        db = self._pview(cname + "/bias", self.G)
        self._keep += [pb2, bs, ws2]

        def bias_grad(st, pr=ctypes.byref(pb2), n=self.g.convs[cname]["cout"], rows=len(cops), stride=2 * cw):
            _C.check(lib.rn_bn_stats(pr, _C.ptr(ws2), ws2.numel(), st), "bias colsum")
            # sum of the per-level column sums (row 0 of every [2][cw] block), levels in order
            _C.check(lib.rn_reduce_rows_f32(_C.ptr(bs), rows, stride, n, 0.0, _C.ptr(db), st), "bias grad")
        self.bwd_steps.append(BackwardStep(bias_grad, side=True, writes=[cname + "/bias"]))

    def _plan_conv_backward(self, ops, joins):
        """Backward of the conv launch over `ops`: gradient at the conv outputs (through the BatchNorm, or plain), weight and
        bias gradient of every distinct (shared) conv layer, data gradients."""
        live = self._conv_trainable(ops[0])
        if not live and not self._passes_gradient(ops[0]):
            return
        live_bn = bool(self._bn_trainable(ops[0]))
        if live_bn or self._bn_apart(ops[0]):
            dy_of = self._plan_bn_backward(ops, joins)
        else:
            dy_of = self._plan_plain_dy(ops)
        self.dy_of.update(dy_of)
        by_conv = {}
        for op in ops if live else ():    # a frozen launch: the gradient at its outputs and the data gradients, no more
            by_conv.setdefault(op["conv"], []).append(op)
        for cname, cops in by_conv.items():
            self._plan_wgrad(cname, cops, dy_of)
            if self.g.convs[cname]["bias"]:
                self._plan_bias_grad(cname, cops, ops, dy_of, self.bn_groups[ops[0]["out"]] if live_bn else None)
        packs = {}
        for sub in self._distinct_inputs([op for op in ops if self.requires.get(op["inp"])]):
            self._plan_dgrad_launch(sub, dy_of, joins, packs)

    def _plan_dw_backward(self, ops, joins):
        """depthwise conv (+BN+act) backward: BN backward -> dy; weight gradient (summed over the levels of a
        shared separable conv); data gradient = the forward kernel on (zero-upsampled) dy with the
        tap-reversed filter, accumulating into gradient buffers that already hold a contribution."""
        lib, B = self.lib, self.B
        live = self._conv_trainable(ops[0])
        if not live and not self._passes_gradient(ops[0]):
            return
        if self._bn_trainable(ops[0]) or self._bn_apart(ops[0]):
            dy_of = self._plan_bn_backward(ops, joins)
        else:
            dy_of = {op["out"]: self.grad[op["out"]] for op in ops}
        by_layer = {}
        for op in ops if live else ():    # a frozen launch: the data gradients only
            by_layer.setdefault(op["dw"], []).append(op)
        for dname, dops in by_layer.items():
            d = self.g.dws[dname]
            p = _C.DwProblem()
            p.k, p.stride, p.pad_top, p.pad_left, p.act = d["k"], d["stride"], dops[0]["pad_top"], dops[0]["pad_left"], 0
            p.num_segments = len(dops)
            for i, op in enumerate(dops):
                x, dy = self._src(op["inp"]), dy_of[op["out"]]
                s = p.seg[i]
                s.x, s.y = x.data_ptr(), dy.data_ptr()
                s.N, s.H, s.W, s.C, s.Ho, s.Wo = B, x.shape[1], x.shape[2], d["C"], dy.shape[1], dy.shape[2]
            ws = torch.empty((max(lib.rn_depthwise_wgrad_workspace_bytes(ctypes.byref(p)), 256),), dtype=torch.uint8,
                             device=self.dev)
            self._keep += [p, ws]
            self.dw_wgrad_launches.append(("dw_wgrad:" + dname, p))
            a = (ctypes.byref(p), self._pview(d["kvar"], self.G).data_ptr(), ws.data_ptr(), ws.numel())
            self.bwd_steps.append(BackwardStep(lambda st, a=a: _C.check(lib.rn_depthwise_conv2d_nhwc_wgrad(*a, st), "dw wgrad"),
                                               side=True, writes=[d["kvar"]]))
        flips = {}
        for sub in self._distinct_inputs([op for op in ops if self.requires.get(op["inp"])]):
            d0 = self.g.dws[sub[0]["dw"]]
            k, stride = d0["k"], d0["stride"]
            if stride not in (1, 2):
                raise NotImplementedError("stride > 2")
            p = _C.DwProblem()
            p.k, p.stride, p.act, p.num_segments = k, 1, 0, len(sub)
            p.pad_top, p.pad_left = k - 1 - sub[0]["pad_top"], k - 1 - sub[0]["pad_left"]
            name = "dw_dgrad:" + "+".join(o["out"] for o in sub)
            ups = []
            for i, op in enumerate(sub):
                d = self.g.dws[op["dw"]]
                if op["dw"] not in flips:
                    buf = torch.empty((k * k, d["C"]), dtype=self.h16, device=self.dev)
                    flips[op["dw"]] = buf
                    if live:
                        off, _ = self.p_off[d["kvar"]]
                        self.dw_flip_packs.append((self.P.data_ptr() + 4 * off, k, d["C"], buf))
                    else:         # a constant: _pack_frozen_dgrad_weights
                        self.frozen_dw_flip_packs.append((d["kvar"], k, d["C"], buf))
                src = dy_of[op["out"]]
                x = self._src(op["inp"])
                H, W = x.shape[1], x.shape[2]
                if stride == 2:
                    src = self._zero_upsampled(src, H, W, ups)
                gbuf, accumulate = joins.add(op["inp"], name)
                s = p.seg[i]
                s.x, s.w, s.y = src.data_ptr(), flips[op["dw"]].data_ptr(), gbuf.data_ptr()
                s.scale, s.shift = None, None
                s.residual = gbuf.data_ptr() if accumulate else None
                s.N, s.H, s.W, s.C, s.Ho, s.Wo = B, H, W, d["C"], H, W
            self._keep.append(p)
            self.dw_launches.append((name, "dgrad", p, ups))
            self.bwd_steps.append(self._dgrad_step(ups, functools.partial(lib.rn_depthwise_conv2d_nhwc_fwd, ctypes.byref(p)),
                                                   what="dw dgrad"))

    def _bn_bwd_fusable(self, name):
        """(rn_bn_problem, segment) of the BatchNorm + ReLU layer that produced `name` when stage 1 of its backward
        reduction can run in the epilogue of the ONE data-gradient launch that writes its dz: trainable BatchNorm,
        relu, no residual input, no drop_connect factors, a single-segment group, a single consumer."""
        if not self.fuse_bn_bwd or name in self.bal_src or len(self.readers.get(name, [])) != 1:
            return None
        hit = self._bn_of_tensor.get(name)
        if hit is None:
            return None
        pb, i, o, nseg = hit
        if nseg != 1 and not self.fuse_bn_bwd_groups:
            return None
        if (o["op"] != "conv" or o.get("act") != "relu" or o.get("residual") or
                o.get("survival") is not None or not self._bn_trainable(o) or pb.seg[i].sample_scale):
            return None
        return pb, i

    def _fuse_bn_bwd(self, p, need):
        """Stage 1 of the BatchNorm backward reduction of the layers whose dz the data-gradient launch `p` over `need`
        writes, in its epilogue.  Returns the algorithmic bytes this adds to `p` (the y its epilogue reads).
        All segments of a BatchNorm problem or none (rn_bn_bwd_reduce): a problem is switched over once the launches
        planned so far write dz of EVERY one of its segments, each exactly once — one launch for a bottleneck layer,
        one launch over both heads x five levels for head-tower depths 0-2, the two prediction convs' data gradients
        together for depth 3.  Until then the assignments wait in self._bn_bwd_pending; the rn_conv_problem structs
        are read at launch time, so they can still be patched when the last segment turns up."""
        lib = self.lib
        hits = [self._bn_bwd_fusable(op["inp"]) for op in need]
        if any(h is None for h in hits):
            return 0
        added = 0
        for i, (op, (pb, j)) in enumerate(zip(need, hits)):
            pend = self._bn_bwd_pending.setdefault(id(pb), {"pb": pb, "seg": {}})
            if j in pend["seg"]:          # a second writer: not a single-consumer layer after all
                pend["dead"] = True
            pend["seg"][j] = (p, i, op["inp"])
        for key in {id(pb) for pb, _ in hits}:
            pend = self._bn_bwd_pending[key]
            pb = pend["pb"]
            if pend.get("dead") or pend.get("done") or sorted(pend["seg"]) != list(range(pb.num_segments)):
                continue
            pend["done"] = True
            for j, (cp, ci, _) in pend["seg"].items():
                pb.seg[j].ext_chunks_bwd = lib.rn_conv_bn_row_blocks(ctypes.byref(cp), ci)
            wsb = torch.zeros((max(lib.rn_bn_workspace_bytes(ctypes.byref(pb)), 256),), dtype=torch.uint8, device=self.dev)
            self.bn_bwd_ws[key] = wsb
            for j, (cp, ci, name) in pend["seg"].items():
                sg = cp.seg[ci]
                sg.bn_partial = wsb.data_ptr() + lib.rn_bn_bwd_partial_offset_bytes(ctypes.byref(pb), j)
                sg.bn_bwd_y = self.raw[name].data_ptr()
                sg.bn_bwd_fwd = pb.seg[j].fwd
                self.bn_bwd_fused.append(name)
                y_bytes = 2 * int(pb.seg[j].P) * int(pb.seg[j].C)
                if cp is p:
                    added += y_bytes
                else:                      # an earlier launch: add the bytes of y its epilogue now reads
                    fl0, by0 = self._algo[id(cp)]
                    self._algo[id(cp)] = (fl0, by0 + y_bytes)
        return added

    def _plan_dgrad_launch(self, need, dy_of, joins, packs):
        """One data-gradient launch over the ops `need` (distinct inputs): the forward implicit-GEMM kernel on dy with the
        flipped / transposed weights, in one of three forms chosen per launch."""
        lib, B = self.lib, self.B
        c0 = self.g.convs[need[0]["conv"]]
        k, stride, pad = c0["k"], c0["stride"], need[0]["pad"]
        if stride not in (1, 2):
            raise NotImplementedError("stride > 2")
        # 1x1 / stride 2 (projection shortcuts): dx is non-zero only at the even positions, so the GEMM runs on dy
        # as it is (a quarter of the pixels of the zero-upsampled form) and rn_scatter_add2x puts the rows in place
        lowres = k == 1 and stride == 2 and pad == 0
        # 3x3 / stride 2 / pad 1 on even inputs (the first block of ResNet stages 2-4): sub-pixel form — one 2x2
        # stride-1 conv of dy with 4*Cin phase-major output channels + a depth-to-space, 16 tap products per dy pixel
        # instead of the 36 (9 useful) of the zero-upsampled form (rn_dgrad_pack.pad_ == 1)
        subpixel = (k == 3 and stride == 2 and pad == 1
                    and all(self._src(o["inp"]).shape[1] % 2 == 0 and self._src(o["inp"]).shape[2] % 2 == 0
                            and self.g.convs[o["conv"]]["cin"] % 8 == 0 for o in need))   # rn_depth_to_space2x: C % 8
        # every other layer: dy itself (stride 1) or zero-upsampled (stride 2), written or accumulated in place
        p = _C.attach_splitk_workspace(_C.ConvProblem(), self.splitk_ws)
        p.opts = self.launch_opts
        p.R = p.S = 2 if subpixel else k
        p.stride_h = p.stride_w = 1
        p.pad_top = p.pad_left = 0 if subpixel else k - 1 - pad
        p.act, p.out_dtype, p.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, len(need)
        ups, post, joined = [], [], False   # rn_upsample_zero2x before the launch; per-segment arguments of the form's post-op
        post_op = ((lib.rn_depth_to_space2x, "rn_depth_to_space2x") if subpixel else
                   (lib.rn_scatter_add2x, "rn_scatter_add2x") if lowres else None)
        name = "dgrad:" + (need[0].get("group") or need[0]["out"])
        fl = by = 0
        for i, op in enumerate(need):
            c = self.g.convs[op["conv"]]
            cin = c["cin"]
            dy = dy_of[op["out"]]
            cw = dy.shape[3]
            cwp = lib.rn_conv_cin_pad(cw)     # K of the dgrad GEMM, zero padded in the packed weights only
            if op["conv"] not in packs:
                shape = (lib.rn_conv_cout_pad(4 * cin), 2, 2, cwp) if subpixel else (lib.rn_conv_cout_pad(cin), k, k, cwp)
                packs[op["conv"]] = torch.empty(shape, dtype=self.h16, device=self.dev)
                kvar = c.get("kvar", op["conv"] + "/kernel")
                if kvar in self.p_off:
                    self.dgrad_packs.append((self.P.data_ptr() + 4 * self.p_off[kvar][0], k, cin, c["cout"], cwp,
                                             packs[op["conv"]], 1 if subpixel else 0))
                else:             # frozen conv: a constant, packed when weights are loaded (_pack_frozen_dgrad_weights)
                    self.frozen_dgrad_packs.append((kvar, k, cin, c["cout"], cwp, packs[op["conv"]], 1 if subpixel else 0))
            x = self._src(op["inp"])
            H, W = x.shape[1], x.shape[2]
            gbuf, accumulate = joins.add(op["inp"], name)
            joined = joined or accumulate
            # what the forms differ in: source, destination, output channels, residual, post-op arguments
            src, dst, cout, res = dy, gbuf, cin, None
            if subpixel:
                cout = 4 * cin
                dst = torch.empty((B, dy.shape[1], dy.shape[2], cout), dtype=self.h16, device=self.dev)
                post.append((dst.data_ptr(), gbuf.data_ptr(), B, dy.shape[1], dy.shape[2], cin, int(accumulate)))
            elif lowres:
                dst = torch.empty((B, dy.shape[1], dy.shape[2], cin), dtype=self.h16, device=self.dev)
                post.append((dst.data_ptr(), gbuf.data_ptr(), B, dy.shape[1], dy.shape[2], cin, H, W, int(accumulate)))
            else:
                if stride == 2:
                    src = self._zero_upsampled(dy, H, W, ups)
                res = gbuf.data_ptr() if accumulate else None
            if dst is not gbuf:
                self._keep.append(dst)
            s = p.seg[i]
            s.x, s.w, s.y = src.data_ptr(), packs[op["conv"]].data_ptr(), dst.data_ptr()
            s.scale, s.shift, s.residual = None, None, res
            s.N, s.H, s.W, s.Cin, s.pix_stride = B, src.shape[1], src.shape[2], cw, cw
            s.Ho, s.Wo, s.Cout = dst.shape[1], dst.shape[2], cout
            # algorithmic work — the layer's own MACs and tensors: dy [B,Ho,Wo,Cout] in, dx [B,H,W,Cin] out (+ accumulate read)
            Ho, Wo = self.tensors[op["out"]][:2]
            fl += 2 * B * Ho * Wo * k * k * cin * c["cout"]
            by += 2 * B * Ho * Wo * c["cout"] + 2 * B * H * W * cin * (2 if res else 1) + 2 * k * k * cin * c["cout"]
        # the BatchNorm-backward epilogue takes dz as it leaves the GEMM: the plain stride-1 form, first writer everywhere
        if post_op is None and stride == 1 and not joined:
            by += self._fuse_bn_bwd(p, need)
        self._algo[id(p)] = (fl, by)
        self._keep.append(p)
        self.conv_launches.append((name, p))
        self.bwd_steps.append(self._dgrad_step(ups, functools.partial(self._launch_conv, p, what="dgrad"), post_op, post))

    # op kind -> planner(self, the op or the ops of its launch, joins) of its backward steps (_build_backward)
    _backward_planners = {"conv": _plan_conv_backward, "dwconv": _plan_dw_backward, "se": _plan_se_backward,
                          "maxpool": _plan_maxpool_backward, "stem": _plan_stem_backward,
                          "topdown": _plan_topdown_backward, "balance": _plan_balance_backward}

    # ---- one training step -----------------------------------------------------------------------------
    def refresh_dgrad_weights(self, st):
        lib = self.lib
        if self.dgrad_packs:
            _C.check(lib.rn_pack_conv_weight_dgrad_batch(self._dgrad_pack_items, len(self.dgrad_packs), st),
                     "pack dgrad")
        for (mptr, k, C, buf) in self.dw_flip_packs:
            _C.check(lib.rn_pack_depthwise_weight_flip(mptr, k, C, buf.data_ptr(), st), "pack dw flip")

    def draw_drop_connect(self):
        """binary = floor(survival_prob + U[0,1)); factor = binary / survival_prob, per image (:107-112)."""
        u = torch.rand(self.dc_all.shape, generator=self.dc_generator, device=self.dev, dtype=torch.float32)
        torch.div(torch.floor(u.add_(self.dc_p)), self.dc_p, out=self.dc_all)

    def forward(self, images, draw=True):
        st = _C.current_stream()
        if draw and self.dc_masks:
            self.draw_drop_connect()
        own = self.t["images"]
        if (images.device == own.device and images.dtype == own.dtype and images.shape == own.shape
                and images.is_contiguous()):
            # the only reader is the NHWC4 packing kernel at the head of the launch list: read the batch where it is
            # (a 157 MB device copy per step at 640x640x32 otherwise)
            self._images_ref = images
            self._images_ptr = images.data_ptr()
        else:
            own.copy_(images, non_blocking=True)
            self._images_ptr = own.data_ptr()
        for fn in self.fwd_steps:
            fn(st)
        return self.outputs

    def _ensure_side_stream(self):
        if self._side_stream is None:
            # a stream that really runs beside the caller's (probed: HIP's stream -> hardware-queue map depends on how
            # many streams the process created before — _C.concurrent_stream)
            probes, agree = [], None
            if self.small.through_c10d:
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_backend(self.pg) == "nccl":
                    # the SyncBN messages hop main -> c10d's stream -> main: that stream must not share a queue with this
                    # one either (its packets would wait behind every weight gradient queued before them)
                    tiny = torch.zeros((64,), dtype=torch.float32, device=self.dev)
                    dist.all_reduce(tiny, group=self.pg)      # (c10d picks its stream at the first collective)
                    probes.append(lambda tiny=tiny: dist.all_reduce(tiny, group=self.pg))

                    def agree(ok, dist=dist):          # every rank keeps or drops the candidate together
                        v = torch.tensor([1.0 if ok else 0.0], device=self.dev)
                        dist.all_reduce(v, op=dist.ReduceOp.MIN, group=self.pg)
                        return bool(v.item() == 1.0)
            self._side_stream, self.side_stream_probed = _C.concurrent_stream(
                self.lib, self.dev, [torch.cuda.current_stream(self.dev)], probes=probes, agree=agree)
            self._side_events = [torch.cuda.Event() for _ in self.bwd_steps]
        return self._side_stream

    def _prepack_dgrad_weights(self):
        """The data-gradient weight layouts (taps flipped, [Cin][R][S][Cout]) depend only on the weights the last
        optimizer step left: repack them on the second stream while the forward pass runs instead of at the head
        of the backward pass (0.2 ms of HBM-bound work off the critical path)."""
        if not self.side_stream_on:
            return
        side = self._ensure_side_stream()
        side.wait_stream(torch.cuda.current_stream(self.dev))   # after the optimizer and the previous backward pass
        with torch.cuda.stream(side):
            self.refresh_dgrad_weights(ctypes.c_void_p(side.cuda_stream))
        self._dgrad_prepacked = True

    def loss_grad_buffers(self):
        """The dy tensors of the prediction convs (bf16 [B,H,W,padded channels]) keyed like the predictions: handed to
        RetinaNetLoss(grads_bf16=...) so that the loss kernels write the upstream gradients where backward() reads
        them (pad channels stay zero from allocation)."""
        return self._loss_dy

    def backward(self, loss_grads):
        """loss_grads: RetinaNetLoss.grads (f32, per level), or None when the loss wrote loss_grad_buffers()
        -> parameter gradients in self.G."""
        lib, st = self.lib, _C.current_stream()
        if loss_grads is not None:   # None: the loss kernels already wrote bf16 into loss_grad_buffers()
            for key in self.g.outputs:   # class-predictions, box-predictions (+ iou-predictions: the auxiliary head)
                for lv, name in self.g.outputs[key].items():
                    gsrc = loss_grads[key][lv]
                    dst = self.dy_of[name]
                    C = gsrc.shape[-1]
                    _C.check(lib.rn_cast_pad_f32_to_bf16(gsrc.data_ptr(), dst.data_ptr(), gsrc.numel() // C, C,
                                                         dst.shape[3], st), "cast")
        if self._dgrad_prepacked:     # train_step repacked them beside the forward pass
            torch.cuda.current_stream(self.dev).wait_stream(self._side_stream)
            self._dgrad_prepacked = False
        else:
            self.refresh_dgrad_weights(st)
        overlap = self.overlap.begin(self._train_step_active, self._step_args)
        if not self.side_stream_on:
            for i, step in enumerate(self.bwd_steps):
                step.run(st)
                if overlap:
                    self.overlap.after_step(i, torch.cuda.current_stream(self.dev), None)
            return
        # two streams: a side step waits (event) for everything the main stream has enqueued so far — its inputs
        # dy / x are complete at that point and are not written again before the join below — and the main stream
        # carries on with the data gradients; the optimizer (clip: global norm over every gradient) follows the join
        main = torch.cuda.current_stream(self.dev)
        side = self._ensure_side_stream()
        sst = ctypes.c_void_p(side.cuda_stream)
        fresh = False            # the side stream already waits for the newest main-stream work
        for i, step in enumerate(self.bwd_steps):
            if step.side:
                if not fresh:
                    ev = self._side_events[i]
                    ev.record(main)
                    side.wait_event(ev)
                    fresh = True
                with torch.cuda.stream(side):
                    step.run(sst)
            else:
                step.run(st)
                fresh = False
            if overlap:
                self.overlap.after_step(i, main, side)
        main.wait_stream(side)

    def _ready_steps(self):
        """variable -> index of the last backward step that writes its gradient (GradientOverlap plans its buckets by it)"""
        ready = {k: i for i, step in enumerate(self.bwd_steps) for k in step.writes}
        missing = [k for k in self.train_names if k not in ready]
        if missing:
            raise RuntimeError(f"no backward step completes the gradient of {missing[:4]}")
        return ready

    # ---- what bench.py and retinanet.comm reach through the engine ---------------------------------------------------
    _buckets = property(lambda self: self.overlap.buckets)
    _overlap_unsafe = property(lambda self: self.overlap.unsafe)
    clip_fired = property(lambda self: self.overlap.clip_fired)
    bucket_host_ms = property(lambda self: self.overlap.bucket_host_ms)

    @property
    def native_comm(self):
        return self.small.native_comm

    @native_comm.setter
    def native_comm(self, comm):
        self.small.native_comm = comm

    @property
    def native_comm_buckets(self):
        return self.overlap.native_comm

    @native_comm_buckets.setter
    def native_comm_buckets(self, comm):
        self.overlap.native_comm = comm

    def _optim_rule(self, opt, lr, ema_decay):
        """rn_optim_rule of an optimizer configuration; lr is the kernel's scalar (OptimizerConfig.step_size)"""
        rule = {"sgd": _C.RN_OPT_SGD, "adam": _C.RN_OPT_ADAM, "rmsprop": _C.RN_OPT_RMSPROP,
                "adagrad": _C.RN_OPT_ADAGRAD}[opt.name]
        flags = 0
        if opt.name == "sgd" and opt.nesterov:
            flags |= _C.RN_OPT_NESTEROV
        if opt.name == "adam" and opt.amsgrad:
            flags |= _C.RN_OPT_AMSGRAD
        if opt.name == "rmsprop":
            flags |= (_C.RN_OPT_CENTERED if opt.centered else 0) | (_C.RN_OPT_MOMENTUM if opt.momentum > 0.0 else 0)
        return _C.OptimRule(rule=rule, flags=flags, lr=lr, beta1=opt.beta_1, beta2=opt.beta_2, rho=opt.rho,
                            momentum=opt.momentum, epsilon=opt.epsilon,
                            ema_decay=ema_decay if ema_decay is not None else 0.0)

    def optimizer_step(self, lr, momentum, clipnorm, wd_alpha, ema_decay, nesterov=False, overlapped=False, opt=None):
        """weight decay + per-tensor / global clipping (executor.py:401-407) + all-reduce SUM (executor.py:436-437)
        + the update rule / moving average (optimizers/builder.py:45-54).  overlapped=True: backward() already sent the
        buckets (GradientOverlap); only the flag check / correction and the step kernel are left.  opt: the
        OptimizerConfig whose name picks the rule of rn_optim_step, lr being the rule's scalar (for Adam alpha_t); None:
        the SGD rule of lr, momentum, nesterov."""
        lib, st = self.lib, _C.current_stream()
        unscale = 1.0 / self.loss_scale["scale"] if self.loss_scale else 1.0
        if opt is not None and opt.name != self._slot_owner:
            raise RuntimeError(f"optimizer_step: the slot arenas belong to {self._slot_owner}, not {opt.name}")
        if opt is not None:
            rule = self._optim_rule(opt, lr, ema_decay)
        else:
            rule = _C.OptimRule(rule=_C.RN_OPT_SGD, flags=_C.RN_OPT_NESTEROV if nesterov else 0, lr=lr, momentum=momentum,
                                ema_decay=ema_decay if ema_decay is not None else 0.0)

        def update(skip_ptr):
            _C.check(lib.rn_optim_step(self.P.data_ptr(), self.G.data_ptr(), self.V.data_ptr(), _C.ptr(self.S1),
                                       _C.ptr(self.S2), self.E.data_ptr() if ema_decay is not None else None,
                                       self.Pbf.data_ptr(), self.segs_dev.data_ptr(), self.block_seg_dev.data_ptr(),
                                       self.n_blocks, ctypes.byref(rule), skip_ptr, st), "rn_optim_step")
        if overlapped:
            # G[0] = sum over the ranks of "a clip factor != 1 or the gradient norm is not finite".  A NaN norm leaves every
            # factor at 1 (fmaxf drops it): rn_optim_clip_factors tests the global norm for finiteness on its own and
            # sets flags[0] then too, so G[0] == 0 also says every gradient is finite
            applied = self.overlap.finish(lambda: update(self.G.data_ptr()), read_flag=not self.price_without_flag_read)
            if applied:
                self.refresh_packs()
                if self.loss_scale:
                    self._update_loss_scale()
                return
            skip = self.G.data_ptr() + 4 if self.loss_scale else None     # G[1]: not finite on some rank
        else:
            _C.check(lib.rn_optim_clip(self.G.data_ptr(), self.P.data_ptr(), self.segs_dev.data_ptr(), self.n_segs,
                                       self.block_seg_dev.data_ptr(), self.n_blocks, wd_alpha / self.world, wd_alpha,
                                       unscale, clipnorm if clipnorm else 0.0, self.metrics.data_ptr(),
                                       self.opt_ws.data_ptr(), self.opt_ws.numel(), st), "rn_optim_clip")
            skip = None
            if self.loss_scale:
                self.G[1:2].copy_(self.metrics[5:6])
                skip = self.G.data_ptr() + 4
            if self.dp_active:
                from retinanet.distribute import all_reduce_sum_bucketed
                all_reduce_sum_bucketed(self.G, 2 if self.world == 1 else self.world, self.pg)   # executor.py:436-437: SUM after clipping
        update(skip)
        self.refresh_packs()
        if self.loss_scale:
            self._update_loss_scale()

    def _update_loss_scale(self, flags=None):
        """tf.keras.mixed_precision.LossScaleOptimizer(dynamic=True) (optimizers/builder.py:56-64): halve the scale
        when a step's gradients were not finite (the step was dropped), double it after `growth_steps` good steps.
        flags: the arena whose slot [1] holds "not finite" (default G; the accumulated step hands in A).

        The step kernel drops the update itself (skip pointer); what the HOST needs — the next loss scale, whether
        optimizer.iterations advances — it needs only when the NEXT step reaches its loss: the flag goes to pinned
        memory with an asynchronous copy here and is applied by _resolve_loss_scale(), which the next train_step calls
        after it has enqueued its forward pass (or finish_step(), for whoever reads the counters in between).  Reading
        it here (`.item()`) drained the queue at the end of every mixed_float16 step: the device then idled ~1 ms at the
        head of the next step until the host had launched its first kernels (tools/trace_gaps.py on configs[4])."""
        if self._ls_host is None:
            self._ls_host = torch.zeros((1,), dtype=torch.float32, pin_memory=True)
            self._ls_event = torch.cuda.Event()
        self._ls_host.copy_((self.G if flags is None else flags)[1:2], non_blocking=True)
        self._ls_event.record(torch.cuda.current_stream(self.dev))
        self._ls_pending = True

    def _resolve_loss_scale(self):
        if not self._ls_pending:
            return
        self._ls_pending = False
        self._ls_event.synchronize()
        ls = self.loss_scale
        bad = float(self._ls_host[0]) != 0.0
        ls["skipped"] = bad
        if bad:
            ls["scale"], ls["good"] = max(ls["scale"] / 2.0, 1.0), 0
            self.step_count -= 1              # a dropped step does not advance optimizer.iterations
            self.model.optimizer.iterations = self.step_count
        else:
            ls["good"] += 1
            if ls["good"] >= ls["growth_steps"]:
                ls["scale"], ls["good"] = ls["scale"] * 2.0, 0

    def finish_step(self):
        """Host-side state of the last train_step (loss scale, optimizer.iterations) brought up to date: call before
        reading them between steps (the executor does after each execution; state_dict does)."""
        self._resolve_loss_scale()

    def weights_info(self, histogram=False, bucket_count=30):
        """The reference's --enable_weights_info (executor.py:329-344) for every trainable variable at once: tf.norm, the
        finite minimum / maximum, the count of NaN / inf elements and, histogram=True, TensorBoard's `bucket_count` buckets
        over linspace(min, max, bucket_count + 1) (rn_arena_stats / rn_arena_histogram, include/rnet_hip.h).  Reads the fp32
        master weights P — not the moving average, not the 16-bit copies — in the stream that ordered the last optimizer
        step; writes no arena and touches no planned launch.  One device -> host copy per call.
        -> {"names": train_names, "norm" f32[n], "min" f32[n], "max" f32[n], "nonfinite" i32[n], "counts" i32[n, buckets] | None}"""
        if not 1 <= int(bucket_count) <= 64:
            raise ValueError(f"weights_info: bucket_count {bucket_count} is outside 1..64")
        lib, n, nb = self.lib, self.n_segs, int(bucket_count)
        self.finish_step()
        with torch.cuda.device(self.dev):
            if self._wi is None:
                ws = torch.empty((lib.rn_arena_stats_workspace_bytes(self.n_blocks, n),), dtype=torch.uint8, device=self.dev)
                # one i32 result arena, so that one copy brings everything over: [n][3] stats (f32 bits), [n] nonfinite,
                # [n][64] counts (the first n * bucket_count of them are in use)
                out = torch.zeros((n * (4 + 64),), dtype=torch.int32, device=self.dev)
                self._wi = (ws, out, torch.empty((n * (4 + 64),), dtype=torch.int32, pin_memory=True))
            ws, out, host = self._wi
            st = _C.current_stream()
            stats, bad, counts = out.data_ptr(), out.data_ptr() + 12 * n, out.data_ptr() + 16 * n
            _C.check(lib.rn_arena_stats(self.P.data_ptr(), self.segs_dev.data_ptr(), n, self.block_seg_dev.data_ptr(),
                                        self.n_blocks, stats, bad, ws.data_ptr(), ws.numel(), st), "rn_arena_stats")
            if histogram:
                _C.check(lib.rn_arena_histogram(self.P.data_ptr(), self.segs_dev.data_ptr(), n,
                                                self.block_seg_dev.data_ptr(), self.n_blocks, stats, nb, counts, st),
                         "rn_arena_histogram")
            used = n * (4 + (nb if histogram else 0))
            host[:used].copy_(out[:used], non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()
        res = host[:used].numpy().copy()
        s = res[:3 * n].view(np.float32).reshape(n, 3)
        return {"names": list(self.train_names), "norm": s[:, 0].copy(), "min": s[:, 1].copy(), "max": s[:, 2].copy(),
                "nonfinite": res[3 * n:4 * n].copy(),
                "counts": res[4 * n:].reshape(n, nb).copy() if histogram else None}

    def train_step(self, images, targets):
        """(images f32[B,H,W,3], targets from LabelEncoder.encode_batch) -> the loss dict of Executor._train_step
        (executor.py:409-441; device scalars)."""
        if self.accumulation_steps != 1:
            raise RuntimeError(f"train_step is one optimizer step over one batch; this engine accumulates "
                               f"{self.accumulation_steps} micro-batches per step: call train_step_accumulated")
        cfg = self.params_cfg.training
        opt = self.model.optimizer
        if self.model.loss._num_replicas() != self.world:
            raise RuntimeError(f"RetinaNetLoss sees {self.model.loss._num_replicas()} replicas, the engine {self.world}")
        if opt.dynamic_loss_scale and self.loss_scale is None:
            self.loss_scale = dict(scale=float(opt.initial_loss_scale), good=0, growth_steps=int(opt.loss_scale_growth_steps),
                                   skipped=False)
        with torch.cuda.device(self.dev):
            self._bind_optimizer()          # slot arenas of the rule `opt` names (a no-op unless the optimizer was replaced)
            alpha = cfg.weight_decay_alpha if cfg.use_weight_decay else 0.0
            self._prepack_dgrad_weights()
            # the moving-average normaliser is replica-local: nothing of it rides in the SyncBN messages, and
            # c2_normalizer stays None for the loss call below
            self.small.begin_step(targets["num-positives"],
                                  carry_normalizer=not self.model.loss.use_moving_average_normalizer)
            preds = self.forward(images)
            self._resolve_loss_scale()      # the previous step's "gradients not finite" flag: long since on the host
            step = self.step_count
            scale = self.loss_scale["scale"] if self.loss_scale else 1.0
            self._step_args = dict(wdc=alpha / self.world, alpha=alpha, unscale=1.0 / scale,
                                   clip=float(opt.clipnorm) if opt.clipnorm else 0.0)
            # per_replica_loss = total / replicas, times the loss scale under mixed_float16 (executor.py:421-425)
            loss = self.model.loss(targets, preds, compute_grads=True, grad_scale=scale / self.world,
                                   grads_bf16=self.loss_grad_buffers(), normalizer=self.small.c2_normalizer)
            self._train_step_active = True
            try:
                self.backward(None)
            finally:
                self._train_step_active = False
            overlapped = self.overlap.on      # backward() sent the gradient buckets as it completed them
            if overlapped and self.overlap.done != len(self.overlap.buckets):
                raise RuntimeError("overlapped all-reduce: not every gradient bucket was launched")
            # step_size: the schedule's rate; Adam's alpha_t with t = step + 1 — `step` was read after
            # _resolve_loss_scale(), so a dropped mixed_float16 step does not advance t
            self.optimizer_step(opt.step_size(step), opt.momentum, opt.clipnorm, alpha,
                                opt.ema_decay(step) if opt.use_moving_average else None, nesterov=opt.nesterov,
                                overlapped=overlapped, opt=opt)
            self.syncbn_messages_per_step = self.small.end_step()
            self.step_count += 1              # (taken back by _resolve_loss_scale when the step turns out dropped)
            opt.iterations = self.step_count
        out = dict(loss)
        out["total-loss"] = loss["weighted-loss"]                # executor.py:414-419
        if cfg.use_weight_decay:
            out["l2-regularization"] = self.metrics[3]
            out["total-loss"] = loss["weighted-loss"] + self.metrics[3]
        out["gradient-norm"] = self.metrics[0] * self.world      # executor.py:440
        out["num-anchors-matched"] = loss["num-anchors-matched"] / self.B   # executor.py:439
        return out

    # ---- gradient accumulation (training.gradient_accumulation_steps = N > 1; DESIGN "Gradient accumulation") -------------
    def accumulate_micro_step(self, images, targets, index):
        """Micro-step `index` of N: forward, loss and backward as in train_step on a micro-batch of B images, with the
        reference's per-replica arithmetic for R * N replicas (executor.py:401-437: loss / (R N), alpha / (R N) of the decay
        gradient, the clip on THIS micro-step's gradient alone), then factor * t into (index 0) or onto the accumulator A.
        G holds the stage-1 tensor t afterwards.  Returns the micro-step's loss dict (values of its own, not views)."""
        N = self.accumulation_steps
        if N < 2:
            raise RuntimeError("accumulate_micro_step: the engine was built with accumulation_steps = 1: call train_step")
        if index != self._micro_next or not 0 <= index < N:
            raise RuntimeError(f"accumulate_micro_step: micro-step {index} of {N}, expected {self._micro_next}")
        cfg = self.params_cfg.training
        opt = self.model.optimizer
        if self.model.loss._num_replicas() != self.world:
            raise RuntimeError(f"RetinaNetLoss sees {self.model.loss._num_replicas()} replicas, the engine {self.world}")
        if opt.dynamic_loss_scale and self.loss_scale is None:
            self.loss_scale = dict(scale=float(opt.initial_loss_scale), good=0, growth_steps=int(opt.loss_scale_growth_steps),
                                   skipped=False)
        replicas = self.world * N
        with torch.cuda.device(self.dev):
            self._bind_optimizer()
            alpha = cfg.weight_decay_alpha if cfg.use_weight_decay else 0.0
            self._prepack_dgrad_weights()
            self.small.begin_step(targets["num-positives"],
                                  carry_normalizer=not self.model.loss.use_moving_average_normalizer)
            preds = self.forward(images)
            if index == 0:                  # one loss scale for the N micro-steps of an optimizer step
                self._resolve_loss_scale()
                self._micro_scale = self.loss_scale["scale"] if self.loss_scale else 1.0
                self._micro_messages = 0
            scale = self._micro_scale
            clip = float(opt.clipnorm) if opt.clipnorm else 0.0
            self._step_args = dict(wdc=alpha / replicas, alpha=alpha, unscale=1.0 / scale, clip=clip)
            loss = self.model.loss(targets, preds, compute_grads=True, grad_scale=scale / replicas,
                                   grads_bf16=self.loss_grad_buffers(), normalizer=self.small.c2_normalizer)
            self.backward(None)             # (_train_step_active stays False: no bucket leaves during a micro-step)
            _C.check(self.lib.rn_optim_clip_accumulate(
                self.G.data_ptr(), self.P.data_ptr(), self.A.data_ptr(), 1 if index == 0 else 0, self.segs_dev.data_ptr(),
                self.n_segs, self.block_seg_dev.data_ptr(), self.n_blocks, alpha / replicas, alpha, 1.0 / scale, clip,
                self.metrics.data_ptr(), self.opt_ws.data_ptr(), self.opt_ws.numel(), _C.current_stream()),
                "rn_optim_clip_accumulate")
            self._micro_messages += self.small.end_step()
            self._micro_next = index + 1
            out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in loss.items()}
            out["total-loss"] = out["weighted-loss"]                 # executor.py:414-419
            if cfg.use_weight_decay:
                out["l2-regularization"] = self.metrics[3].clone()
                out["total-loss"] = out["weighted-loss"] + out["l2-regularization"]
            out["gradient-norm"] = self.metrics[0] * replicas    # executor.py:440 with R * N replicas
            out["num-anchors-matched"] = loss["num-anchors-matched"] / self.B
        return out

    def apply_accumulated(self):
        """After micro-step N - 1: all-reduce SUM of A over the ranks (plain order), ONE rn_optim_step from A — dropped
        under a LossScaleOptimizer when any micro-step on any rank was not finite (A[1]) —, refresh_packs, the loss-scale
        bookkeeping and the counters of one optimizer step."""
        N = self.accumulation_steps
        if N < 2 or self._micro_next != N:
            raise RuntimeError(f"apply_accumulated: {self._micro_next} of {N} micro-steps accumulated")
        opt = self.model.optimizer
        step = self.step_count              # read after micro-step 0 resolved the previous step's flag
        with torch.cuda.device(self.dev):
            if opt.name != self._slot_owner:
                raise RuntimeError(f"apply_accumulated: the slot arenas belong to {self._slot_owner}, not {opt.name}")
            ema_decay = opt.ema_decay(step) if opt.use_moving_average else None
            rule = self._optim_rule(opt, opt.step_size(step), ema_decay)
            if self.dp_active:
                from retinanet.distribute import all_reduce_sum_bucketed
                all_reduce_sum_bucketed(self.A, 2 if self.world == 1 else self.world, self.pg)   # executor.py:436-437
            skip = self.A.data_ptr() + 4 if self.loss_scale else None
            _C.check(self.lib.rn_optim_step(self.P.data_ptr(), self.A.data_ptr(), self.V.data_ptr(), _C.ptr(self.S1),
                                            _C.ptr(self.S2), self.E.data_ptr() if ema_decay is not None else None,
                                            self.Pbf.data_ptr(), self.segs_dev.data_ptr(), self.block_seg_dev.data_ptr(),
                                            self.n_blocks, ctypes.byref(rule), skip, _C.current_stream()), "rn_optim_step")
            self.refresh_packs()
            if self.loss_scale:
                self._update_loss_scale(self.A)
            self.syncbn_messages_per_step = self._micro_messages
            self._micro_next = 0
            self.step_count += 1              # (taken back by _resolve_loss_scale when the step turns out dropped)
            opt.iterations = self.step_count

    def train_step_accumulated(self, micro_batches):
        """One optimizer step over N (images, targets) micro-batches -> the loss dict of train_step: every loss entry and
        num-anchors-matched the mean over the micro-steps, gradient-norm the mean of the micro-steps' clipped norms times
        R * N, l2-regularization that of the last micro-step (the weights do not change inside a step)."""
        micro_batches = list(micro_batches)
        N = self.accumulation_steps
        if len(micro_batches) != N:
            raise ValueError(f"train_step_accumulated: {len(micro_batches)} micro-batches for accumulation_steps = {N}")
        outs = [self.accumulate_micro_step(images, targets, i) for i, (images, targets) in enumerate(micro_batches)]
        self.apply_accumulated()
        return mean_loss_dict(outs)
