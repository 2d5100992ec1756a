"""The data-parallel machinery of the training step, apart from the launch planning of TrainEngine:
  * plan_buckets: which slice of the gradient arena goes out after which backward step (pure host arithmetic);
  * GradientOverlap: the bucketed gradient all-reduce overlapped with the backward pass;
  * SmallMessages: the SyncBatchNorm all-reduces and the loss normaliser that rides in the step's first one.
"""
from __future__ import annotations

import ctypes
import logging
import os
import time

import torch

from retinanet import _C


def plan_buckets(train_names, p_off, seg_blocks, ready_step, bucket_bytes):
    """-> (buckets, bucket_at).  train_names: the trainable variables in arena order; p_off[name] = (arena offset, floats),
    seg_blocks[name] = (first optimizer block, blocks), ready_step[name] = the last backward step that writes the
    variable's gradient.  A bucket = dict(begin, end: arena extent in floats; block_begin, block_count: its optimizer
    blocks; ready: the backward step after which it is complete); a new one starts once the current holds `bucket_bytes`.
    bucket_at[step] = the buckets that go out after that step, bucket 0 after the others: it carries the flag slots at
    the head of the arena and must be the last bucket of the pass (GradientOverlap._launch_bucket)."""
    buckets, cur = [], None
    for k in train_names:     # arena order = forward order: the backward pass completes the tail first
        off, n = p_off[k]
        b0, nb = seg_blocks[k]
        if cur is None or (cur["end"] - cur["begin"]) * 4 >= bucket_bytes:
            cur = dict(begin=off, end=off, block_begin=b0, block_count=0, ready=-1)
            buckets.append(cur)
        cur["end"] = (off + n + 3) // 4 * 4
        cur["block_count"] += nb
        cur["ready"] = max(cur["ready"], ready_step[k])
    buckets[0]["begin"] = 0        # the flag slots ride in the bucket that completes last
    order = sorted(range(len(buckets)), key=lambda j: (buckets[j]["ready"], -j))
    if order[-1] != 0:             # keep the invariant simple: bucket 0 goes last
        buckets[0]["ready"] = max(b["ready"] for b in buckets)
    bucket_at = {}
    for j, bkt in enumerate(buckets):
        bucket_at.setdefault(bkt["ready"], []).append(j)
    for lst in bucket_at.values():
        lst.sort(reverse=True)     # bucket 0 after the others that become ready with the same step
    return buckets, bucket_at


class SmallMessages:
    """The small per-layer messages of a data-parallel step: SyncBatchNorm sums (C3) and the loss normaliser (C2), which
    rides in the spare slot of the step's FIRST SyncBN message instead of being a collective of its own."""

    def __init__(self, lib, dev, pg, world, sync_bn):
        self.lib, self.dev, self.pg, self.world, self.sync_bn = lib, dev, pg, world, sync_bn
        self.native_comm = None    # retinanet.comm.NativeComm (maybe_enable_native), else torch.distributed carries them
        self.count = 0             # messages sent since the step began
        self._c2_local = None      # this rank's sum(num-positives) + 1 until a message has taken it along
        self.c2_normalizer = None  # all_reduce_sum(...) / replicas, once that message is merged
        # False: the step sends no SyncBN forward message (every BatchNorm frozen), so nothing can take the normaliser
        # along — c2_normalizer stays None and RetinaNetLoss does its own all-reduce
        self.has_carrier = True

    @property
    def through_c10d(self):
        """the messages hop main stream -> c10d's stream -> main stream"""
        return self.sync_bn and self.native_comm is None

    def begin_step(self, num_positives, carry_normalizer=True):
        """carry_normalizer=False: the loss keeps a replica-local moving average (loss.normalizer.use_moving_average,
        retinanet_loss.py:40-44) and all-reduces nothing — the C2 slot stays empty, as without a carrier."""
        self.count = 0
        self._c2_local = self.c2_normalizer = None
        if self.sync_bn and self.has_carrier and carry_normalizer:    # sum(num-positives) + 1 of this rank (retinanet_loss.py:38): folded into SyncBN traffic
            # (a device kernel reads it: a host tensor, or one on another GPU, must be moved first)
            npos = num_positives.to(self.dev, torch.float32).contiguous()
            self._c2_local = torch.empty((1,), dtype=torch.float32, device=self.dev)
            _C.check(self.lib.rn_reduce_rows_f32(_C.ptr(npos), npos.numel(), 1, 1, 1.0, _C.ptr(self._c2_local),
                                                 _C.current_stream()), "num-positives + 1")

    def all_reduce(self, t):
        """rn_allreduce_small on the compute stream when a native communicator was handed in, torch.distributed otherwise"""
        self.count += 1
        if self.native_comm is not None:
            self.native_comm.all_reduce_small(t)
        else:
            import torch.distributed as dist
            dist.all_reduce(t, group=self.pg)

    def merge_stats(self, sums):
        """SUM of a BatchNorm group's [sum | sumsq] message over the replicas, in place (retinanet_loss.py:46-49 for the
        normaliser the first one takes along)"""
        from retinanet.distribute import syncbn_merge
        c2, self._c2_local = self._c2_local, None
        norm = syncbn_merge(sums, self.world, self.all_reduce, c2)
        if c2 is not None:
            self.c2_normalizer = norm

    def end_step(self):
        self._c2_local = None      # a forward pass outside train_step sends plain messages
        return self.count if self.sync_bn else 0


class GradientOverlap:
    """Gradient all-reduce overlapped with the backward pass.

    executor.py:432-437 clips the LOCAL gradients and then sums them over the replicas; the clip factors need every
    gradient, so a literal translation can only start the all-reduce after the whole backward pass.  Here the
    buckets go out as the backward pass completes them, UNclipped ("optimistic": local gradients are pre-divided by
    the replica count, so the per-tensor / global norms sit far below clipnorm after the first steps), each rank
    keeps a copy of what it sent, and at the end one flag that rode in the last bucket says whether any rank's
    factor was != 1.  Only then is the correction sum_r (factor_r - 1) * g_r all-reduced and added — the result is
    sum_r factor_r * g_r, the reference's clip-then-sum.

    backward() drives it: begin() at the head of the pass, after_step() behind every backward step; optimizer_step()
    calls finish()."""

    def __init__(self, lib, dev, *, G, P, metrics, segs_dev, block_seg_dev, n_blocks, n_segs, opt_ws, train_names, p_off,
                 seg_blocks, ready_steps, small, pg, world, dp_active, side_stream, accumulation_steps=1):
        """G, P, metrics: the engine's gradient / parameter arenas and metric slots; segs_dev .. opt_ws: the optimizer's
        tables; train_names, p_off, seg_blocks: plan_buckets' inputs; ready_steps(): variable -> last backward step that
        writes its gradient, asked when the buckets are planned; small: the engine's SmallMessages; side_stream(): the
        weight-gradient stream, or None while there is none; accumulation_steps > 1: the engine accumulates micro-steps,
        whose clip needs each micro-step's whole gradient before anything is summed — the overlap stays off."""
        self.accumulation_steps = accumulation_steps
        self.lib, self.dev, self.small, self.pg, self.world, self.dp_active = lib, dev, small, pg, world, dp_active
        self.G, self.P, self.metrics, self.opt_ws = G, P, metrics, opt_ws
        self.segs_dev, self.block_seg_dev, self.n_blocks, self.n_segs = segs_dev, block_seg_dev, n_blocks, n_segs
        self.train_names, self.p_off, self.seg_blocks = train_names, p_off, seg_blocks
        self._ready_steps, self._side_stream = ready_steps, side_stream
        self._stream_probe = os.environ.get("RNET_STREAM_PROBE", "1") != "0"   # _bucket_group_is_safe
        self._bucket_bytes = int(os.environ.get("RNET_C1_BUCKET_MB", "25")) << 20
        self.native_comm = None   # retinanet.comm.NativeComm for the buckets (rn_allreduce_bucket), or None
        self.on = False           # this backward pass sends the buckets
        self.done = 0             # buckets launched in this pass
        self.buckets = None       # plan_buckets' plan, made by the first pass that uses it
        self._bucket_at = {}      # backward step -> buckets complete after it
        self._comm_events = []    # per bucket: "the main stream's gradients of this bucket are enqueued"
        self._bucket_stream = None   # the stream that carried the last pass's buckets
        self._works = []
        self._step_args = None
        self.L = None             # what this rank contributed to the buckets (for the clip correction)
        self.pg_c1 = None         # the buckets' own process group
        self._probe_bucket_group = False   # pg_c1 is new: _bucket_group_is_safe has not looked at it yet
        self.unsafe = False       # ... and found that its stream blocks the main stream: plain order
        self._helper = None       # _bucket_group_is_safe's stream
        self._flag_host = self._flag_event = None   # pinned copy of the clip flag G[0] and its event
        self.clip_fired = False
        self.bucket_host_ms = 0.0   # longest host time inside one torch.distributed bucket all-reduce call (bench.py)

    def begin(self, train_step_active, step_args):
        """True when this backward pass launches the gradient all-reduce bucket by bucket (world > 1, or forced
        with RNET_C1_OVERLAP=1 for the single-replica equivalence test).  step_args: wdc, alpha, unscale, clip of the step."""
        mode = os.environ.get("RNET_C1_OVERLAP", "auto")
        on = train_step_active and (mode == "1" or (mode != "0" and self.dp_active)) and self.accumulation_steps == 1
        self._works = []
        self._step_args = step_args
        self.on = on
        if not on:
            return False
        if self.buckets is None:
            self.buckets, self._bucket_at = plan_buckets(self.train_names, self.p_off, self.seg_blocks, self._ready_steps(),
                                                         self._bucket_bytes)
            # Which stream prepares a bucket and hands it to RCCL.  Round 3 used a third stream of its own; round 5 measured
            # (tools/probes/dp_overlap_trace.py, 1-rank nccl group on one MI355X, rocprofv3 kernel trace) that HIP mapped
            # it onto the SAME hardware queue as the weight-gradient stream: a bucket's "wait for the main stream" packet
            # then sat in front of weight-gradient kernels that had nothing to wait for — 2.3 ms of chip idle per step
            # against 0.7 ms, step 34.4 ms against 31.4 ms for the plain order (and 44 ms with GPU_MAX_HW_QUEUES=8) — the
            # overlap machinery cost more than the all-reduce it hides.  So the bucket work rides on the weight-gradient
            # stream itself (most of a bucket's producers are there; it waits for the main stream's BatchNorm gamma / beta
            # gradients through one event per bucket) or, in the one-stream backward, on the main stream: no extra queue.
            self._comm_events = [torch.cuda.Event() for _ in self.buckets]
            self.L = torch.zeros_like(self.G)
            self._flag_host = torch.zeros((1,), dtype=torch.float32, pin_memory=True)
            self._flag_event = torch.cuda.Event()
            if self.dp_active:
                import torch.distributed as dist
                self._probe_bucket_group = True
                # its own communicator: the latency-bound SyncBN all-reduces of the main stream must not queue
                # behind a 25 MB bucket on the same RCCL stream
                self.pg_c1 = dist.new_group(backend=dist.get_backend(self.pg))
        if self._probe_bucket_group:
            self._probe_bucket_group = False
            if self.native_comm is None and not self._bucket_group_is_safe():
                # c10d's stream for the bucket group shares a hardware queue with the main stream: every bucket's "wait for
                # the weight-gradient stream" packet would stall the main stream's kernels behind it.  All ranks agreed
                # (MIN): this job keeps the plain order — all-reduce after the backward pass.
                logging.warning("gradient-bucket overlap disabled: c10d's stream for the bucket group blocks the main stream "
                                "on this process's hardware-queue map (RNET_STREAM_PROBE=0 skips the probe)")
                self.unsafe = True
        if self.unsafe:
            self.on = False
            return False
        self.done = 0
        return True

    def _bucket_group_is_safe(self):
        """Does an async all-reduce of the bucket group, issued from the weight-gradient stream while that stream still
        waits for something, leave the main stream alone — its kernels AND the SyncBN all-reduces it issues through the
        other group (two c10d streams on one hardware queue: every SyncBN message would wait for the bucket's producers)?
        (_C.wait_blocks; collective: the ranks agree.)  c10d picks a group's stream when the group is first used, so a group
        that fails is replaced by a fresh one, three times at most."""
        import torch.distributed as dist
        side = self._side_stream()
        if side is None or not self._stream_probe or dist.get_backend(self.pg_c1) != "nccl":
            return True
        main = torch.cuda.current_stream(self.dev)
        tiny = torch.zeros((64,), dtype=torch.float32, device=self.dev)
        tiny2 = torch.zeros((64,), dtype=torch.float32, device=self.dev)
        helper = self._helper = torch.cuda.Stream(self.dev)
        for attempt in range(4):
            with torch.cuda.stream(side):
                dist.all_reduce(tiny, group=self.pg_c1)          # c10d picks the group's stream at its first collective
            torch.cuda.synchronize(self.dev)
            blocked = False
            probes = [lambda: _C.check(self.lib.rn_probe_spin(1, ctypes.c_void_p(main.cuda_stream)), "rn_probe_spin")]
            if self.small.through_c10d:
                probes.append(lambda: dist.all_reduce(tiny2, group=self.pg))
            for probe in probes:                                 # (every probe on every rank: they may be collectives)
                works = []

                def pre(works=works):   # the group's stream now waits for the weight-gradient stream, which waits for the helper
                    with torch.cuda.stream(side):
                        works.append(dist.all_reduce(tiny, group=self.pg_c1, async_op=True))
                blocked = _C.wait_blocks(self.lib, side, probe, main, helper, pre=pre) or blocked
                with torch.cuda.stream(side):
                    for w in works:
                        w.wait()
                torch.cuda.synchronize(self.dev)
            v = torch.tensor([0.0 if blocked else 1.0], device=self.dev)
            dist.all_reduce(v, op=dist.ReduceOp.MIN, group=self.pg)
            if bool(v.item() == 1.0):
                return True
            if attempt < 3:
                self.pg_c1 = dist.new_group(backend=dist.get_backend(self.pg))
        return False

    def after_step(self, i, main, side):
        """backward step i is enqueued (main: the stream of the data gradients, side: the weight-gradient stream or None)"""
        for j in self._bucket_at.get(i, ()):
            self._launch_bucket(j, main, side)

    def _launch_bucket(self, j, main, side):
        lib, bkt = self.lib, self.buckets[j]
        comm = side if side is not None else main   # the weight-gradient stream (or the only stream) carries the bucket work
        if side is not None:
            self._comm_events[j].record(main)
            side.wait_event(self._comm_events[j])
        self._bucket_stream = comm
        cst = ctypes.c_void_p(comm.cuda_stream)
        a = self._step_args
        with torch.cuda.stream(comm):
            _C.check(lib.rn_optim_clip_prepare(self.G.data_ptr(), self.P.data_ptr(), self.segs_dev.data_ptr(),
                                               self.block_seg_dev.data_ptr(), self.n_blocks, bkt["block_begin"],
                                               bkt["block_count"], a["wdc"], a["unscale"], self.L.data_ptr(),
                                               self.opt_ws.data_ptr(), self.opt_ws.numel(), cst), "rn_optim_clip_prepare")
            self.done += 1
            if self.done == len(self.buckets):
                assert j == 0
                # every gradient of this rank is final: clip factors, metrics, and the two flags into G[0:2]
                _C.check(lib.rn_optim_clip_factors(self.segs_dev.data_ptr(), self.n_segs, self.n_blocks, a["clip"],
                                                   a["alpha"], self.metrics.data_ptr(), self.G.data_ptr(),
                                                   self.opt_ws.data_ptr(), self.opt_ws.numel(), cst), "rn_optim_clip_factors")
            if self.dp_active and self.native_comm is not None:
                # rn_allreduce_bucket (rn_comm.hip): one ncclAllReduce on the bucket's stream, behind its prepare kernel
                self.native_comm.all_reduce_bucket(self.G[bkt["begin"]:bkt["end"]])
            elif self.dp_active:
                import torch.distributed as dist
                t0 = time.perf_counter()
                self._works.append(dist.all_reduce(self.G[bkt["begin"]:bkt["end"]], group=self.pg_c1, async_op=True))
                self.bucket_host_ms = max(self.bucket_host_ms, (time.perf_counter() - t0) * 1e3)

    def finish(self, optimistic_update, read_flag=True):
        """After the join: wait for the buckets; when some rank's clip fired, all-reduce the correction.
        optimistic_update: callable that enqueues the step kernel with the device-side predicate "G[0] == 0" (no clip fired on
        any rank, no gradient non-finite: the common case).  The flag goes to pinned host memory with an asynchronous copy
        enqueued BEFORE that kernel, the host waits for the copy's event only — the kernel runs while the host decides and
        carries on enqueueing (a blocking `.item()` left the device idle for the host's wake-up and the next launches:
        0.24 - 0.38 ms per step, bench.py's extra.dp_overhead).  Returns True when the optimistic kernel applied the step;
        False when the flag fired (the kernel was a no-op: the caller runs the step kernel after the correction below).
        read_flag=False (bench.py's extra.dp_overhead ONLY: what the host read costs): no read, no kernel, "not fired"."""
        cur = torch.cuda.current_stream(self.dev)
        for w in self._works:
            w.wait()
        if self._bucket_stream is not None and self._bucket_stream != cur:
            cur.wait_stream(self._bucket_stream)
        applied = fired = False
        if read_flag:
            self._flag_host.copy_(self.G[0:1], non_blocking=True)
            self._flag_event.record(cur)
            optimistic_update()                      # predicate on the device: a no-op when G[0] != 0
            self._flag_event.synchronize()
            fired = float(self._flag_host[0]) != 0.0
            applied = not fired
        self.clip_fired = fired
        if not fired:
            return applied
        st = _C.current_stream()
        _C.check(self.lib.rn_optim_clip_apply(self.L.data_ptr(), self.L.data_ptr(), self.segs_dev.data_ptr(),
                                              self.block_seg_dev.data_ptr(), self.n_blocks, self.opt_ws.data_ptr(),
                                              self.opt_ws.numel(), st), "rn_optim_clip_apply")
        self.L[:4].zero_()
        if self.dp_active:
            from retinanet.distribute import all_reduce_sum_bucketed
            all_reduce_sum_bucketed(self.L, 2 if self.world == 1 else self.world, self.pg)   # (forced: issue it anyway)
        self.G[4:].add_(self.L[4:])
        return False
