"""Host logic of the convolution dispatchers (no GPU: rn_conv_kernel_id / rn_conv_tile_rows / rn_conv_bn_row_blocks /
rn_conv_splitk_workspace_bytes and, for the weight gradients, rn_wgrad_kernel_id / rn_wgrad_workspace_bytes /
rn_wgrad_group_fused / rn_wgrad_group_workspace_bytes are pure functions of the problem descriptors; without a device the
library assumes the MI355X's 256 compute units).  Pins which kernel family, tile shape and split plan the layers of the
bench configurations get — the policy DESIGN.md section 4 describes — so that a dispatcher edit shows up as a diff here,
not as a silent slow-down on the GPU box."""
import ctypes
import json
import os

import pytest

from retinanet import _C

WS = 64 << 20   # a split-K workspace "is attached" (address never dereferenced by the queries)


def _problem(B, H, W, Cin, Cout, k, stride=1, ws=False, f32=False, w_terms=0, w_pair=0, segs=None):
    p = _C.ConvProblem()
    p.R = p.S = k
    p.stride_h = p.stride_w = stride
    p.pad_top = p.pad_left = (k - 1) // 2
    p.act, p.out_dtype = 0, (_C.RN_DT_F32 if f32 else _C.RN_DT_BF16)
    segs = segs or [(H, W, Cin, Cout)]
    p.num_segments = len(segs)
    for i, (h, w, ci, co) in enumerate(segs):
        s = p.seg[i]
        ho, wo = (h + 2 * p.pad_top - k) // stride + 1, (w + 2 * p.pad_left - k) // stride + 1
        s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = B, h, w, ci, ci, ho, wo, co
        s.w_terms, s.w_pair = w_terms, w_pair
    if ws:
        p.splitk_ws, p.splitk_ws_bytes = 16, WS
    return p


def _q(p):
    lib = _C.lib()
    r = ctypes.byref(p)
    return (lib.rn_conv_kernel_id(r), lib.rn_conv_tile_rows(r), lib.rn_conv_bn_row_blocks(r, 0),
            int(lib.rn_conv_splitk_workspace_bytes(r)))


PYR = [(80, 80), (40, 40), (20, 20), (10, 10), (5, 5)]

CASES = [
    # name, problem kwargs, (kernel id, tile rows), balanced?, splits?
    ("B32 head tower 3x3 (both heads, five levels)", dict(B=32, H=0, W=0, Cin=0, Cout=0, k=3, segs=[(h, w, 256, 256) for h, w in PYR] * 2), (3, 512), False, False),
    ("B32 stage-3 3x3 256", dict(B=32, H=40, W=40, Cin=256, Cout=256, k=3), (3, 512), False, False),
    ("B32 stage-2 3x3 128", dict(B=32, H=80, W=80, Cin=128, Cout=128, k=3), (3, 512), False, False),
    ("B32 stage-1 3x3 64 (plain form)", dict(B=32, H=160, W=160, Cin=64, Cout=64, k=3), (0, 128), False, False),
    ("B32 stage-1 3x3 64 as pixel pairs", dict(B=32, H=160, W=80, Cin=128, Cout=128, k=3), (3, 512), False, False),
    ("B32 stage-2 *_out 1x1 128->512", dict(B=32, H=80, W=80, Cin=128, Cout=512, k=1), (1, 256), True, False),
    ("B32 stage-3 *_out 1x1 256->1024", dict(B=32, H=40, W=40, Cin=256, Cout=1024, k=1), (1, 256), True, False),
    ("B32 stage-3 *_a 1x1 1024->256 (K > 512: whole tiles)", dict(B=32, H=40, W=40, Cin=1024, Cout=256, k=1), (1, 256), False, False),
    ("B32 stage-1 *_out 1x1 64->256 (12.5 rounds: nothing to balance)", dict(B=32, H=160, W=160, Cin=64, Cout=256, k=1), (1, 256), False, False),
    ("B32 stage-2 *_a 1x1 512->128 (narrow: 128-row kernel)", dict(B=32, H=80, W=80, Cin=512, Cout=128, k=1), (0, 128), False, False),
    ("B32 stage-4 first 1x1 2048->512 (100 256-row tiles: 128-row kernel)", dict(B=32, H=20, W=20, Cin=2048, Cout=512, k=1), (0, 128), False, False),
    ("B32 class prediction 3x3, one plane (training)", dict(B=32, H=0, W=0, Cin=0, Cout=0, k=3, f32=True, segs=[(h, w, 256, 720) for h, w in PYR]), (3, 512), False, False),
    ("B32 box prediction 3x3, planes along Cout", dict(B=32, H=0, W=0, Cin=0, Cout=0, k=3, f32=True, w_pair=1, segs=[(h, w, 256, 36) for h, w in PYR]), (3, 512), False, False),
    ("B8 stage-4 3x3 512 with a workspace: 128-row kernel (200 tiles of 128 x 64: nothing to split)", dict(B=8, H=20, W=20, Cin=512, Cout=512, k=3, ws=True), (0, 128), False, False),
    ("B8 stage-3 3x3 256 with a workspace: 128-row kernel", dict(B=8, H=40, W=40, Cin=256, Cout=256, k=3, ws=True), (0, 128), False, False),
    ("B8 stage-4 3x3 512 without a workspace: 128-row kernel", dict(B=8, H=20, W=20, Cin=512, Cout=512, k=3), (0, 128), False, False),
    ("B1 stage-4 3x3 512: 128-row kernel, split along K", dict(B=1, H=20, W=20, Cin=512, Cout=512, k=3, ws=True), (0, 128), False, True),
    ("B1 stage-4 first 1x1 2048->512: split", dict(B=1, H=20, W=20, Cin=2048, Cout=512, k=1, ws=True), (0, 128), False, True),
    ("B1 stage-1 1x1 64->64 (one K step: nothing to split)", dict(B=1, H=160, W=160, Cin=64, Cout=64, k=1, ws=True), (0, 128), False, False),
    ("B1 head tower 3x3: 128-row kernel (the pyramid launches stay off the halo kernel's split tiles)", dict(B=1, H=0, W=0, Cin=0, Cout=0, k=3, ws=True, segs=[(h, w, 256, 256) for h, w in PYR] * 2), (0, 128), False, False),
    ("B1 FPN output 3x3: 128-row kernel", dict(B=1, H=0, W=0, Cin=0, Cout=0, k=3, ws=True, segs=[(h, w, 256, 256) for h, w in PYR]), (0, 128), False, False),
]


@pytest.mark.parametrize("name,kw,kernel,balanced,splits", CASES, ids=[c[0] for c in CASES])
def test_dispatch_of_the_bench_layers(name, kw, kernel, balanced, splits):
    p = _problem(**kw)
    kid, rows, blocks, ws = _q(p)
    assert (kid, rows) == kernel, (kid, rows)
    s = p.seg[0]
    M = s.N * s.Ho * s.Wo
    whole = (rows // 128) * -(-M // rows)
    if balanced:
        assert blocks > whole and blocks % 2 == 0, (blocks, whole)       # two (short) blocks per balanced tile
        r = 2 * M / blocks                                               # rows per tile, within rounding
        n_tiles = -(-s.Cout // 256)
        tiles = (blocks // 2) * n_tiles
        assert tiles <= -(-(-(-M // 256) * n_tiles) // 256) * 256        # the same number of rounds as whole tiles
        assert 64 <= r <= 240
    else:
        assert blocks == whole, (blocks, whole)
    assert (ws > 0) == splits, ws
    if splits:
        assert ws <= _C.lib().rn_conv_splitk_workspace_max_bytes()


def test_forced_tile_shapes_keep_whole_tiles():
    """rn_launch_opts (tests, A/B timing) switch the balancing off: the partial-sum layout of a forced launch is the plain one"""
    p = _problem(B=32, H=40, W=40, Cin=256, Cout=1024, k=1)
    assert _q(p)[2] == 512
    p.opts = _C.LaunchOpts(conv_tile=2)
    assert _q(p)[:3] == (1, 256, 400)
    p.opts = _C.LaunchOpts(max_workgroups=64)
    assert _q(p)[2] == 400



def _table():
    with open(os.path.join(os.path.dirname(__file__), "golden", "conv_dispatch_table.json")) as f:
        return json.load(f)["rows"]


def test_dispatch_table():
    """The whole policy, not only the bench layers: tests/golden/conv_dispatch_table.json holds (descriptor, kernel id, tile
    rows, BatchNorm row blocks per segment, split-K workspace bytes) as the dispatcher answered BEFORE its decisions moved
    into one plan (rn_conv_dispatch.hip: conv_plan) — recorded from that library, 256 compute units, never from the
    planner.  The rows are one or two descriptors of every distinct outcome (kernel id x tile rows x splits or not x balanced
    or not x forced rn_launch_opts) of a grid of 610 984 descriptors, and of every such outcome with each batch (1 / 2 / 8 /
    32), shape (the pyramid sizes, odd and wide ones, one of more than 2^22 pixels), 1x1 / 3x3, stride 1 / 2, output type with
    w_terms / w_pair, workspace (none / 64 MB / 1 MB), bias + residual, and segment count (1, 2, 3, the five-level and
    ten-segment launches).  The library must reproduce every row."""
    lib = _C.lib()
    rows = _table()
    assert 300 <= len(rows) <= 2500
    assert {r[10] for r in rows} == {0, 1, 2, 3}
    bad = []
    for B, k, stride, segs, f32, w_terms, w_pair, ws_bytes, opts, bias_res, kid, tile_rows, blocks, ws in rows:
        p = _problem(B, 0, 0, 0, 0, k, stride=stride, f32=bool(f32), w_terms=w_terms, w_pair=w_pair, segs=[tuple(s) for s in segs])
        p.opts = _C.LaunchOpts(**opts)
        if ws_bytes:
            p.splitk_ws, p.splitk_ws_bytes = 16, ws_bytes
        for i in range(len(segs)):
            if bias_res:   # read as "null or not" only
                p.seg[i].bias, p.seg[i].residual = 16, 16
        r = ctypes.byref(p)
        got = [lib.rn_conv_kernel_id(r), lib.rn_conv_tile_rows(r), [lib.rn_conv_bn_row_blocks(r, i) for i in range(len(segs))],
               int(lib.rn_conv_splitk_workspace_bytes(r))]
        if got != [kid, tile_rows, blocks, ws]:
            bad.append((B, k, stride, segs, f32, w_terms, w_pair, ws_bytes, opts, bias_res, got, [kid, tile_rows, blocks, ws]))
    assert not bad, (len(bad), bad[:5])

# ---- weight gradients (rn_wgrad_dispatch.hip: wgrad_plan) -------------------------------------------------------------
def _wgrad_layer(R, S, stride, pad, segs, opts):
    p = _C.WgradProblem()
    p.R, p.S, p.stride_h, p.stride_w, p.pad_top, p.pad_left = R, S, stride, stride, pad, pad
    p.num_segments = len(segs)
    for i, (N, H, W, Cin, Ho, Wo, Cout, dyS, xS, null) in enumerate(segs):
        s = p.seg[i]
        s.x, s.dy = (0 if null else 16), 16      # dummy addresses: the queries read them as "null or not" only
        s.N, s.H, s.W, s.Cin, s.Ho, s.Wo, s.Cout, s.dy_pix_stride, s.x_pix_stride = N, H, W, Cin, Ho, Wo, Cout, dyS, xS
    p.opts = _C.LaunchOpts(**opts)
    return p


def _wgrad_group(R, S, stride, pad, segs, opts, n, alt):
    """n layers of one geometry; alt = [k, "segs" | "opts", value]: layer k has its own segments or options"""
    layers = []
    for i in range(n):
        sg, op = segs, opts
        if alt and alt[0] == i:
            sg, op = (alt[2], opts) if alt[1] == "segs" else (segs, alt[2])
        layers.append(_wgrad_layer(R, S, stride, pad, sg, op))
    return layers


def _wgrad_answers(layers):
    lib = _C.lib()
    n = len(layers)
    arr = (ctypes.POINTER(_C.WgradProblem) * n)(*[ctypes.pointer(p) for p in layers])
    return [[lib.rn_wgrad_kernel_id(ctypes.byref(p)) for p in layers],
            [int(lib.rn_wgrad_workspace_bytes(ctypes.byref(p))) for p in layers],
            lib.rn_wgrad_group_fused(arr, n), int(lib.rn_wgrad_group_workspace_bytes(arr, n))]


def _dense(k, Cin, Cout, sizes, B=32):
    return [[B, h, w, Cin, h, w, Cout, 0, 0, 0] for h, w in sizes]


WGRAD_CASES = [
    # name, (k, stride, pad), segments, layers in the group, then at batch 32 WITHOUT and WITH the engine's default cap
    # (wgrad_target_blocks = 160 for the wide kernels, 208 for the 128-tile kernel): (kernel id of a layer, split-K chunks of
    # a layer on its own, fused, chunks the group's workspace holds: the fused launch's or one layer's, whichever is more)
    ("head towers: eight 3x3 256 layers over five levels, one launch", (3, 1, 1), _dense(3, 256, 256, PYR), 8, (2, 32, 1, 32), (2, 20, 1, 20)),
    ("stage-3 3x3 256: five layers, one launch", (3, 1, 1), _dense(3, 256, 256, [(40, 40)]), 5, (2, 32, 1, 32), (2, 20, 1, 20)),
    ("stage-2 3x3 128: three layers, one launch", (3, 1, 1), _dense(3, 128, 128, [(80, 80)]), 3, (2, 128, 1, 128), (2, 80, 1, 80)),
    ("stage-4 3x3 512: two layers of 12 800 pixels (alone: 128 tiles; as a group: segments of one launch)", (3, 1, 1), _dense(3, 512, 512, [(20, 20)]), 2, (0, 4, 1, 8), (0, 2, 1, 6)),
    ("stage-3 *_a 1x1 1024->256: five layers as segments", (1, 1, 0), _dense(1, 1024, 256, [(40, 40)]), 5, (1, 64, 1, 64), (1, 40, 1, 40)),
    ("stage-3 *_out 1x1 256->1024: six layers as segments", (1, 1, 0), _dense(1, 256, 1024, [(40, 40)]), 6, (1, 64, 1, 64), (1, 40, 1, 40)),
    ("stage-2 *_a 1x1 512->128: three layers as segments (128-tile kernel)", (1, 1, 0), _dense(1, 512, 128, [(80, 80)]), 3, (0, 128, 1, 129), (0, 52, 1, 54)),
    ("class prediction 3x3 256->720 over five levels", (3, 1, 1), _dense(3, 256, 720, PYR), 1, (2, 10, 0, 10), (2, 6, 0, 6)),
    ("box prediction 3x3 256->36 over five levels (Cout % 8: per-tap 128 tiles)", (3, 1, 1), _dense(3, 256, 36, PYR), 1, (0, 32, 0, 32), (0, 15, 0, 15)),
    ("FPN output 3x3 256 at 80 x 80", (3, 1, 1), _dense(3, 256, 256, [(80, 80)]), 1, (2, 32, 0, 32), (2, 20, 0, 20)),
    ("stem 7x7 stride 2 on the packed image (R = 7, S = 1, 32 channels, x_pix_stride 4)", (7, 2, 0), [[32, 646, 648, 32, 320, 320, 64, 0, 4, 0]], 1, (0, 74, 0, 74), (0, 30, 0, 30)),
]


@pytest.mark.parametrize("name,filt,segs,n,free,capped", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_dispatch_of_the_bench_layers(name, filt, segs, n, free, capped):
    k, stride, pad = filt
    R, S = (k, 1) if name.startswith("stem") else (k, k)
    weight_bytes = segs[0][6] * R * S * segs[0][3] * 4
    for want, cap in ((free, False), (capped, True)):
        opts = {"wgrad_target_blocks": 208 if want[0] == 0 else 160} if cap else {}
        kids, wss, fused, gws = _wgrad_answers(_wgrad_group(R, S, stride, pad, segs, opts, n, None))
        assert kids == [want[0]] * n, (cap, kids)
        assert [w / weight_bytes for w in wss] == [want[1]] * n, (cap, wss)      # workspace = chunks x |W| x 4 bytes
        assert fused == want[2], (cap, fused)
        assert gws / weight_bytes == want[3], (cap, gws)


def test_wgrad_dispatch_table():
    """The weight-gradient policy: tests/golden/wgrad_dispatch_table.json holds (filter, segments, rn_launch_opts, layers in
    the group and the one layer that differs) -> (rn_wgrad_kernel_id and rn_wgrad_workspace_bytes per layer,
    rn_wgrad_group_fused, rn_wgrad_group_workspace_bytes) as the library answered BEFORE the decisions moved into one plan
    (rn_wgrad_dispatch.hip: wgrad_plan) — recorded from that library, 256 compute units, never from the planner.  Workspace
    bytes / weight bytes is the number of split-K chunks, so the rows pin the split plan and not only the kernel family.
    The rows are one descriptor of every distinct outcome (kernel ids x fused or not x which need sets the group's workspace
    x rejected or not x kind of odd layer) with each value of every axis of a grid of 1 052 968 descriptors (688 326 of them
    groups of 2 / 5 / 8 / 9 layers): batch 1 / 2 / 8 / 32, the pyramid sizes, 37 x 37 and 24 x 56 (pixel totals on both sides
    of 16 384), 1x1, 3x3 stride 1 / 2, the stem form (7 x 1, 32 channels, x_pix_stride 4), a strided dy, 19 channel pairs
    (2048 -> 2048 3x3: 576 tiles of 256, which wgrad_big_kernel refuses), 1 / 3 / 5 segments, wgrad_kernel 0 - 3,
    wgrad_target_blocks 0 / 1 / 64 / 160 / 176 / 208 / 300, reserved_cus 0 / 8; groups of identical layers that the halo kernel
    serves and that it does not (layers as segments), with one layer of another shape, with one layer of other options; and
    every rejection (Cin % 8, Cout % 4, a null tensor, 2^24 pixels, 2 GiB tensors, no segments, bad strides, bad options) alone
    and inside a group.  (A merged plan whose chunk count does not divide by the group size cannot be built: layers of
    identical geometry get equal chunk counts.)  The library must reproduce every row."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "wgrad_dispatch_table.json")) as f:
        rows = json.load(f)["rows"]
    assert 300 <= len(rows) <= 2500
    assert {k for r in rows for k in r[8]} == {-1, 0, 1, 2}          # every kernel, and the rejections
    assert {r[10] for r in rows} == {0, 1}                           # both answers of rn_wgrad_group_fused
    assert any(r[11] == 0 for r in rows) and any(r[9] == [0] for r in rows)
    bad = []
    for R, S, stride, pad, segs, opts, n, alt, kids, wss, fused, gws in rows:
        got = _wgrad_answers(_wgrad_group(R, S, stride, pad, segs, opts, n, alt))
        if got != [kids, wss, fused, gws]:
            bad.append((R, S, stride, pad, segs, opts, n, alt, got, [kids, wss, fused, gws]))
    assert not bad, (len(bad), bad[:5])


def _bn_problem(segs):
    p = _C.BnProblem()
    p.num_segments, p.act, p.bessel, p.eps, p.momentum, p.count_scale = len(segs), 0, 0, 1e-3, 0.9, 1.0
    for i, (P, C, ext, ext_bwd) in enumerate(segs):
        q = p.seg[i]
        q.P, q.C, q.ext_chunks, q.ext_chunks_bwd = P, C, ext, ext_bwd
    return p


def test_bn_workspace_layout():
    """rn_bn_workspace_bytes = [partial sums of the mode that needs more][one ticket counter per (segment, 16 channels)]
    [part slots of the split segments] (rnet_hip.h).  The partial offsets of both modes stay inside the partial region —
    the counters must never be written by a partial sum — and only segments with more than 512 rows of partials get slots."""
    lib = _C.lib()
    # a 160 x 160 stage-1 layer at batch 32: 6 400 rows of epilogue partials forward, the library's own chunking backward
    segs = [(819200, 256, 6400, 0)]
    p = _bn_problem(segs)
    need = lib.rn_bn_workspace_bytes(ctypes.byref(p))
    partial = 6400 * 2 * 256 * 4
    counters = 256 // 16 * 4
    slots = 256 // 16 * 25 * 256                       # 25 parts of 256 rows, 2 x 16 doubles each
    assert need == partial + 256 + slots, (need, partial, counters, slots)   # counters padded to 256 bytes
    # the five head levels: only the finest (1 600 rows of partials) is split
    head = [(32 * h * h, 256, 2 * -(-(32 * h * h) // 256), 0) for h in (80, 40, 20, 10, 5)]
    p = _bn_problem(head)
    need = lib.rn_bn_workspace_bytes(ctypes.byref(p))
    partial = sum(c * 2 * 256 * 4 for (_, _, c, _) in head)
    assert [c for (_, _, c, _) in head] == [1600, 400, 100, 26, 8]
    slots = 256 // 16 * 7 * 256                        # level 0: ceil(1600 / 256) = 7 parts
    assert need == (partial + 255) // 256 * 256 + 5 * 64 // 256 * 256 + 256 * (5 * 64 % 256 > 0) + slots
    for i in range(5):
        assert lib.rn_bn_partial_offset_bytes(ctypes.byref(p), i) < partial
        assert lib.rn_bn_bwd_partial_offset_bytes(ctypes.byref(p), i) < partial
    # a small layer: no slots, just the counters behind the partials of the mode that needs more of them (backward: the
    # library's own chunking, 200 chunks of 64 rows, against the 100 rows of epilogue partials forward)
    p = _bn_problem([(12800, 2048, 100, 0)])
    assert lib.rn_bn_workspace_bytes(ctypes.byref(p)) == 200 * 2 * 2048 * 4 + 2048 // 16 * 4
