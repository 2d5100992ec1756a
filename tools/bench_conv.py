"""Micro-benchmark of rn_conv2d_nhwc_fwd on one (grouped) problem — used for A/B timing and
for short rocprofv3 PMC passes.  python tools/bench_conv.py --preset tower --batch 8 --iters 20"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
import torch  # noqa: E402

from retinanet import _C  # noqa: E402

PRESETS = {
    # name: (list of (H, Cin, Cout) segments, k, stride, out_f32, residual)
    "tower": ([(s, 256, 256) for s in (80, 40, 20, 10, 5)] * 2, 3, 1, False, False),
    "tower_1x1": ([(s, 256, 256) for s in (80, 40, 20, 10, 5)] * 2, 1, 1, False, False),
    "tower_c64": ([(s, 64, 256) for s in (80, 40, 20, 10, 5)] * 2, 1, 1, False, False),
    "pred_class": ([(s, 256, 720) for s in (80, 40, 20, 10, 5)], 3, 1, True, False),
    "pred_class_bf16": ([(s, 256, 720) for s in (80, 40, 20, 10, 5)], 3, 1, False, False),
    "pred_768": ([(s, 256, 768) for s in (80, 40, 20, 10, 5)], 3, 1, True, False),
    "pred_768_bf16": ([(s, 256, 768) for s in (80, 40, 20, 10, 5)], 3, 1, False, False),
    "pred_box": ([(s, 256, 36) for s in (80, 40, 20, 10, 5)], 3, 1, True, False),
    "tower1": ([(s, 256, 256) for s in (80, 40, 20, 10, 5)], 3, 1, False, False),
    "g1_3x3": ([(160, 64, 64)], 3, 1, False, False),
    "g1_out": ([(160, 64, 256)], 1, 1, False, True),
    "g1_a": ([(160, 256, 64)], 1, 1, False, False),
    "g1_sc": ([(160, 64, 256)], 1, 1, False, False),
    "g2_out": ([(80, 128, 512)], 1, 1, False, True),
    "g2_a": ([(80, 512, 128)], 1, 1, False, False),
    "g3_a": ([(40, 1024, 256)], 1, 1, False, False),
    "g2_3x3": ([(80, 128, 128)], 3, 1, False, False),
    "g3_3x3": ([(40, 256, 256)], 3, 1, False, False),
    "g3_out": ([(40, 256, 1024)], 1, 1, False, True),
    "g4_3x3": ([(20, 512, 512)], 3, 1, False, False),
    "g4_a": ([(20, 2048, 512)], 1, 1, False, False),
    "g4_out": ([(20, 512, 2048)], 1, 1, False, True),
    # EfficientNet-B3 MBConv 1x1 layers (expand / project), batch 32 at 640^2
    "e_exp160": ([(160, 32, 192)], 1, 1, False, False),
    "e_exp80": ([(80, 48, 288)], 1, 1, False, False),
    "e_exp40": ([(40, 136, 816)], 1, 1, False, False),
    "e_exp20": ([(20, 232, 1392)], 1, 1, False, False),
    "e_proj80": ([(80, 288, 48)], 1, 1, False, True),
    "e_proj40": ([(40, 816, 136)], 1, 1, False, True),
    "e_proj20": ([(20, 1392, 232)], 1, 1, False, True),
    "g3_sc": ([(40, 512, 1024)], 1, 1, False, False),
    # pixel-pair forms of the narrow 1x1 layers (run at HALF the batch: the same bytes as the plain layer at the full one)
    "g2_a_pair": ([(80, 1024, 256)], 1, 1, False, False),
    "g2b0_a": ([(160, 256, 128)], 1, 1, False, False),
    "g2b0_a_pair": ([(160, 512, 256)], 1, 1, False, False),
    "g1_a_pair": ([(160, 512, 128)], 1, 1, False, False),
    "fpn_out": ([(s, 256, 256) for s in (80, 40, 20, 10, 5)], 3, 1, False, False),
    "fpn_lat": ([(80, 512, 256), (40, 1024, 256), (20, 2048, 256)], 1, 1, False, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="tower")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--zeros", action="store_true", help="all-zero activations and weights (DVFS check: no toggling)")
    ap.add_argument("--halo-grid", type=int, default=0, help="limit conv_halo_kernel to this many workgroups")
    ap.add_argument("--raw", action="store_true", help="no scale / shift / activation (the training forward's raw conv output)")
    ap.add_argument("--bias", action="store_true", help="shift only (bias + relu: the head towers)")
    ap.add_argument("--no-halo", action="store_true", help="3x3 launches on conv_big_kernel instead of conv_halo_kernel")
    ap.add_argument("--tile", type=int, default=0, help="1 = force 128-row kernel, 2 = force the 256x256 kernel, 3 = force 512x128 halo tiles")
    ap.add_argument("--splitk", action="store_true", help="attach a split-K workspace (rn_conv_problem.splitk_ws)")
    ap.add_argument("--min-tiles", type=int, default=0, help="rn_launch_opts.conv_big_min_tiles (a large value keeps a small launch on the 128-row kernel, split-K allowed)")
    a = ap.parse_args()
    lib = _C.lib()
    opts = _C.LaunchOpts(conv_tile=a.tile or 0, conv_no_halo=1 if a.no_halo else 0,
                         max_workgroups=a.halo_grid or 0, conv_big_min_tiles=a.min_tiles or 0)   # rn_launch_opts of every launch below
    dev = torch.device("cuda:0")
    for name in a.preset.split(","):
        segs, k, stride, f32, use_res = PRESETS[name]
        p = _C.ConvProblem()
        p.opts = opts
        p.R = p.S = k
        p.stride_h = p.stride_w = stride
        p.pad_top = p.pad_left = (k - 1) // 2
        p.act, p.out_dtype, p.num_segments = (_C.RN_ACT_NONE if a.raw else _C.RN_ACT_RELU), (_C.RN_DT_F32 if f32 else _C.RN_DT_BF16), len(segs)
        keep, flops, byts = [], 0, 0
        for i, (H, cin, cout) in enumerate(segs):
            x = torch.randn((a.batch, H, H, cin), device=dev).to(torch.bfloat16)
            w = (torch.randn((lib.rn_conv_cout_pad(cout), k, k, cin), device=dev) / (k * k * cin) ** 0.5).to(torch.bfloat16)
            if a.zeros:
                x.zero_(); w.zero_()
            Ho = (H + 2 * p.pad_top - k) // stride + 1
            y = torch.empty((a.batch, Ho, Ho, cout), dtype=torch.float32 if f32 else torch.bfloat16, device=dev)
            sc = torch.rand((cout,), device=dev) + 0.5
            sh = torch.randn((cout,), device=dev)
            res = torch.randn((a.batch, Ho, Ho, cout), device=dev).to(torch.bfloat16) if use_res else None
            s = p.seg[i]
            s.x, s.w, s.y, s.scale, s.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr()
            if a.raw:
                s.scale, s.shift = None, None
            if a.bias:   # Conv2D + bias (the head towers): the bias is the accumulators' initial value
                s.scale, s.shift, s.bias = None, None, sh.data_ptr()
            s.residual = res.data_ptr() if use_res else None
            s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = a.batch, H, H, cin, cin, Ho, Ho, cout
            keep += [x, w, y, sc, sh, res]
            flops += 2 * a.batch * Ho * Ho * k * k * cin * cout
            byts += x.numel() * 2 + y.numel() * y.element_size() + (res.numel() * 2 if use_res else 0) + k * k * cin * cout * 2
        if a.splitk:
            ws = torch.zeros((int(lib.rn_conv_splitk_workspace_max_bytes()),), dtype=torch.uint8, device=dev)
            p.splitk_ws, p.splitk_ws_bytes = ws.data_ptr(), ws.numel()
            keep.append(ws)
            print(f"  kernel id {lib.rn_conv_kernel_id(ctypes.byref(p))}, split workspace {lib.rn_conv_splitk_workspace_bytes(ctypes.byref(p))} bytes")
        st = _C.current_stream()
        for _ in range(3):
            _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), st))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), st))
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        if hasattr(lib, "rn_debug_halo_clocks"):     # probe builds: core clock of workgroup 0 during the last launch
            clk = (ctypes.c_ulonglong * 48)()
            if lib.rn_debug_halo_clocks(clk) == 0 and clk[3] > clk[1]:
                cyc, wall = clk[2] - clk[0], (clk[3] - clk[1]) / 100.0   # wall clock ticks at 100 MHz -> us
                print(f"  workgroup 0: {cyc} core cycles in {wall:.1f} us -> {cyc / wall / 1e3:.3f} GHz; "
                      f"cycles per slot in passes 2-4 of tile 0: {[round((clk[5 + i] - clk[4 + i]) / 18) for i in range(3)]}; "
                      f"2nd tile: epilogue {clk[9] - clk[8]} cycles, + set-up {int(clk[11]) - int(clk[9])}, + load segment {int(clk[10]) - int(clk[11])}, "
                      f"cycles per slot in passes 0..8 of the first tile (the 9th is the next tile's first): {[round((int(clk[23 + i]) - int(clk[22 + i])) / 18) for i in range(9)]}; "
                      f"inside (entry, then per 32-pixel block: transposes | read-back + stores): "
                      f"{[int(clk[k + 1] - clk[k]) for k in range(12, 21)]}; first in-loop pixel set-up "
                      f"{int(clk[33]) - int(clk[32])} cycles, weight set-up {int(clk[35]) - int(clk[34])}")
        print(f"{name:12s} B={a.batch} {ms * 1e3:9.1f} us  {flops / ms / 1e9:8.1f} TFLOP/s  "
              f"{byts / ms / 1e6:8.1f} GB/s (algorithmic {byts / 1e6:.1f} MB)", flush=True)


if __name__ == "__main__":
    main()
