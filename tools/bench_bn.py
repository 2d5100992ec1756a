"""Micro-benchmark of the training BatchNorm passes on EfficientNet-B3's swish layers (batch 32, IEEE-half build) or, with
--shapes resnet50, on ResNet-50's largest BatchNorm geometries at 640 x 640 (relu, bfloat16 build):
rn_bn_stats_finalize, rn_bn_apply, rn_bn_bwd_reduce, rn_bn_bwd_apply and rn_bn_frozen_bwd (the whole backward of a frozen
BatchNorm, on the same tensors with the same scale / shift table; relu / relu6: with the gate bits the engine gives such a
layer) — time per launch and GB/s of algorithmic bytes.  The yardstick `copy` is a pass that does nothing: a device copy of
one tensor of the shape (one read, one write); `frozen/copy` is the frozen pass's time over the copy's, scaled to the
frozen pass's algorithmic bytes, `frozen/live` its time over rn_bn_bwd_apply's in the same run.
python tools/bench_bn.py [--shapes effnet-b3|resnet50] [--batch 32] [--act swish] [--lib f16|bf16]"""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
import torch
from retinanet import _C

SHAPES = [(320, 40), (320, 144), (160, 144), (160, 192), (80, 192), (80, 288), (40, 288), (40, 576), (40, 816), (20, 816),
          (20, 1392), (20, 2304)]
# stem, the 64 / 256-channel layers of stage 1, the 128 / 512 of stage 2, 256 / 1024 of stage 3, and the head towers' level 3
RESNET50_SHAPES = [(320, 64), (160, 64), (160, 256), (80, 128), (80, 512), (40, 256), (40, 1024), (80, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="effnet-b3", choices=["effnet-b3", "resnet50"])
    ap.add_argument("--act", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    a.act = a.act or ("swish" if a.shapes == "effnet-b3" else "relu")
    a.lib = a.lib or ("f16" if a.shapes == "effnet-b3" else "bf16")
    lib = _C.lib(f16=(a.lib == "f16"))
    h16 = torch.float16 if a.lib == "f16" else torch.bfloat16
    dev = torch.device("cuda:0")
    st = _C.current_stream()
    for H, C in (SHAPES if a.shapes == "effnet-b3" else RESNET50_SHAPES):
        N = a.batch
        y = (torch.randn((N, H, H, C), device=dev) * 2 + 0.5).to(h16)
        dz = torch.randn((N, H, H, C), device=dev).to(h16)
        z, dy = torch.empty_like(y), torch.empty_like(y)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        keep = dict(sums=f32(2, C), bsums=f32(2, C), fwd=f32(4, C), gamma=f32(C) + 1, beta=f32(C), mm=f32(C), mv=f32(C) + 1,
                    dg=f32(C), db=f32(C))
        p = _C.BnProblem()
        p.num_segments, p.act, p.bessel, p.eps, p.momentum, p.count_scale = 1, _C.ACT_IDS[a.act], 1, 1e-3, 0.99, 1.0
        g = p.seg[0]
        g.y, g.z, g.dz, g.dy = y.data_ptr(), z.data_ptr(), dz.data_ptr(), dy.data_ptr()
        g.sums, g.bsums, g.fwd = keep["sums"].data_ptr(), keep["bsums"].data_ptr(), keep["fwd"].data_ptr()
        g.gamma, g.beta, g.moving_mean, g.moving_var = (keep["gamma"].data_ptr(), keep["beta"].data_ptr(),
                                                        keep["mm"].data_ptr(), keep["mv"].data_ptr())
        g.dgamma, g.dbeta = keep["dg"].data_ptr(), keep["db"].data_ptr()
        g.P, g.C, g.dres_accumulate = N * H * H, C, 0
        ws = torch.zeros((lib.rn_bn_workspace_bytes(ctypes.byref(p)),), dtype=torch.uint8, device=dev)
        # the frozen pass: the same tensors and table, plus the gate bits of a relu / relu6 layer (rn_bn_apply fills them)
        pf = _C.BnProblem.from_buffer_copy(p)
        mask = None
        if a.act in ("relu", "relu6"):
            mask = torch.zeros((y.numel() // 8,), dtype=torch.uint8, device=dev)
            pf.seg[0].act_mask = mask.data_ptr()
        n = y.numel() * 2
        frozen_bytes = 2 * n + (n // 16 if mask is not None else n if a.act == "swish" else 0)
        calls = [("stats", lambda: lib.rn_bn_stats_finalize(ctypes.byref(p), _C.ptr(ws), ws.numel(), st), 1),
                 ("apply", lambda: lib.rn_bn_apply(ctypes.byref(p), st), 2),
                 ("bwd_reduce", lambda: lib.rn_bn_bwd_reduce(ctypes.byref(p), _C.ptr(ws), ws.numel(), st), 2),
                 ("bwd_apply", lambda: lib.rn_bn_bwd_apply(ctypes.byref(p), st), 3),
                 ("fill_bits", lambda: lib.rn_bn_apply(ctypes.byref(pf), st), None),
                 ("frozen_bwd", lambda: lib.rn_bn_frozen_bwd(ctypes.byref(pf), st), frozen_bytes / n),
                 ("copy", lambda: (dy.copy_(dz), 0)[1], 2)]
        line = f"{H:3d}x{H:<3d} C={C:4d} ({y.numel() * 2 / 1e6:6.0f} MB)"
        took = {}
        for name, fn, tensors in calls:
            if tensors is None:       # not timed: the forward pass of the frozen problem, once, for the gate bits
                _C.check(fn(), name)
                continue
            for _ in range(2):
                _C.check(fn(), name)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                _C.check(fn(), name)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / a.iters * 1e3
            took[name] = us
            line += f"  {name} {us:7.1f} us {tensors * y.numel() * 2 / us / 1e3:5.0f} GB/s"
        line += (f"  frozen/copy {took['frozen_bwd'] / (took['copy'] * frozen_bytes / (2 * n)):.2f}"
                 f"  frozen/live {took['frozen_bwd'] / took['bwd_apply']:.2f}")
        print(line, flush=True)


if __name__ == "__main__":
    main()
