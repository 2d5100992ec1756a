"""Micro-benchmark of the FPN top-down launches at the training bench's geometry (batch 32, 640 x 640: levels 80 .. 5,
256 channels): the weighted FeatureFusion kernels (rn_fpn_topdown_fused, rn_fpn_fused_bwd_level + finalize) next to the
'sum' kernels (rn_fpn_topdown, rn_fpn_topdown_bwd_level) at the same shapes, alternating in one process.  Per launch:
time, algorithmic bytes from the shapes, and their rate as a fraction of the 8 TB/s HBM peak.
  forward bytes : every in[j] read, every out[j] (j < L - 1) written
  backward bytes: dout, out, in[j] read, the four-times-larger g_{j-1} read, the quarter-size out[j+1] read, g_j and
                  din written (the 'sum' level: dout, out, the finer din read, din written)
python tools/bench_fusion.py [--batch 32] [--size 640] [--rounds 5] [--iters 20] [--lib bf16|f16] [--mode fast_channel_attention]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
import torch
from retinanet import _C

PEAK_HBM_GBS = 8000.0


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def report(name, us_list, byts):
    us = sorted(us_list)[len(us_list) // 2]
    print(f"{name:34s} {us:8.1f} us (min {min(us_list):7.1f}, max {max(us_list):7.1f})  {byts / 1e6:7.1f} MB  "
          f"{byts / us / 1e3:6.0f} GB/s  {byts / us / 1e3 / PEAK_HBM_GBS:5.3f} of the HBM peak", flush=True)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", default="bf16")
    ap.add_argument("--mode", default="fast_channel_attention")
    ap.add_argument("--act", default="relu")
    a = ap.parse_args()
    lib = _C.lib(f16=(a.lib == "f16"))
    h16 = torch.float16 if a.lib == "f16" else torch.bfloat16
    dev = torch.device("cuda:0")
    st = _C.current_stream()
    N, C, L, H0 = a.batch, a.channels, 5, a.size // 8
    act, mode = _C.ACT_IDS[a.act], _C.FUSION_IDS[a.mode]
    shapes = [(N, H0 >> l, H0 >> l, C) for l in range(L)]
    ins = [torch.randn(s, device=dev).to(h16) for s in shapes]
    outs = [torch.empty_like(t) for t in ins[:-1]] + [ins[-1]]
    n = 1 if a.mode == "fast_attention" else C
    w = [(torch.rand((n,), device=dev) * 1.5 + 0.5, torch.rand((n,), device=dev) * 1.5 + 0.5) for _ in range(L - 1)]
    coef = [torch.empty((lib.rn_fpn_fusion_coef_bytes(C),), dtype=torch.uint8, device=dev) for _ in range(L - 1)]
    pin, pout = _C.ptr_array(ins), _C.ptr_array(outs)
    pwl, pwu, pco = _C.ptr_array([x[0] for x in w]), _C.ptr_array([x[1] for x in w]), _C.ptr_array(coef)
    nbytes = [t.numel() * 2 for t in ins]
    fwd_bytes = sum(nbytes) + sum(nbytes[:-1])

    def fwd_sum():
        _C.check(lib.rn_fpn_topdown(pin, pout, L, N, H0, H0, C, act, st), "rn_fpn_topdown")

    def fwd_fused():
        _C.check(lib.rn_fpn_topdown_fused(pin, pout, pwl, pwu, pco, L, N, H0, H0, C, act, mode, st), "rn_fpn_topdown_fused")

    print(f"batch {N}, {a.size} x {a.size}, C = {C}, {a.lib}, {a.mode}, act {a.act}; weighted forward: preparation kernel + "
          f"{lib.rn_fpn_topdown_fused_launches(L, N, H0, H0, C)} top-down launches")
    t_sum, t_fused = [], []
    for _ in range(a.rounds):
        t_sum.append(timed(fwd_sum, a.iters))
        t_fused.append(timed(fwd_fused, a.iters))
    s = report("forward  sum", t_sum, fwd_bytes)
    f = report("forward  " + a.mode, t_fused, fwd_bytes)
    print(f"forward  weighted / sum = {f / s:.2f}")

    douts = [torch.randn(s_, device=dev).to(h16) for s_ in shapes]
    dins = [torch.empty_like(t) for t in douts]
    gs = [torch.empty_like(t) for t in douts]
    for l in range(L):
        _, H, W, _ = shapes[l]
        top = l == L - 1
        finer = nbytes[l - 1] if l else 0
        sum_bytes = nbytes[l] * (2 if top else 3) + finer
        fused_bytes = nbytes[l] * 2 + finer if top else nbytes[l] * 5 + finer + nbytes[l + 1]
        a_sum = (douts[l].data_ptr(), dins[l - 1].data_ptr() if l else None, None if top else outs[l].data_ptr(),
                 dins[l].data_ptr(), N, H, W, C, _C.RN_ACT_NONE if top else act)
        if top:
            a_f = (douts[l].data_ptr(), gs[l - 1].data_ptr(), coef[l - 1].data_ptr(), None, None, None, None, None,
                   dins[l].data_ptr(), None, 0, N, H, W, C, _C.RN_ACT_NONE)
            fin = None
        else:
            ws = torch.empty((lib.rn_fpn_fused_bwd_workspace_bytes(N, H, W, C),), dtype=torch.uint8, device=dev)
            dw = torch.empty((2, n), dtype=torch.float32, device=dev)
            a_f = (douts[l].data_ptr(), gs[l - 1].data_ptr() if l else None, coef[l - 1].data_ptr() if l else None,
                   outs[l].data_ptr(), ins[l].data_ptr(), outs[l + 1].data_ptr(), coef[l].data_ptr(), gs[l].data_ptr(),
                   dins[l].data_ptr(), ws.data_ptr(), ws.numel(), N, H, W, C, act)
            fin = (ws.data_ptr(), ws.numel(), N, H, W, C, w[l][0].data_ptr(), w[l][1].data_ptr(), coef[l].data_ptr(), mode,
                   None, dw[0].data_ptr(), dw[1].data_ptr())
        b_sum = lambda a_sum=a_sum: _C.check(lib.rn_fpn_topdown_bwd_level(*a_sum, st), "bwd sum")
        b_fused = lambda a_f=a_f: _C.check(lib.rn_fpn_fused_bwd_level(*a_f, st), "bwd fused")
        t_sum, t_fused, t_fin = [], [], []
        for _ in range(a.rounds):
            t_sum.append(timed(b_sum, a.iters))
            t_fused.append(timed(b_fused, a.iters))
            if fin:
                t_fin.append(timed(lambda: _C.check(lib.rn_fpn_fused_bwd_finalize(*fin, st), "finalize"), a.iters))
        s = report(f"backward level {l} ({H:2d} x {W:2d}) sum", t_sum, sum_bytes)
        f = report(f"backward level {l} ({H:2d} x {W:2d}) weighted", t_fused, fused_bytes)
        if fin:
            report(f"backward level {l} finalize", t_fin, ws.numel())
        print(f"backward level {l} weighted / sum = {f / s:.2f}")


if __name__ == "__main__":
    main()
