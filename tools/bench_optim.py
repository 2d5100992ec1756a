"""Micro-benchmark of the optimizer step kernels on the training engine's own arenas (ResNet50-640: the engine's real
segment and block tables): every mode of rn_optim_step, alternated in one process — time per launch,
algorithmic bytes (arrays read + written) and bytes/s.  `accumulate`: the accumulate stage of gradient accumulation
(rn_optim_clip_apply_accumulate: 12 bytes per element, 8 with `first`) alternated with the SGD rule of rn_optim_step.
python tools/bench_optim.py [rules|accumulate] [--size 640] [--window 0.25] [--rounds 3] [--lib bf16|f16] [--no-ema]"""
import argparse, ctypes, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
import torch
from retinanet import _C

# mode -> (rule, flags, fp32 arrays read, fp32 arrays written) without the moving average (one more each with it);
# `sgd` comes first: it is the base of the "vs sgd" column
MODES = {"sgd": (_C.RN_OPT_SGD, 0, 3, 2), "sgd+nesterov": (_C.RN_OPT_SGD, _C.RN_OPT_NESTEROV, 3, 2),
         "adam": (_C.RN_OPT_ADAM, 0, 4, 3), "adam+amsgrad": (_C.RN_OPT_ADAM, _C.RN_OPT_AMSGRAD, 5, 4),
         "rmsprop": (_C.RN_OPT_RMSPROP, 0, 3, 2), "rmsprop+momentum": (_C.RN_OPT_RMSPROP, _C.RN_OPT_MOMENTUM, 4, 3),
         "rmsprop+centered": (_C.RN_OPT_RMSPROP, _C.RN_OPT_CENTERED, 4, 3),
         "rmsprop+centered+momentum": (_C.RN_OPT_RMSPROP, _C.RN_OPT_CENTERED | _C.RN_OPT_MOMENTUM, 5, 4),
         "adagrad": (_C.RN_OPT_ADAGRAD, 0, 3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="rules", choices=["rules", "accumulate"])
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per measurement")
    ap.add_argument("--rounds", type=int, default=3, help="measurements per mode, the modes alternated")
    ap.add_argument("--lib", default="bf16")
    ap.add_argument("--no-ema", action="store_true")
    a = ap.parse_args()
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    p = default_params(input_size=a.size, precision="mixed_float16" if a.lib == "f16" else "mixed_bfloat16")
    b = ModelBuilder(p, "train", device=dev)
    eng = TrainEngine(b(), 1, frozen_regexes=[b.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables])
    lib, st = eng.lib, _C.current_stream()
    n = sum(size for _, size in eng.p_off.values())
    n16 = sum(size for (_, size), _ in eng._bf_copies)
    ema = not a.no_ema
    S1, S2 = torch.zeros_like(eng.P), torch.zeros_like(eng.P)
    eng.G.copy_(torch.randn_like(eng.G) * 1e-3)
    eng.G[:4] = 0.0
    args = (eng.Pbf.data_ptr(), eng.segs_dev.data_ptr(), eng.block_seg_dev.data_ptr(), eng.n_blocks)
    E = eng.E.data_ptr() if ema else None

    def rule_call(rule, flags):
        r = _C.OptimRule(rule=rule, flags=flags, lr=1e-6, beta1=0.9, beta2=0.999, rho=0.9, momentum=0.9, epsilon=1e-7,
                         ema_decay=0.9998)
        return lambda: lib.rn_optim_step(eng.P.data_ptr(), eng.G.data_ptr(), eng.V.data_ptr(), S1.data_ptr(), S2.data_ptr(),
                                         E, *args, ctypes.byref(r), None, st)

    # name -> (launch, fp32 arrays read, written, "a rule of rn_optim_step": the moving average and the 16-bit copy come on top)
    calls = {name: (rule_call(rule, flags), rd, wr, True) for name, (rule, flags, rd, wr) in MODES.items()}
    if a.what == "accumulate":
        acc = torch.zeros_like(eng.G)
        ws = (eng.opt_ws.data_ptr(), eng.opt_ws.numel())
        # stages 1 and 2 once: the factors the timed stage reads (a clip that fires: the stage has no branch on them)
        _C.check(lib.rn_optim_clip_accumulate(eng.G.data_ptr(), eng.P.data_ptr(), acc.data_ptr(), 1, eng.segs_dev.data_ptr(),
                                              eng.n_segs, eng.block_seg_dev.data_ptr(), eng.n_blocks, 0.0, 0.0, 1.0, 1e-3,
                                              eng.metrics.data_ptr(), *ws, st), "rn_optim_clip_accumulate")

        def accumulate_call(first):
            return lambda: lib.rn_optim_clip_apply_accumulate(eng.G.data_ptr(), acc.data_ptr(), first, eng.metrics.data_ptr(),
                                                              eng.segs_dev.data_ptr(), eng.block_seg_dev.data_ptr(),
                                                              eng.n_blocks, *ws, st)
        calls = {"sgd": calls["sgd"], "accumulate": (accumulate_call(0), 2, 1, False),
                 "accumulate first": (accumulate_call(1), 1, 1, False)}

    def timed(fn, name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            _C.check(fn(), name)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3          # seconds per launch

    reps = {}
    for name, (fn, _, _, _) in calls.items():             # warm, and size the window
        timed(fn, name, 5)
        reps[name] = max(10, math.ceil(a.window / timed(fn, name, 20)))
        eng.V.fill_(0.1)                                  # a state every rule can continue from
        S1.zero_(), S2.fill_(0.1)
    times = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, (fn, _, _, _) in calls.items():
            times[name].append(timed(fn, name, reps[name]))
            eng.V.fill_(0.1)
            S1.zero_(), S2.fill_(0.1)
    print(f"{n / 1e6:.1f} M parameters in {eng.n_segs} tensors, {eng.n_blocks} blocks, {n16 / 1e6:.1f} M 16-bit copies, "
          f"moving average {'on' if ema else 'off'}, build {a.lib}", flush=True)
    print(f"{'mode':28s} {'arrays r+w':>10s} {'MB':>8s} {'us (median)':>12s} {'us (min)':>9s} {'GB/s':>7s} {'vs sgd':>7s}")
    base = None
    for name, (fn, rd, wr, rule) in calls.items():
        if rule:
            rd, wr = rd + (1 if ema else 0), wr + (1 if ema else 0)
        nbytes = 4 * n * (rd + wr) + (2 * n16 if rule else 0)
        t = sorted(times[name])
        med = t[len(t) // 2]
        gbs = nbytes / med / 1e9
        base = gbs if base is None else base
        print(f"{name:28s} {rd:>6d}+{wr:<3d} {nbytes / 1e6:8.1f} {med * 1e6:12.1f} {t[0] * 1e6:9.1f} {gbs:7.0f} {gbs / base:7.2f}",
              flush=True)


if __name__ == "__main__":
    main()
