"""Micro-benchmark of --enable_weights_info on the training engine's own arena (ResNet50-640: the engine's real segment and
block tables): rn_arena_stats and rn_arena_histogram against the two things they stand against, alternated in one process —
  vector_norm(P)        one torch.linalg.vector_norm over the whole arena: the same bytes read once, the streaming yardstick;
  per-variable .item()  the literal form of the reference, one torch.linalg.vector_norm(view).item() per variable: what the
                        feature replaces (host-synchronous, so its time is wall time around a device synchronise);
  weights_info()        TrainEngine.weights_info end to end, launches + the one device -> host copy + the host-side split.
Time per call (median and minimum over the rounds), bytes of P read, bytes/s.
python tools/bench_stats.py [--size 640] [--window 0.5] [--rounds 5] [--lib bf16|f16] [--freeze resnet_initial ...]"""
import argparse, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
import torch
from retinanet import _C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per measurement")
    ap.add_argument("--rounds", type=int, default=5, help="measurements per form, the forms alternated")
    ap.add_argument("--lib", default="bf16")
    ap.add_argument("--freeze", nargs="*", default=[], help="training.freeze_variables keys (default: everything trains)")
    a = ap.parse_args()
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    p = default_params(input_size=a.size, precision="mixed_float16" if a.lib == "f16" else "mixed_bfloat16")
    b = ModelBuilder(p, "train", device=dev)
    eng = TrainEngine(b(), 1, frozen_regexes=[b.FREEZE_VARS_REGEX[n] for n in a.freeze])
    lib, st = eng.lib, _C.current_stream()
    n = sum(size for _, size in eng.p_off.values())
    nseg, nblk, buckets = eng.n_segs, eng.n_blocks, 30
    ws = torch.empty((lib.rn_arena_stats_workspace_bytes(nblk, nseg),), dtype=torch.uint8, device=dev)
    stats = torch.zeros((nseg, 3), dtype=torch.float32, device=dev)
    bad = torch.zeros((nseg,), dtype=torch.int32, device=dev)
    counts = torch.zeros((nseg, buckets), dtype=torch.int32, device=dev)
    tables = (eng.segs_dev.data_ptr(), nseg, eng.block_seg_dev.data_ptr(), nblk)
    views = [eng._pview(k) for k in eng.train_names]

    def stats_call():
        _C.check(lib.rn_arena_stats(eng.P.data_ptr(), *tables, stats.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(), st),
                 "rn_arena_stats")

    def hist_call():
        _C.check(lib.rn_arena_histogram(eng.P.data_ptr(), *tables, stats.data_ptr(), buckets, counts.data_ptr(), st),
                 "rn_arena_histogram")

    # name -> (call, passes over P, synchronises on its own)
    calls = {"rn_arena_stats": (stats_call, 1, False),
             "rn_arena_histogram": (hist_call, 1, False),
             "vector_norm(P)": (lambda: torch.linalg.vector_norm(eng.P), 1, False),
             "per-variable .item()": (lambda: [torch.linalg.vector_norm(v).item() for v in views], 1, True),
             "weights_info()": (lambda: eng.weights_info(), 1, True),
             "weights_info(histogram)": (lambda: eng.weights_info(histogram=True), 2, True)}

    def timed(fn, host, reps):
        torch.cuda.synchronize()
        if host:                                          # every call ends in a device synchronise of its own
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3          # seconds per call

    stats_call()                                          # the min / max the histogram reads
    reps = {}
    for name, (fn, _, host) in calls.items():             # warm, and size the window
        timed(fn, host, 3)
        reps[name] = max(5, math.ceil(a.window / timed(fn, host, 10)))
    times = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, (fn, _, host) in calls.items():
            times[name].append(timed(fn, host, reps[name]))
    torch.cuda.synchronize()
    info = eng.weights_info(histogram=True)
    ref = torch.stack([torch.linalg.vector_norm(v.double()) for v in views]).cpu().numpy()
    err = max(abs(float(g) - float(r)) / float(r) for g, r in zip(info["norm"], ref) if r > 0)
    assert int(info["counts"].sum()) + int(info["nonfinite"].sum()) == n
    print(f"{n / 1e6:.1f} M parameters in {nseg} tensors, {nblk} blocks of {lib.rn_optim_chunk()}, {buckets} buckets, "
          f"build {a.lib}; worst norm error vs float64 {err:.2e}; every element counted once", flush=True)
    print(f"{'form':26s} {'calls':>6s} {'MB read':>8s} {'us (median)':>12s} {'us (min)':>9s} {'GB/s':>7s} {'vs vector_norm':>15s}")
    base = sorted(times["vector_norm(P)"])[len(times["vector_norm(P)"]) // 2]
    for name, (fn, passes, host) in calls.items():
        nbytes = 4 * n * passes
        t = sorted(times[name])
        med = t[len(t) // 2]
        print(f"{name:26s} {reps[name]:>6d} {nbytes / 1e6:8.1f} {med * 1e6:12.1f} {t[0] * 1e6:9.1f} {nbytes / med / 1e9:7.0f} "
              f"{med / base:15.2f}", flush=True)


if __name__ == "__main__":
    main()
