"""INT8 detection heads against the bf16 engine, in ONE process (DESIGN.md "INT8 serving").

For every batch size: the bf16 InferenceEngine and the INT8 one (heads on rn_conv3x3_i8_fwd, calibrated here on seeded
synthetic batches) of the same model,
  * graph-replay ms of the whole forward pass, the two engines alternating round by round;
  * per-launch us of the head launches of both (each launch alone on the stream, events around `reps` back-to-back runs);
  * fidelity: max / mean absolute deviation of the class logits and box regressions, INT8 against bf16, on a batch the
    calibration did not see, once per calibration method.
--pred-scale S multiplies the class-prediction kernel by S first (the logit spread of a trained detector: the round-6
measurement of tools/ab_pred_planes.py used 7).  One JSON document on stdout.
Usage (GPU box): python tools/bench_int8.py [--depth 50] [--size 640] [--batches 8,1] [--pred-scale 7]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
import torch  # noqa: E402


def replay_ms(eng, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def head_launch_us(eng, reps):
    from retinanet import _C
    out = {}
    st = _C.current_stream()
    for fn, name in eng.steps:
        if not (name.startswith(("conv_i8:", "quantize_i8:")) or (name.startswith("conv:") and ("tower" in name or "pred_" in name))):
            continue
        fn(st)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(st)
        e1.record()
        torch.cuda.synchronize()
        out[name] = round(e0.elapsed_time(e1) / reps * 1e3, 2)
    out["total"] = round(sum(out.values()), 2)
    return out


def deviation(a, b):
    res = {}
    for key in ("class-predictions", "box-predictions"):
        d = torch.cat([(a[key][lv].double() - b[key][lv].double()).abs().reshape(-1) for lv in a[key]])
        ref = torch.cat([b[key][lv].double().reshape(-1) for lv in b[key]])
        res[key] = {"max_abs": d.max().item(), "mean_abs": d.mean().item(), "std_of_reference": ref.std().item()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", default="8,1")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calibration-batches", type=int, default=2)
    ap.add_argument("--pred-scale", type=float, default=7.0)
    a = ap.parse_args()
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.quantization import Calibrator
    dev = torch.device("cuda:0")
    p = default_params(input_size=a.size)
    p.architecture.backbone.depth = a.depth
    model = ModelBuilder(p, "val", device=dev, seed=1337)()
    if a.pred_scale != 1.0:
        model.variables["class-head/class-head-prediction-conv2d/kernel"].mul_(a.pred_scale)
    out = {"depth": a.depth, "size": a.size, "pred_scale": a.pred_scale, "batches": {}}
    for B in [int(v) for v in a.batches.split(",")]:
        gen = torch.Generator().manual_seed(1337 + B)
        batches = [torch.randn((B, a.size, a.size, 3), generator=gen).to(dev) for _ in range(a.calibration_batches)]
        x = torch.randn((B, a.size, a.size, 3), generator=gen).to(dev)
        eng16 = model.inference_engine(B, capture_graph=True)
        tables = {m: Calibrator(model.inference_engine(B), m).run(batches) for m in ("minmax", "entropy")}
        res = {"fidelity": {}}
        ref = {k: {lv: t.clone() for lv, t in d.items()} for k, d in eng16(x).items()}
        engs8 = {m: model.inference_engine(B, capture_graph=True, quantization=t) for m, t in tables.items()}
        for m, eng in engs8.items():
            res["fidelity"][m] = deviation(eng(x), ref)
        eng8 = engs8["entropy"]
        for eng in (eng8, eng16):
            replay_ms(eng, x, 5)
        times = {"int8": [], "bf16": []}
        for _ in range(a.rounds):
            times["int8"].append(round(replay_ms(eng8, x, a.iters), 4))
            times["bf16"].append(round(replay_ms(eng16, x, a.iters), 4))
        res["graph_replay_ms"] = times
        res["head_launch_us"] = {"int8": head_launch_us(eng8, a.reps), "bf16": head_launch_us(eng16, a.reps)}
        out["batches"][str(B)] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
