"""Time of one optimizer step over N micro-batches (TrainEngine.train_step_accumulated) against N plain steps at the
micro-batch size (TrainEngine.train_step), with HIP events around each group of N: ResNet50 RetinaNet, bf16, one GPU, the
benchmark's synthetic data.  The two modes are separate runs (`--plain` also runs on a commit without the feature);
alternate them on one box and compare the medians with the spread of the repeats.
python tools/bench_accumulated_step.py [--plain] [--steps 4] [--micro-batch 8] [--size 640] [--groups 12] [--warmup 3]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
sys.path.insert(0, ROOT)
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", action="store_true", help="N plain train_steps at the micro-batch size, no accumulation")
    ap.add_argument("--steps", type=int, default=4, help="N: micro-batches per optimizer step")
    ap.add_argument("--micro-batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--groups", type=int, default=12, help="timed groups of N micro-batches")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from bench import synth_ground_truth
    from retinanet.cfg import default_params
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    N, B = a.steps, a.micro_batch
    p = default_params(input_size=a.size, batch_train=B * N)
    builder = ModelBuilder(p, "train", device=dev, seed=1337)
    model = builder()
    rx = [builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables]
    kw = {} if a.plain else {"accumulation_steps": N}
    eng = TrainEngine(model, B, frozen_regexes=rx, world_size=1, **kw)
    enc = LabelEncoder(p, device=dev)
    data = []
    for i in range(N):
        gb, gc, cnt = [t.to(dev) for t in synth_ground_truth(B, a.size, 1337 + i)]
        images = torch.randn((B, a.size, a.size, 3), generator=torch.Generator().manual_seed(1337 + i)).to(dev)
        data.append((images, gb, gc, cnt))

    def group():
        batches = [(images, enc.encode_batch(gb, gc, cnt)) for images, gb, gc, cnt in data]
        if a.plain:
            for images, targets in batches:
                out = eng.train_step(images, targets)
            return out
        return eng.train_step_accumulated(batches)

    for _ in range(a.warmup):
        out = group()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = group()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    t = sorted(times)
    print(json.dumps({"mode": "plain" if a.plain else "accumulated", "N": N, "micro_batch": B, "size": a.size,
                      "optimizer_steps": eng.step_count, "ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3),
                      "ms_max": round(t[-1], 3), "groups": a.groups, "total_loss": round(float(out["total-loss"]), 5)}))


if __name__ == "__main__":
    main()
