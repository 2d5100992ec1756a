"""Within-process timing of the training step under training.freeze_variables key lists (run on the GPU box): one engine
per key list on the same model configuration, same weights and batch, timed in interleaved rounds; median ms / step.
A step with frozen layers launches a subset of the unfrozen step's backward work, so no row may be slower than `none`.

    python tools/bench_freeze.py --model efficientnet-b3 --keys "none;backbone"          # BASELINE configs[4], 32 images, f16
    python tools/bench_freeze.py --model resnet50 --keys "none;head;fpn,head"            # ResNet-50 at 640 x 640, 32 images
    [--size 640] [--batch 32] [--rounds 3] [--steps 5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--keys", default="none;head;fpn,head", help="key lists separated by ';', keys by ','; none = no freeze")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    from bench import synth_ground_truth
    from retinanet.cfg import default_params, efficientnet_params
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    gb, gc, cnt = [t.to(dev) for t in synth_ground_truth(a.batch, a.size, 1337)]
    images = torch.randn((a.batch, a.size, a.size, 3), generator=torch.Generator().manual_seed(1337)).to(dev)
    variants = a.keys.split(";")
    engs, encs = {}, {}
    for v in variants:
        keys = [] if v == "none" else v.split(",")
        if a.model.startswith("efficientnet"):
            params = efficientnet_params(a.model, input_size=a.size, batch_train=a.batch)
        else:
            params = default_params(input_size=a.size, batch_train=a.batch)
            params.architecture.backbone.depth = int(a.model[len("resnet"):])
        params.training.freeze_variables = keys
        builder = ModelBuilder(params, "train", device=dev, seed=1337)
        engs[v] = TrainEngine(builder(), a.batch, frozen_regexes=[builder.FREEZE_VARS_REGEX[k] for k in keys], world_size=1)
        encs[v] = LabelEncoder(params, device=dev)

    def step(v):
        return engs[v].train_step(images, encs[v].encode_batch(gb, gc, cnt))
    for v in variants:      # warm-up, and every variant must train
        for _ in range(2):
            out = step(v)
        torch.cuda.synchronize()
        assert np.isfinite(float(out["weighted-loss"].item())), v
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            step(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(v)
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / a.steps * 1e3)
    base = statistics.median(times[variants[0]])
    for v in variants:
        t, e = times[v], engs[v]
        print(f"{a.model} {a.size}x{a.size} B={a.batch} freeze={v:14s} median {statistics.median(t):7.3f} ms/step  min {min(t):7.3f}  "
              f"x{statistics.median(t) / base:5.3f} of {variants[0]}  ({len(e.train_names)} trainable variables, "
              f"{len(e.bwd_steps)} backward steps, {len(e.wgrad_launches) + len(e.dw_wgrad_launches)} weight-gradient launches)")


if __name__ == "__main__":
    main()
