#!/usr/bin/env python
"""Step time of the captured FlowNetS train step (batch 8, 384x512, split fp16: the trainer of bench.py --mode train) for
every optimiser, with and without per-tensor gradient clipping, against the Adam step of the same build -- the default
trainer, the step bench.py --mode train measures.  One process; every variant is captured and
warmed first, then the variants are timed in alternating rounds (device events around `--steps` replays each) and the
median round is reported, with the spread.  A record, not a threshold.  One JSON line on stdout.

  timeout -k 10 900 python tools/bench_optim.py [--steps 30 --rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flownet2-tf_amd"))
from src import _hip, weights as W  # noqa: E402
from src.trainer import FlowNetSTrainer  # noqa: E402

VARIANTS = [("adam", -1.0), ("adam", 1.0), ("sgd", -1.0), ("sgd", 1.0), ("momentum", -1.0), ("momentum", 1.0),
            ("adamw", -1.0), ("adamw", 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--dtype", default="f16x2", choices=["f32", "f16x2"])
    args = ap.parse_args()
    dev = _hip.require_device()
    rng = np.random.default_rng(0)
    n, h, w = args.batch, args.height, args.width
    a = torch.from_numpy(rng.random((n, h, w, 3), dtype=np.float32)).to(dev)
    b = torch.roll(a, (2, -3), (1, 2))
    gt = torch.from_numpy(np.clip(rng.standard_normal((n, h, w, 2)) * 5, -40, 40).astype(np.float32)).to(dev)
    wts = W.init_weights("FlowNetS", 1234)
    trainers = {}
    for kind, clip in VARIANTS:
        tr = FlowNetSTrainer(wts, n, h, w, dtype=args.dtype, optimizer=kind, clip_grad_norm=clip,
                             momentum=0.9 if kind == "momentum" else None)
        for _ in range(args.warmup):
            loss = tr.train_step(a, b, gt)
        torch.cuda.synchronize()
        if not np.isfinite(float(loss.item())):
            raise RuntimeError("%s: non-finite loss" % kind)
        trainers[(kind, clip)] = tr
    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for key, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                tr.train_step(a, b, gt)
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) / args.steps)
    base = float(np.median(times[("adam", -1.0)]))
    rows = []
    for (kind, clip), t in times.items():
        med = float(np.median(t))
        rows.append({"optimizer": kind, "clip": clip > 0, "step_ms": round(med, 4), "min_ms": round(min(t), 4),
                     "max_ms": round(max(t), 4), "vs_adam_ms": round(med - base, 4)})
    print(json.dumps({"what": "captured FlowNetS train step per optimiser", "batch": n, "size": [h, w], "dtype": args.dtype,
                      "steps": args.steps, "rounds": args.rounds, "unit": "ms per step (median of rounds)", "rows": rows}))


if __name__ == "__main__":
    main()
