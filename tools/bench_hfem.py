#!/usr/bin/env python
"""Step time of the FlowNetS_interp trainer (batch 8, 384x512, split fp16) through train_step in the three loss modes:
'' (plain AEPE), 'hard' (top 50 % EPE pixels of the batch) and 'edges'.  One process; every variant is built and warmed
first (which captures the step where the build can capture that mode), then the variants are timed in alternating rounds
(device events around `--steps` steps each) and the median round is reported, with the spread.  The file uses nothing but
FlowNetSTrainer(...).train_step(a, b, gt), so the same file runs on a build whose mining modes take the eager launch
sequence; each row says whether its step was captured.  Where train_step accepts an edge map the 'edges' variant gets one
(without it that mode is plain AEPE); the row says so.  A record, not a threshold.  One JSON line on stdout.

  timeout -k 10 600 python tools/bench_hfem.py [--steps 30 --rounds 5]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flownet2-tf_amd"))
from src import _hip, weights as W  # noqa: E402
from src.trainer import FlowNetSTrainer  # noqa: E402

MODES = ["", "hard", "edges"]


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
    gt_np = np.clip(rng.standard_normal((n, h, w, 2)) * 5, -40, 40).astype(np.float32)
    matches = (rng.random((n, h, w, 1)) < 0.05).astype(np.float32)
    # the tower's second input of FlowNetS_interp: [0.05 * sparse flow | matches]
    b = torch.from_numpy(np.concatenate([gt_np * matches * np.float32(0.05), matches], axis=3)).to(dev)
    gt = torch.from_numpy(gt_np).to(dev)
    edges = torch.from_numpy(rng.random((n, h, w, 1), dtype=np.float32)).to(dev)
    takes_edges = "edges" in inspect.signature(FlowNetSTrainer.train_step).parameters
    wts = W.init_weights("FlowNetS_interp", 1234)
    trainers = {}
    for mode in MODES:
        tr = FlowNetSTrainer(wts, n, h, w, dtype=args.dtype, model="FlowNetS_interp", add_hard_flow_mining=mode,
                             lambda_weight=2.0, hard_examples_perc=50)
        kw = {"edges": edges} if mode == "edges" and takes_edges else {}
        for _ in range(args.warmup):
            loss = tr.train_step(a, b, gt, **kw)
        torch.cuda.synchronize()
        if not np.isfinite(float(loss.item())):
            raise RuntimeError("%r: non-finite loss" % mode)
        trainers[mode] = (tr, kw)
    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for mode, (tr, kw) in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                tr.train_step(a, b, gt, **kw)
            e1.record()
            e1.synchronize()
            times[mode].append(e0.elapsed_time(e1) / args.steps)
    base = float(np.median(times[""]))
    rows = []
    for mode, t in times.items():
        med = float(np.median(t))
        tr, kw = trainers[mode]
        rows.append({"mode": mode, "captured": getattr(tr, "_step_graphs", None) is not None, "edge_map": bool(kw),
                     "step_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                     "vs_plain_ms": round(med - base, 4)})
    print(json.dumps({"what": "FlowNetS_interp train step per loss mode", "batch": n, "size": [h, w], "dtype": args.dtype,
                      "steps": args.steps, "rounds": args.rounds, "unit": "ms per step (median of rounds)", "rows": rows}))


if __name__ == "__main__":
    main()
