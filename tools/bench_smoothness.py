#!/usr/bin/env python
"""The edge-aware smoothness term, timed two ways in one process.  A record, not a threshold.

1. The launch (fn2_smoothness_loss_grad, accumulate = 1 as the trainer calls it) on one table of FlowNetS's five loss scales
   for batch 8 at 384x512, both orders, device events around `--inner` back-to-back launches, median of `--rounds`.  The
   predictions are a smooth flow of a few pixels plus noise, the frames random; all buffers together are a few MB and stay
   in the caches between launches, so these are cache-warm times.  `bytes` is what the algorithm moves once (every flow and
   frame read once, every gradient read and written once), computed from the shapes; the neighbour taps a pixel re-reads
   are cache traffic and not counted.
2. The captured unsupervised step with smoothness_weight 0 (what the step was before the term existed) and with a weight,
   per order, in alternating rounds of `--steps` steps: `added_ms` is the difference of the medians.

  timeout -k 10 600 python tools/bench_smoothness.py [--steps 30 --rounds 5 --dtype f16x2]

One JSON line on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flownet2-tf_amd"))
from src import _hip, weights as W  # noqa: E402
from src.trainer import LOSS_WEIGHTS, FlowNetSTrainer  # noqa: E402


def timed(fn, rounds, inner):
    """[ms per call] over `rounds` windows of `inner` calls."""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return out


def row(name, t, **kw):
    return dict(name=name, ms=round(float(np.median(t)), 5), min_ms=round(min(t), 5), max_ms=round(max(t), 5), **kw)


def op_rows(args, dev):
    n, H, Wd = args.batch, args.height, args.width
    lib, rng = _hip.lib(), np.random.default_rng(0)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    levels, keep, pix = [], [], 0
    for lvl in (6, 5, 4, 3, 2):
        h, w = H >> lvl, Wd >> lvl
        scale = 20.0 * w / Wd
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        flow = np.stack([1.5 * np.sin(yy / 7.0) + 0.8, 1.2 * np.cos(xx / 9.0) - 0.5], -1)[None]       # level pixels
        flow = flow + 0.05 * rng.standard_normal((n, h, w, 2))
        pred = torch.from_numpy((flow / scale).astype(np.float32)).to(dev)
        img = torch.from_numpy(rng.random((n, h, w, 3), dtype=np.float32)).to(dev)
        dpred = torch.zeros_like(pred)
        keep += [pred, img, dpred]
        levels.append(_hip.Fn2PhotometricLevel(pred.data_ptr(), img.data_ptr(), None, None, dpred.data_ptr(), h, w, scale,
                                               LOSS_WEIGHTS[lvl] / 5.0))
        pix += n * h * w
    table = (_hip.Fn2PhotometricLevel * 5)(*levels)
    rows = []
    for order in (1, 2):
        def launch():
            _hip.check(lib.fn2_smoothness_loss_grad(table, 5, n, order, 150.0, 1e-3, 1.0, 1.0, 1, _hip.ptr(loss),
                                                    _hip.stream_ptr()))
        launch()
        torch.cuda.synchronize()
        if not np.isfinite(float(loss.item())):
            raise RuntimeError("non-finite loss")
        rows.append(row("fn2_smoothness_loss_grad order %d (accumulate)" % order, timed(launch, args.rounds, args.inner),
                        bytes=int(pix * (8 + 12 + 8 + 8))))
    return rows


def step_rows(args, dev):
    n, h, w = args.batch, args.height, args.width
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.random((n // 2, h, w, 3), dtype=np.float32)).to(dev)
    b = torch.roll(a, (2, -3), (1, 2))
    wts = W.init_weights("FlowNetS", 1234)
    make = lambda **kw: FlowNetSTrainer(wts, n, h, w, dtype=args.dtype, unsupervised=True, **kw)
    trainers = {"weight 0": make(), "order 1": make(smoothness_weight=1.0, smoothness_order=1),
                "order 2": make(smoothness_weight=1.0, smoothness_order=2)}
    for tr in trainers.values():
        for _ in range(args.warmup):
            loss = tr.train_step_unsupervised(a, b)
        torch.cuda.synchronize()
        if not np.isfinite(float(loss.item())):
            raise RuntimeError("non-finite loss")
    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for k, tr in trainers.items():
            times[k] += timed(lambda: tr.train_step_unsupervised(a, b), 1, args.steps)
    base = float(np.median(times["weight 0"]))
    return [row("unsupervised step, smoothness %s (captured: %s)" % (k, getattr(tr, "_step_graphs", None) is not None),
                times[k], added_ms=round(float(np.median(times[k])) - base, 5)) for k, tr in trainers.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--dtype", default="f16x2", choices=["f32", "f16x2"])
    args = ap.parse_args()
    dev = _hip.require_device()
    print(json.dumps({"what": "smoothness term: the launch alone, and the captured unsupervised step without and with it",
                      "batch": args.batch, "size": [args.height, args.width], "dtype": args.dtype, "cache_warm": True,
                      "unit": "ms (median of rounds)", "ops": op_rows(args, dev), "steps": step_rows(args, dev)}))


if __name__ == "__main__":
    main()
