#!/usr/bin/env python
"""The ternary census data term, timed two ways in one process.  A record, not a threshold.

1. The three launches (fn2_census_warp, fn2_census_cost, fn2_census_grad) on one table of FlowNetS's five loss scales for
   batch 8 at 384x512 (the 6 x 8 scale is in the table: it has no interior and costs its tiles' staging only), device
   events around `--inner` back-to-back launches, median of `--rounds`.  The predictions are a smooth flow of a few pixels
   plus noise, the frames random, the mask all ones; all buffers together are a few MB and stay in the caches between
   launches, so these are cache-warm times.
2. The captured unsupervised step with data_term='census' next to the one with data_term='photometric' (FlowNetS, same
   batch, size, dtype and weights), in alternating rounds of `--steps` steps, and the loss stage of either alone on the
   trainer's own buffers outside the graph.

  timeout -k 10 600 python tools/bench_census.py [--steps 30 --rounds 5 --dtype f16x2]

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
from src.census import level, level_table  # noqa: E402
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
    new = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    counts, loss = new(5), new(1)
    levels, npix, keep = [], [], []
    for i, lvl in enumerate((6, 5, 4, 3, 2)):
        h, w = H >> lvl, Wd >> lvl
        scale = 20.0 * w / Wd
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        flow = np.stack([1.5 * np.sin(yy / 7.0) + 0.8, 1.2 * np.cos(xx / 9.0) - 0.5], -1)[None]       # level pixels
        flow = flow * np.where(np.arange(n) % 2, -1.0, 1.0)[:, None, None, None] + 0.05 * rng.standard_normal((n, h, w, 2))
        pred = torch.from_numpy((flow / scale).astype(np.float32)).to(dev)
        img = torch.from_numpy(rng.random((n, h, w, 3), dtype=np.float32)).to(dev)
        bufs = (pred, img, torch.ones((n, h, w), device=dev), new(n, h, w, 2), new(n, h, w), new(3, n, h, w), new(n, h, w),
                new(2, n, h, w))
        keep.append(bufs)  # (a level holds addresses, not tensors)
        levels.append(level(*bufs, counts[i:i + 1], scale, LOSS_WEIGHTS[lvl] / 5.0))
        npix.append(n * h * w)
    table = level_table(levels)
    s = _hip.stream_ptr

    def warp():
        _hip.check(lib.fn2_fill_zero(_hip.ptr(counts), 20, s()))
        _hip.check(lib.fn2_census_warp(table, 5, n, s()))

    def cost():
        _hip.check(lib.fn2_census_cost(table, 5, n, 0.4, _hip.ptr(loss), s()))

    def grad():
        _hip.check(lib.fn2_census_grad(table, 5, n, 1.0, s()))

    warp(), cost(), grad()
    torch.cuda.synchronize()
    share = float(counts.sum().item()) / sum(npix)
    if not np.isfinite(float(loss.item())):
        raise RuntimeError("non-finite loss")
    t = [timed(fn, args.rounds, args.inner) for fn in (warp, cost, grad)]
    return [row("fn2_census_warp (+ the 20-byte memset of its counters)", t[0]), row("fn2_census_cost", t[1]),
            row("fn2_census_grad", t[2])], share


def step_rows(args, dev):
    n, h, w = args.batch, args.height, args.width
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.random((n // 2, h, w, 3), dtype=np.float32)).to(dev)
    b = torch.roll(a, (2, -3), (1, 2))
    wts = W.init_weights("FlowNetS", 1234)
    trainers = {term: FlowNetSTrainer(wts, n, h, w, dtype=args.dtype, unsupervised=True, data_term=term)
                for term in ("photometric", "census")}
    steps = {term: (lambda tr=tr: tr.train_step_unsupervised(a, b)) for term, tr in trainers.items()}
    for fn in steps.values():
        for _ in range(args.warmup):
            loss = fn()
        torch.cuda.synchronize()
        if not np.isfinite(float(loss.item())):
            raise RuntimeError("non-finite loss")
    times = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, fn in steps.items():
            times[k] += timed(fn, 1, args.steps)
    rows = [row("%s step (captured: %s)" % (k, getattr(tr, "_step_graphs", None) is not None), times[k])
            for k, tr in trainers.items()]
    # the loss stage of either step alone, on the trainer's own buffers, outside the graph
    for k, tr in trainers.items():
        body = timed(lambda tr=tr: tr._stage.launch(_hip.stream_ptr()), args.rounds, args.inner)
        rows.append(row("%s loss stage as the step launches it (frames, masks, data term)" % k, body))
    return rows, float(np.median(times["census"])) / float(np.median(times["photometric"]))


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
    ops, share = op_rows(args, dev)
    steps, ratio = step_rows(args, dev)
    print(json.dumps({"what": "census data term: the three launches, and the census next to the photometric step",
                      "batch": args.batch, "size": [args.height, args.width], "dtype": args.dtype, "cache_warm": True,
                      "counted_share": round(share, 4), "census_over_photometric_step": round(ratio, 4),
                      "unit": "ms (median of rounds)", "ops": ops, "steps": steps}))


if __name__ == "__main__":
    main()
