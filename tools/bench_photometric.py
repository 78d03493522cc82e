#!/usr/bin/env python
"""The occlusion-aware photometric loss, timed two ways in one process.  A record, not a threshold.

1. The two launches (fn2_photometric_masks, fn2_photometric_loss_grad) on one table of FlowNetS's five loss scales for
   batch 8 at 384x512, device events around `--inner` back-to-back launches, median of `--rounds`.  The predictions are a
   smooth flow of a few pixels plus noise, the frames random; all buffers together are a few MB and stay in the caches
   between launches, so these are cache-warm times.  `bytes` is what the algorithm moves (own flow, four partner taps,
   mask, and on unmasked pixels five RGB reads; gradient stores), computed from the shapes and the measured mask share.
2. The captured unsupervised step next to the captured supervised step of the same trainer configuration (FlowNetS,
   same batch, size and dtype), in alternating rounds of `--steps` steps; `loss_share` is the two launches (plus the five
   frame downsamples, timed the same way) over the unsupervised step.

  timeout -k 10 600 python tools/bench_photometric.py [--steps 30 --rounds 5 --dtype f16x2]

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
from src.photometric import level, level_table  # noqa: E402
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
    levels, npix = [], []
    for i, lvl in enumerate((6, 5, 4, 3, 2)):
        h, w = H >> lvl, Wd >> lvl
        scale = 20.0 * w / Wd
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        flow = np.stack([1.5 * np.sin(yy / 7.0) + 0.8, 1.2 * np.cos(xx / 9.0) - 0.5], -1)[None]       # level pixels
        flow = flow * np.where(np.arange(n) % 2, -1.0, 1.0)[:, None, None, None] + 0.05 * rng.standard_normal((n, h, w, 2))
        pred = torch.from_numpy((flow / scale).astype(np.float32)).to(dev)
        img = torch.from_numpy(rng.random((n, h, w, 3), dtype=np.float32)).to(dev)
        levels.append(level(pred, img, new(n, h, w), counts[i:i + 1], new(n, h, w, 2), scale, LOSS_WEIGHTS[lvl] / 5.0))
        npix.append(n * h * w)
    table = level_table(levels)
    s = _hip.stream_ptr

    def masks():
        _hip.check(lib.fn2_fill_zero(_hip.ptr(counts), 20, s()))
        _hip.check(lib.fn2_photometric_masks(table, 5, n, 0.01, 0.5, s()))

    def grad():
        _hip.check(lib.fn2_photometric_loss_grad(table, 5, n, 0.4, 1.0, _hip.ptr(loss), s()))

    masks(), grad()
    torch.cuda.synchronize()
    share = float(counts.sum().item()) / sum(npix)
    pix = float(sum(npix))
    b_masks = pix * (8 + 4 * 8 + 4)
    b_grad = pix * (4 + 8) + pix * share * (8 + 5 * 12)
    t_m, t_g = timed(masks, args.rounds, args.inner), timed(grad, args.rounds, args.inner)
    return [row("fn2_photometric_masks (+ the 20-byte memset of its counters)", t_m, bytes=int(b_masks)),
            row("fn2_photometric_loss_grad", t_g, bytes=int(b_grad))], share


def step_rows(args, dev):
    n, h, w = args.batch, args.height, args.width
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.random((n, h, w, 3), dtype=np.float32)).to(dev)
    b = torch.roll(a, (2, -3), (1, 2))
    gt = torch.from_numpy(np.clip(rng.standard_normal((n, h, w, 2)) * 5, -40, 40).astype(np.float32)).to(dev)
    wts = W.init_weights("FlowNetS", 1234)
    sup = FlowNetSTrainer(wts, n, h, w, dtype=args.dtype)
    uns = FlowNetSTrainer(wts, n, h, w, dtype=args.dtype, unsupervised=True)
    steps = {"supervised": lambda: sup.train_step(a, b, gt),
             "unsupervised": lambda: uns.train_step_unsupervised(a[:n // 2], b[:n // 2])}
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
    # the loss launches of the unsupervised step alone, on the trainer's own buffers, outside the graph
    body = timed(lambda: uns._photo.launch(_hip.stream_ptr()), args.rounds, args.inner)
    rows = [row(k + " step (captured: %s)" % (getattr(tr, "_step_graphs", None) is not None), times[k])
            for k, tr in (("supervised", sup), ("unsupervised", uns))]
    rows.append(row("frames at five sizes + masks + loss_grad, as the step launches them", body))
    return rows, float(np.median(body)) / float(np.median(times["unsupervised"]))


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
    steps, loss_share = step_rows(args, dev)
    print(json.dumps({"what": "photometric loss: the two launches, and the unsupervised next to the supervised step",
                      "batch": args.batch, "size": [args.height, args.width], "dtype": args.dtype, "cache_warm": True,
                      "unmasked_share": round(share, 4), "loss_share": round(loss_share, 4),
                      "unit": "ms (median of rounds)", "ops": ops, "steps": steps}))


if __name__ == "__main__":
    main()
