#!/usr/bin/env python
"""The sparse multi-scale EPE, timed two ways in one process.  A record, not a threshold.

1. The two launches alone (fn2_sparse_epe_count, fn2_sparse_epe_loss_grad) on one table of FlowNetS's five loss scales for
   batch 8 at 384x512, with about 20 % and with 100 % valid labels, device events around `--inner` back-to-back launches,
   every shape warmed up, the variants in alternating rounds, median of `--rounds`.  All buffers together are a few MB and
   stay in the caches between launches, so these are cache-warm times.  `bytes` is what the algorithm moves once (count:
   every label read; loss_grad: every prediction and label read, every gradient written), computed from the shapes.
2. The captured supervised step of the same tree with the dense loss and with sparse_gt=True, the latter on a ground truth
   that is about 20 % valid and on one that is 100 % valid, in alternating rounds of `--steps` steps, every measurement in
   a child process of its own (one trainer per process): `added_ms` is the difference of the medians to the dense step.

  timeout -k 10 600 python tools/bench_sparse_epe.py [--steps 30 --rounds 5 --dtype f16x2]

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
    keep, variants, pix = [], {}, 0
    for share in (0.2, 1.0):
        levels = []
        counts = torch.zeros(5, dtype=torch.int32, device=dev)
        for i, lvl in enumerate((6, 5, 4, 3, 2)):
            h, w = H >> lvl, Wd >> lvl
            pred = torch.from_numpy(rng.standard_normal((n, h, w, 2)).astype(np.float32)).to(dev)
            lab = rng.standard_normal((n, h, w, 2)).astype(np.float32)
            lab[rng.random((n, h, w)) >= share] = np.nan
            label, dpred = torch.from_numpy(lab).to(dev), torch.zeros_like(pred)
            keep += [pred, label, dpred, counts]
            levels.append(_hip.Fn2SparseEpeLevel(pred.data_ptr(), label.data_ptr(), dpred.data_ptr(), counts[i:i + 1].data_ptr(),
                                                 h, w, LOSS_WEIGHTS[lvl] / 5.0))
            pix += n * h * w if share == 1.0 else 0
        variants[share] = ((_hip.Fn2SparseEpeLevel * 5)(*levels), counts)

    def count_of(share):
        table, counts = variants[share]

        def launch():  # (the counters run on: the launch adds; a timing reads no value, and 2^32 is far away)
            _hip.check(lib.fn2_sparse_epe_count(table, 5, n, _hip.stream_ptr()))
        return launch

    def loss_of(share):
        table, counts = variants[share]

        def launch():
            _hip.check(lib.fn2_sparse_epe_loss_grad(table, 5, n, 16384.0, _hip.ptr(loss), _hip.stream_ptr()))
        return launch

    fns = {}
    for share in (0.2, 1.0):
        table, counts = variants[share]
        fns["fn2_sparse_epe_count, %d %% valid" % round(100 * share)] = (count_of(share), 8)
        fns["fn2_sparse_epe_loss_grad, %d %% valid" % round(100 * share)] = (loss_of(share), 24)
        counts.zero_()
        count_of(share)()                                           # the counters the loss launch normalises by
        torch.cuda.synchronize()
    for fn, _ in fns.values():                                      # warm every shape up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    if not np.isfinite(float(loss.item())):
        raise RuntimeError("non-finite loss")
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                                    # alternating rounds
        for k, (fn, _) in fns.items():
            times[k] += timed(fn, 1, args.inner)
    return [row(k, times[k], bytes=int(pix * b)) for k, (_, b) in fns.items()]


def one_step_run(args, variant):
    """The child's half of step_rows: ONE trainer in this process, warmed up, then `--steps` steps timed once."""
    dev = _hip.require_device()
    n, h, w = args.batch, args.height, args.width
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.random((n, h, w, 3), dtype=np.float32)).to(dev)
    b = torch.roll(a, (2, -3), (1, 2))
    gt = torch.from_numpy((3.0 * rng.standard_normal((n, h, w, 2))).astype(np.float32)).to(dev)
    if variant == "sparse20":
        gt[torch.from_numpy(rng.random((n, h, w)) >= 0.2).to(dev)] = float("nan")
    tr = FlowNetSTrainer(W.init_weights("FlowNetS", 1234), n, h, w, dtype=args.dtype, sparse_gt=variant != "dense")
    for _ in range(args.warmup):
        loss = tr.train_step(a, b, gt)
    torch.cuda.synchronize()
    if not np.isfinite(float(loss.item())):
        raise RuntimeError("non-finite loss")
    ms = timed(lambda: tr.train_step(a, b, gt), 1, args.steps)[0]
    out = dict(ms=ms, captured=getattr(tr, "_step_graphs", None) is not None, loss=float(tr.loss_dev.item()))
    if tr._sparse is not None:
        out["valid_per_level"] = [int(c) for c in tr._sparse.counts.cpu().numpy()]
    print(json.dumps(out))


VARIANTS = {"dense": "dense", "sparse20": "sparse_gt, 20 % valid", "sparse100": "sparse_gt, 100 % valid"}


def step_rows(args):
    """One trainer per process: every measurement is a fresh child (started before this process touches the device),
    the variants in alternating rounds.  Several trainers stepping in one process were seen to disturb each other's
    captured steps, and one trainer per process is how the CLIs run."""
    import subprocess
    times, last = {k: [] for k in VARIANTS}, {}
    for _ in range(args.rounds):
        for k in VARIANTS:
            res = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", k,
                                  "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch),
                                  "--height", str(args.height), "--width", str(args.width), "--dtype", args.dtype],
                                 capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError("child %s ended with %d: %s" % (k, res.returncode, res.stderr[-1000:]))
            last[k] = json.loads(res.stdout.strip().splitlines()[-1])
            times[k].append(last[k]["ms"])
    base = float(np.median(times["dense"]))
    return [row("supervised step, %s (captured: %s)" % (VARIANTS[k], last[k]["captured"]), times[k],
                added_ms=round(float(np.median(times[k])) - base, 5),
                **({"valid_per_level": last[k]["valid_per_level"]} if "valid_per_level" in last[k] else {}))
            for k in VARIANTS]


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
    ap.add_argument("--child", default=None, choices=sorted(VARIANTS), help="internal: time one variant's step and exit")
    args = ap.parse_args()
    if args.child:
        return one_step_run(args, args.child)
    steps = step_rows(args)                                        # children first: this process has not opened the device yet
    dev = _hip.require_device()
    print(json.dumps({"what": "sparse multi-scale EPE: the two launches alone, and the captured supervised step with the "
                              "dense and with the sparse loss",
                      "batch": args.batch, "size": [args.height, args.width], "dtype": args.dtype, "cache_warm": True,
                      "unit": "ms (median of rounds)", "ops": op_rows(args, dev), "steps": steps}))


if __name__ == "__main__":
    main()
