#!/usr/bin/env python
"""Time of the variational refinement (src/variational.py, fn2_variational_refine) per pair, with the reference's
default parameters, at batch 1 and 8 for 384x512 and 436x1024.  HIP events on the launch stream after a warm-up call;
`build_ms` is the whole refinement with niter_solver=0 (presmoothing, warps, derivatives and the SOR system of the
five outer iterations), `sor_ms` the rest (the five 30-sweep wavefront solves).  One JSON line on stdout.

  timeout -k 10 600 python tools/bench_variational.py [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flownet2-tf_amd"))
from src import _hip  # noqa: E402
from src.variational import DEFAULTS  # noqa: E402


def frames(n, h, w, seed):
    """Seeded smooth RGB frames and a shifted second frame, with a smooth init flow."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (n, h // 8 + 2, w // 8 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 8, 1), 8, 2)[:, :h + 4, :w + 4]
    a = big[:, :h, :w].astype(np.uint8)
    b = big[:, 2:h + 2, 3:w + 3].astype(np.uint8)
    f = np.zeros((n, h, w, 2), np.float32)
    f[..., 0], f[..., 1] = 2.5, 1.5
    return a, b, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = _hip.require_device()
    lib = _hip.lib()
    res = {"what": "variational refinement, reference defaults (5 outer x 30 SOR sweeps)", "unit": "ms per pair"}
    for h, w in ((384, 512), (436, 1024)):
        for n in (1, 8):
            a, b, f = frames(n, h, w, 0)
            ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            init = torch.from_numpy(f).to(dev)
            flow = init.clone()
            wsb = int(lib.fn2_variational_workspace_bytes(n, h, w))
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            p = dict(DEFAULTS)

            def call(solver):
                _hip.check(lib.fn2_variational_refine(
                    _hip.ptr(ta), _hip.ptr(tb), w * 3, h * w * 3, _hip.ptr(flow), w * 2, h * w * 2, n, h, w,
                    p["alpha"], p["gamma"], p["delta"], p["sigma"], p["niter_outer"], p["niter_inner"], solver,
                    p["sor_omega"], _hip.ptr(ws), wsb, _hip.stream_ptr()))

            def timed(solver):
                flow.copy_(init)
                call(solver)  # warm-up
                ts = []
                for _ in range(args.reps):
                    flow.copy_(init)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(solver)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                return float(np.median(ts))

            total = timed(p["niter_solver"])
            build = timed(0)
            res["%dx%d_b%d" % (h, w, n)] = {"total_ms": round(total / n, 3), "build_ms": round(build / n, 3),
                                            "sor_ms": round((total - build) / n, 3), "batch_ms": round(total, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
