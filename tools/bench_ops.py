#!/usr/bin/env python
"""Achieved HBM bandwidth of the HBM-bound custom ops at the BASELINE sizes (algorithmic
bytes per sample), events on the launch stream, median of `--rounds` rounds of `--inner` launches.

  python tools/bench_ops.py [--batch 8] [--height 384 --width 512] > profiles/rNN_ops_bandwidth.json
  python tools/bench_ops.py --interp [--batch 8 ...]    only the FlowNetS_interp input op against what it replaces
  python tools/bench_ops.py --occlusion --batch 4 --height 436 --width 1024    only the forward-backward occlusion check
  python tools/bench_ops.py --selflow-augment           only the SelFlow-style training augmentation (8 x 384 x 512)
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

HBM_PEAK = 8000.0


def timed(fn, rounds, inner):
    ts = []
    for r in range(rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts))


def timed_pair(fn_a, fn_b, rounds, inner):
    """Two alternatives in the same process, alternating round by round: (median, min, max) ms of each."""
    ts = ([], [])
    for r in range(rounds + 2):
        for k, fn in enumerate((fn_a, fn_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ts[k].append(e0.elapsed_time(e1) / inner)
    return tuple((float(np.median(t)), float(min(t)), float(max(t))) for t in ts)


def bench_interp(N, H, W, rounds, inner, rec):
    """fn2_pack_interp_u8 (uint8 image + uint8 mask + fp32 sparse flow -> split-fp16 stem input) against the sequence it
    stands in for, with every input already on the device: the torch ops of Engine.set_inputs_interp (`sf * 0.05`, cat,
    two staging copies) + fn2_pack_pair."""
    import ctypes as C
    dev = _hip.require_device()
    lib, st, P_ = _hip.lib(), _hip.stream_ptr, _hip.ptr
    g = torch.Generator(device="cpu").manual_seed(1)
    pad = 3
    img8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    m8 = ((torch.rand(N, H, W, generator=g) > 0.9).to(torch.uint8) * 255).to(dev)
    sf = (torch.randn(N, H, W, 2, generator=g) * 8).to(dev) * (m8 > 0)[..., None]
    lut = torch.from_numpy((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)).to(dev)
    flags = torch.ones(N, 2, dtype=torch.uint8, device=dev)
    a_f, m_f = lut[img8.long()], lut[m8.long()][..., None]          # what adapt_x_matches ships as fp32
    in_a, in_b = torch.empty_like(a_f), torch.empty_like(a_f)      # the engine's staging tensors
    stem_new = torch.zeros(N, H + 2 * pad, W + 2 * pad, 8, dtype=torch.float32, device=dev)
    stem_old = torch.zeros_like(stem_new)
    v_new, v_old = _hip.view(stem_new, 6, 0, _hip.FN2_F16X2), _hip.view(stem_old, 6, 0, _hip.FN2_F16X2)

    def new():
        _hip.check(lib.fn2_pack_interp_u8(P_(img8), P_(m8), P_(sf), P_(lut), P_(flags), C.byref(v_new), pad, st()))

    def pack_pair():
        _hip.check(lib.fn2_pack_pair(P_(in_a), P_(in_b), C.byref(v_old), pad, st()))

    def old():
        in_a.copy_(a_f, non_blocking=True)
        in_b.copy_(torch.cat([sf * 0.05, m_f], dim=3), non_blocking=True)
        pack_pair()

    new(), old()
    torch.cuda.synchronize()
    assert torch.equal(stem_new, stem_old), "the two paths must write the same bytes"
    px = N * H * W
    (t_new, lo_n, hi_n), (t_old, lo_o, hi_o) = timed_pair(new, old, rounds, inner)
    rec("pack_interp_u8", t_new, px * (3 + 1 + 8 + 32), "12 B in (rgb bytes, mask byte, sparse flow) + one 32 B group out per pixel; "
        "min %.5f max %.5f ms over the rounds" % (lo_n, hi_n))
    rec("set_inputs_interp_device_ops+pack_pair", t_old, px * (16 + 24 + 48 + 56),
        "what pack_interp_u8 replaces, inputs on the device: mul (8+8 B), cat (12+12), two staging copies (24+24), pack_pair "
        "(24+32) per pixel, 5 launches; min %.5f max %.5f ms over the rounds" % (lo_o, hi_o))
    rec("pack_pair", timed(pack_pair, rounds, inner), px * (24 + 32), "the last launch of that sequence by itself")


def bench_occlusion(N, H, W, rounds, inner, rec):
    """fn2_fb_occlusion on a smooth flow pair (the case its gathers are laid out for: neighbouring lanes read neighbouring
    taps) and on an incoherent one (every tap its own cache line), and fn2_tf_warp_f32 on a two-channel map.  Algorithmic
    traffic per pixel: both flows once (16 B) + both masks (8 B as float32, 2 B as uint8); the 8 gathered taps are reuse."""
    dev = _hip.require_device()
    lib, st, P_ = _hip.lib(), _hip.stream_ptr, _hip.ptr
    g = torch.Generator(device="cpu").manual_seed(2)
    coarse = torch.randn(N, 2, H // 32 + 2, W // 32 + 2, generator=g) * 6
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    fw = smooth.contiguous().to(dev)
    bw = (-smooth + 0.3 * torch.randn(N, H, W, 2, generator=g)).contiguous().to(dev)
    rough_fw, rough_bw = (torch.randn(N, H, W, 2, generator=g) * 40).to(dev), (torch.randn(N, H, W, 2, generator=g) * 40).to(dev)
    px = N * H * W
    for tag, (a, b) in (("", (fw, bw)), ("_incoherent", (rough_fw, rough_bw))):
        for code, name, dt, mb in ((_hip.MASK_F32, "f32", torch.float32, 4), (_hip.MASK_U8, "u8", torch.uint8, 1)):
            o1, o2 = torch.empty(px, dtype=dt, device=dev), torch.empty(px, dtype=dt, device=dev)
            ms = timed(lambda: _hip.check(lib.fn2_fb_occlusion(P_(a), P_(b), 2 * W, 2 * W * H, P_(o1), P_(o2), code, N, H, W,
                                                               0.01, 0.5, st())), rounds, inner)
            rec("fb_occlusion_%s%s" % (name, tag), ms, px * (16 + 2 * mb),
                "both flows once + both masks; %.2f of the forward mask set" % float((o1 != 0).float().mean()))
    wo = torch.empty(N, H, W, 2, dtype=torch.float32, device=dev)
    ms = timed(lambda: _hip.check(lib.fn2_tf_warp_f32(P_(bw), 2 * W, 2 * W * H, P_(fw), 2 * W, 2 * W * H, P_(wo), N, H, W, 2,
                                                      st())), rounds, inner)
    rec("tf_warp_f32_c2", ms, px * (8 + 8 + 8), "map + flow + output")


def bench_selflow_augment(N, H, W, rounds, inner, rec):
    """fn2_selflow_stats + fn2_selflow_apply on an `image_matches` batch with every stage on (uniform re-sampling, both
    flips, a permutation, one chain order per sample), timed together as one augmentation and each by itself, then the NumPy
    twin of the tests on the same batch (wall clock, one run) and a FlowNetS train step of the same batch size for scale.
    Algorithmic bytes per pixel: stats reads the image (12 B); apply reads image, matches, sparse flow, edges and ground
    truth (12 + 4 + 8 + 4 + 8 = 36 B) and writes the same five (36 B).  The buffers are reused launch after launch and fit the
    256 MB last-level cache at the default size, so these are cache-warm times."""
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import selflow_twin as twin
    from src import data_augmentation as DA
    dev = _hip.require_device()
    lib, st, P_ = _hip.lib(), _hip.stream_ptr, _hip.ptr
    rng = np.random.default_rng(3)
    host = [rng.random((N, H, W, 3), dtype=np.float32), (rng.random((N, H, W, 1)) < 0.05).astype(np.float32),
            rng.standard_normal((N, H, W, 2)).astype(np.float32), rng.random((N, H, W, 1), dtype=np.float32),
            rng.standard_normal((N, H, W, 2)).astype(np.float32)]
    table = DA.draw_interp_params(rng, N, H, W)
    table[:, DA.DISTRIB] = DA.DISTRIB_UNIFORM
    table[:, DA.THRESHOLD] = DA.density_threshold(25.0)
    table[:, [DA.FLIP_LR, DA.FLIP_UD]] = 1
    table.view(np.int32)[:, DA.COLOUR_ORDER] = np.arange(N) % 4
    img, m, sf, ed, gt = (torch.from_numpy(x).to(dev) for x in host)
    outs = [torch.empty_like(t) for t in (img, m, sf, ed, gt)]
    par = torch.from_numpy(table.view(np.int32)).to(dev)
    need = int(lib.fn2_selflow_workspace_bytes(N, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def stats():
        _hip.check(lib.fn2_selflow_stats(P_(img), None, P_(par), None, P_(ws), need, N, H, W, st()))

    def apply():
        _hip.check(lib.fn2_selflow_apply(P_(img), None, P_(m), P_(sf), P_(ed), P_(gt), P_(outs[0]), None, P_(outs[1]),
                                         P_(outs[2]), P_(outs[3]), P_(outs[4]), P_(par), None, P_(ws), need, N, H, W, st()))

    def both():
        stats(), apply()

    px = N * H * W
    rec("selflow_stats+apply", timed(both, rounds, inner), px * (12 + 36 + 36),
        "both launches of one augmentation (+ the 4 N-byte memset of the counts); cache-warm")
    rec("selflow_stats", timed(stats, rounds, inner), px * 12, "image once; cache-warm")
    rec("selflow_apply", timed(apply, rounds, inner), px * 72, "five tensors in, five out; cache-warm")
    t0 = time.perf_counter()
    want = twin.apply(table, image_a=host[0], matches=host[1], sparse_flow=host[2], edges=host[3], flow=host[4])
    t_twin = (time.perf_counter() - t0) * 1e3
    err = float(np.abs(outs[0].cpu().numpy() - want["image_a"]).max())
    rec("selflow_numpy_twin", t_twin, px * 72, "tests/selflow_twin.py (float64 colour) on the host, one run, wall clock; "
        "max |GPU - twin| on the image %.2e" % err)
    from src import weights as Wt
    from src.trainer import FlowNetSTrainer
    tr = FlowNetSTrainer(Wt.init_weights("FlowNetS", 1), N, H, W, dtype="f16x2", model="FlowNetS")
    a, b, f = img, torch.flip(img, dims=(2,)).contiguous(), gt

    def step():
        tr.train_step(a, b, f)

    rec("flownets_train_step_f16x2", timed(step, max(3, rounds // 3), 3), 0, "one FlowNetS train step of this batch, for scale")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--interp", action="store_true", help="only fn2_pack_interp_u8 and the sequence it replaces")
    ap.add_argument("--occlusion", action="store_true", help="only fn2_fb_occlusion and fn2_tf_warp_f32")
    ap.add_argument("--selflow-augment", dest="selflow_augment", action="store_true",
                    help="only fn2_selflow_stats + fn2_selflow_apply, their NumPy twin and a FlowNetS train step for scale")
    a = ap.parse_args()
    N, H, W = a.batch, a.height, a.width
    dev = _hip.require_device()
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    out = {}

    def rec(name, ms, nbytes, note):
        out[name] = {"ms": round(ms, 5), "algorithmic_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / ms / 1e6, 1),
                     "frac_of_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK, 4), "note": note}

    if a.interp or a.occlusion or a.selflow_augment:
        (bench_interp if a.interp else bench_occlusion if a.occlusion else bench_selflow_augment)(N, H, W, a.rounds, a.inner, rec)
        print(json.dumps({"batch": N, "height": H, "width": W, "hbm_peak_GBps": HBM_PEAK, "ops": out}, indent=1))
        return
    lib, st = _hip.lib(), _hip.stream_ptr
    P_ = _hip.ptr
    buf = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    # the C ABI is called directly on preallocated outputs: the Python op wrappers add 10-20 us of host work per
    # call (allocation, argument checks), more than several of these kernels take
    # correlation at the FlowNetC call site: H/8 x W/8 x 256 -> 441 (fp32 op surface)
    h8, w8 = H // 8, W // 8
    fa, fb, co = rnd(N, h8, w8, 256), rnd(N, h8, w8, 256), buf(N, h8, w8, 441)
    ms = timed(lambda: _hip.check(lib.fn2_correlation_f32(P_(fa), P_(fb), P_(co), N, h8, w8, 256, 1, 20, 1, 2, 20, st())),
               a.rounds, a.inner)
    rec("correlation_f32", ms, N * h8 * w8 * (2 * 256 + 441) * 4, "read A, B once + write 441 channels")
    # the same op with a caller-provided workspace: split-fp16 copies of the features + the fp16 matrix-core kernel
    # (what src.correlation.correlation calls for the FlowNetC attribute set)
    need = int(lib.fn2_correlation_workspace_bytes(N, h8, w8, 256, 1, 20, 1, 2, 20))
    if need > 0:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        ms = timed(lambda: _hip.check(lib.fn2_correlation_f32_ws(P_(fa), P_(fb), P_(co), N, h8, w8, 256, 1, 20, 1, 2, 20,
                                                                 P_(ws), need, st())), a.rounds, a.inner)
        rec("correlation_f32_ws", ms, N * h8 * w8 * (2 * 256 + 441) * 4,
            "read A, B once + write 441 channels (+ the two split-fp16 conversion passes, inside the timed call)")
    # the backward ops of SURVEY 8(a) row a12 (used only when a network with these ops is trained)
    gco, gda, gdb = rnd(N, h8, w8, 441), buf(N, h8, w8, 256), buf(N, h8, w8, 256)
    ms = timed(lambda: _hip.check(lib.fn2_correlation_grad_f32(P_(gco), P_(fa), P_(fb), P_(gda), P_(gdb), N, h8, w8, 256,
                                                                 1, 20, 1, 2, 20, st())), max(3, a.rounds // 3), 2)
    rec("correlation_grad_f32", ms, N * h8 * w8 * (4 * 256 + 441) * 4, "read grad, A, B once + write dA, dB")
    # flow_warp at full resolution
    img, flow, wo = rnd(N, H, W, 3), rnd(N, H, W, 2) * 4, buf(N, H, W, 3)
    ms = timed(lambda: _hip.check(lib.fn2_flow_warp_f32(P_(img), P_(flow), P_(wo), N, H, W, 3, st())), a.rounds, a.inner)
    rec("flow_warp_f32", ms, N * H * W * (3 + 2 + 3) * 4, "image + flow + output")
    gwo, gimg, gflow = rnd(N, H, W, 3), buf(N, H, W, 3), buf(N, H, W, 2)
    ms = timed(lambda: _hip.check(lib.fn2_flow_warp_grad_f32(P_(img), P_(flow), P_(gwo), P_(gimg), P_(gflow), N, H, W, 3, st())),
               a.rounds, a.inner)
    rec("flow_warp_grad_f32", ms, N * H * W * (3 + 2 + 3 + 3 + 2) * 4, "image, flow, grad + image_grad (zeroed, atomics), flow_grad")
    # downsample of the ground-truth flow to the coarsest and finest loss scales
    gt = rnd(N, H, W, 2)
    for lvl in (6, 2):
        h, w = H >> lvl, W >> lvl
        do = buf(N, h, w, 2)
        ms = timed(lambda: _hip.check(lib.fn2_downsample_f32(P_(gt), P_(do), N, H, W, 2, h, w, st())), a.rounds, a.inner)
        rec("downsample_to_%dx%d" % (h, w), ms, N * (H * W + h * w) * 2 * 4, "input once + output")
    # resize of predict_flow2 to full resolution
    pf2, ro = rnd(N, H // 4, W // 4, 2), buf(N, H, W, 2)
    ms = timed(lambda: _hip.check(lib.fn2_resize_bilinear_f32(P_(pf2), P_(ro), N, H // 4, W // 4, 2, H, W,
                                                              _hip.C.c_float(20.0), st())), a.rounds, a.inner)
    rec("resize_bilinear_x4", ms, N * (H * W // 16 + H * W) * 2 * 4, "input once + output")
    # augmentation passes (FlyingChairs: crop 7/8 of the width)
    oh, ow = H, W * 7 // 8
    tr = torch.tensor([[1.0, 0.02, 5.0, -0.02, 1.0, 3.0]] * N).to(dev)
    ch = torch.tensor([[1.1, 0.02, 1.05, 0.95, 1.0, 1.05]] * N).to(dev)
    im01, ao, fo = torch.rand(N, H, W, 3, generator=g).to(dev), buf(N, oh, ow, 3), buf(N, oh, ow, 2)
    ms = timed(lambda: _hip.check(lib.fn2_augment_f32(P_(im01), P_(tr), P_(ch), P_(ao), N, H, W, 3, oh, ow, st())),
               a.rounds, a.inner)
    rec("augment_spatial_chromatic", ms, N * (H * W + oh * ow) * 3 * 4, "source once + crop")
    ms = timed(lambda: _hip.check(lib.fn2_flow_augmentation_f32(P_(gt), P_(tr), P_(tr), P_(fo), N, H, W, oh, ow, st())),
               a.rounds, a.inner)
    rec("flow_augmentation", ms, N * (H * W + oh * ow) * 2 * 4, "flow once + crop")
    bench_interp(N, H, W, a.rounds, a.inner, rec)
    bench_occlusion(N, H, W, a.rounds, a.inner, rec)
    print(json.dumps({"batch": N, "height": H, "width": W, "hbm_peak_GBps": HBM_PEAK, "ops": out}, indent=1))


if __name__ == "__main__":
    main()
