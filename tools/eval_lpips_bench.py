#!/usr/bin/env python
"""LPIPS on the device (evaluation.score_iid with ``lpips=``, csrc/lpips.hip) measured beside the host function it restates
(``metrics.lpips``, torch CPU fp32), on one target of 3 x 768 x 1024 with synthetic weights.

    python tools/eval_lpips_bench.py [--rounds 5] [--reps 10] [--host-reps 1]
    python tools/eval_lpips_bench.py --kernels    # 20 device calls (plain target, then gamma 2.2), nothing else: run it under
                                                  #   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_lpips_bench.py --kernels

Rounds alternate the two sides (host, device, host, device, ...); every figure is host wall clock around a call that ends in the
read-back, the inputs resident on the device.  Per side the median over all rounds and the spread (min .. max of the rounds' medians)
are printed, then the device time as a multiple of the 0.29 ms that the 44.7 GFLOP of the ten convolutions take at the 155 TFLOP/s
fp32-MFMA peak.  The box calibration of bench.py comes first.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 768, 1024
PEAK_TFLOPS = 155.0


def conv_flop(h, w):
    from marigold_amd.evaluation import metrics as M
    flop = 0
    for l, (cin, cout, k, stride, pad) in enumerate(M.LPIPS_CONVS):
        if M.LPIPS_POOL_BEFORE[l]:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        flop += 2 * 2 * h * w * cout * cin * k * k   # two images
    return flop


def synthetic_net(seed=0):
    import torch
    from marigold_amd.evaluation import LpipsNet, metrics as M
    g = torch.Generator().manual_seed(seed)
    cw = [torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5 for ci, co, k, _, _ in M.LPIPS_CONVS]
    cb = [0.1 * torch.randn(co, generator=g) for _, co, _, _, _ in M.LPIPS_CONVS]
    lw = [torch.rand(1, co, 1, 1, generator=g) * (2.0 / co) for _, co, _, _, _ in M.LPIPS_CONVS]
    return LpipsNet(cw, cb, lw)


def _times_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main(rounds, reps, host_reps, calibrate):
    import torch
    from marigold_amd.evaluation import metrics as M, score_iid
    if calibrate:
        from bench import calibration
        from marigold_amd import _lib
        _lib.init(0)
        print("calibration " + json.dumps(calibration(torch.device("cuda", 0))), flush=True)
    r = np.random.default_rng(1)
    gt = r.uniform(0, 1, (3, H, W)).astype(np.float32)
    pred = np.clip(gt + 0.1 * r.normal(size=gt.shape), 0, 1).astype(np.float32)
    net = synthetic_net()
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()

    def host():
        return M.compute_iid_metric(pred[None], gt[None], "albedo", "lpips", None, lpips_net=net)

    def device():
        return score_iid(dp, dg, "albedo", None, metrics=("lpips",), lpips=net)["lpips"]

    def device_all():
        return score_iid(dp, dg, "albedo", None, metrics=("psnr", "ssim", "lpips"), lpips=net)["lpips"]

    def device_without():
        return score_iid(dp, dg, "albedo", None)["psnr"]
    hv, dv = host(), device()   # warm-up of both sides
    device_all(), device_without()
    print(f"lpips {H}x{W}: host fp32 {hv:.9g}  device {dv:.9g}  relative difference {abs(dv - hv) / hv:.3e}", flush=True)
    sides = {"host   metrics.lpips (torch CPU fp32, %d threads)" % torch.get_num_threads(): (host, host_reps),
             "device score_iid lpips only (resident inputs, read-back)": (device, reps),
             "device score_iid psnr + ssim + lpips": (device_all, reps),
             "device score_iid psnr + ssim (no lpips)": (device_without, reps)}
    medians = {k: [] for k in sides}
    every = {k: [] for k in sides}
    for _ in range(rounds):
        for name, (fn, n) in sides.items():
            ts = _times_ms(fn, n)
            medians[name].append(statistics.median(ts))
            every[name] += ts
    for name in sides:
        print(f"{name:62s} median {statistics.median(every[name]):10.3f} ms  rounds' medians {min(medians[name]):10.3f} .. {max(medians[name]):10.3f} ms"
              f"  min {min(every[name]):10.3f} ms", flush=True)
    flop = conv_flop(H, W)
    ideal_ms = flop / (PEAK_TFLOPS * 1e12) * 1e3
    dev_ms = statistics.median(every[list(sides)[1]])
    print(f"convolutions: {flop / 1e9:.1f} GFLOP = {ideal_ms:.3f} ms at {PEAK_TFLOPS:.0f} TFLOP/s; the device call takes {dev_ms / ideal_ms:.1f} x that "
          f"({flop / dev_ms / 1e9:.1f} TFLOP/s over the whole call)", flush=True)


def kernels():
    import torch
    from marigold_amd.evaluation import score_iid
    r = np.random.default_rng(1)
    gt = r.uniform(0, 1, (3, H, W)).astype(np.float32)
    pred = np.clip(gt + 0.1 * r.normal(size=gt.shape), 0, 1).astype(np.float32)
    net = synthetic_net()
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    for gamma in (None, 2.2):
        for _ in range(10):
            score_iid(dp, dg, "albedo", None, metrics=("lpips",), gamma=gamma, lpips=net)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        kernels()
        sys.exit(0)
    main(a.rounds, a.reps, a.host_reps, not a.no_calibration)
