#!/usr/bin/env python
"""The intrinsic-image scorer (evaluation.score_iid, csrc/evalscore.hip) measured beside the host function it restates.

    python tools/eval_iid_bench.py scorer      # ms per target: numpy compute_iid_metric (psnr + ssim) | score_iid (uploads + read-back)
    python tools/eval_iid_bench.py kernels     # 20 score_iid calls per case at 768 x 768, nothing else: run it under
                                               #   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_iid_bench.py kernels

``scorer`` prints the box calibration of bench.py first; every figure is the median (and min) of ``--reps`` calls after one
warm-up call, on host wall clock around a call that ends in the read-back.
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


def _pair(h, w, seed=1):
    r = np.random.default_rng(seed)
    gt = r.uniform(0, 0.7, (3, h, w)).astype(np.float32)
    pred = np.clip(gt * 0.6 + r.normal(0, 0.03, gt.shape), 0, 1).astype(np.float32)
    mask = np.broadcast_to(r.uniform(size=(1, h, w)) > 0.15, gt.shape).copy()
    return pred, gt, mask


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def scorer(reps, calibrate):
    import torch
    from marigold_amd.evaluation import metrics as M, score_iid
    if calibrate:
        from bench import calibration
        print("calibration " + json.dumps(calibration(torch.device("cuda", 0))), flush=True)
    for h, w in ((480, 640), (768, 768)):
        pred, gt, mask = _pair(h, w)
        dev = [torch.from_numpy(a).cuda() for a in (pred, gt, mask)]
        for target, kind in (("albedo", "plain"), ("shading", "up to scale")):
            def host():
                return [M.compute_iid_metric(pred.copy(), gt.copy(), target, m, mask) for m in ("psnr", "ssim")]

            def device():
                return score_iid(pred, gt, target, mask)

            def device_resident():
                return score_iid(dev[0], dev[1], target, dev[2])
            for name, fn in (("host   compute_iid_metric psnr + ssim (numpy, masked)", host),
                             ("device score_iid, numpy pred / gt / mask (3 uploads + read-back)", device),
                             ("device score_iid, pred / gt / mask resident (read-back)", device_resident)):
                med, best = _median_ms(fn, reps)
                print(f"iid {h}x{w} {target:8s} ({kind:11s}) {name:66s} median {med:8.3f} ms  min {best:8.3f} ms", flush=True)


def kernels():
    import torch
    from marigold_amd.evaluation import score_iid
    pred, gt, mask = (torch.from_numpy(a).cuda() for a in _pair(768, 768))
    for target in ("albedo", "shading"):
        for _ in range(20):
            score_iid(pred, gt, target, mask)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["scorer", "kernels"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-calibration", action="store_true")
    a = ap.parse_args()
    {"scorer": lambda: scorer(a.reps, not a.no_calibration), "kernels": kernels}[a.what]()
