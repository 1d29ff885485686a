#!/usr/bin/env python
"""Times the intrinsic-image output stage on the GPU box: ``MarigoldIIDPipeline.fill_outputs`` on a CUDA prediction (MG_OP_IID_VIS,
three read-backs) against the numpy path it replaced there (``MarigoldIIDOutput.fill_entry`` per target: one read-back each, then
maximum / division / power / cast on the host), alternating, on the same seeded prediction.  Host clock around work that ends in
a read-back; the two launches alone by device events.  Needs an MI355X.

    python tools/iid_output_bench.py [--size 768] [--rounds 40] [--log profiles/iid_output_stage.log]
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PROPS = {"target_names": ["albedo", "shading", "residual"], "albedo": {"prediction_space": "linear"},
         "shading": {"prediction_space": "linear", "up_to_scale": True},
         "residual": {"prediction_space": "linear", "up_to_scale": True}}   # the lighting model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: nothing to measure")
    from marigold_amd import _lib as L
    from marigold_amd.pipeline import MarigoldIIDOutput, MarigoldIIDPipeline
    from marigold_amd.util.image_util import iid_visualization_device
    L.init(0)
    names, n, s = PROPS["target_names"], 3, args.size
    pred = torch.rand(1, 3 * n, s, s, generator=torch.Generator().manual_seed(0)).cuda()
    stand_in = SimpleNamespace(target_names=names, target_properties=PROPS, n_targets=n)

    def host():
        out = MarigoldIIDOutput(names)
        for i, name in enumerate(names):
            out.fill_entry(name, pred[:, 3 * i:3 * i + 3], None, PROPS)
        return out

    def device():
        out = MarigoldIIDOutput(names)
        MarigoldIIDPipeline.fill_outputs(stand_in, out, pred, None)
        return out
    times = {"numpy fill_entry x 3": [], "device fill_outputs": []}
    for r in range(args.rounds + 5):   # alternating; the first five rounds warm both paths up
        for label, fn in (("numpy fill_entry x 3", host), ("device fill_outputs", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= 5:
                times[label].append(dt)
    linear = [PROPS[t]["prediction_space"] == "linear" for t in names]
    scale = [PROPS[t].get("up_to_scale", False) for t in names]
    dev = pred.reshape(n, 3, s, s)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel = []
    for r in range(args.rounds + 5):
        ev[0].record()
        iid_visualization_device(dev, linear, scale)
        ev[1].record()
        ev[1].synchronize()
        if r >= 5:
            kernel.append(ev[0].elapsed_time(ev[1]))
    a, b = host(), device()
    same = all((a[t].array == b[t].array).all() for t in names)
    lines = [f"IID output stage, {n} targets of 3 x {s} x {s} (albedo linear; shading, residual linear and up to scale), "
             f"{args.rounds} alternating rounds after 5 warm-up rounds, ms per image (median, min - max):"]
    for label, v in times.items():
        lines.append(f"  {label:24s} {statistics.median(v):7.2f}  ({min(v):.2f} - {max(v):.2f})")
    lines.append(f"  {'MG_OP_IID_VIS launches':24s} {statistics.median(kernel):7.3f}  ({min(kernel):.3f} - {max(kernel):.3f})   (device events)")
    lines.append(f"  arrays identical: {same}")
    text = "\n".join(lines)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
