#!/usr/bin/env python
"""Times the edge-guided enlargement of a prediction (``mg_guided_upsample``, csrc/guided.hip) beside the bilinear ``resize`` it takes
the place of in the pipelines' finish stage, alternating, by device events, on the same seeded data already on the device:

* ``resize``            the fp32 prediction [C, h, w] -> [C, H, W] (MG_OP_RESIZE, bilinear: two launches)
* ``guided kernel``     the one launch of ``mg_guided_upsample``, its low-resolution guide already made
* ``guided_upsample``   what the finish stage calls: the guide (the uint8 picture's planes resampled to h x w) and that launch

Shape: C x 576 x 768 -> 3 000 x 4 000 (a 12-megapixel picture at ``processing_res=768``), C = 1 (depth) and 3 (normals), radius 1 to
4 at sigma 0.1.  The first line of the log is the box's calibration (``mg_clock_probe``).  Needs an MI355X.

    python tools/guided_bench.py [--rounds 50] [--log profiles/guided_upsample.log]
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

WARM = 3


def _stat(v):
    return f"{statistics.median(v):7.3f}  ({min(v):.3f} - {max(v):.3f})"


def _alternate(rounds, pairs):
    """pairs: [(label, fn)] -> {label: [ms by device events]}, the functions taking turns within every round"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {label: [] for label, _ in pairs}
    for r in range(rounds + WARM):
        for label, fn in pairs:
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            if r >= WARM:
                times[label].append(ev[0].elapsed_time(ev[1]))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--log", type=str, default=None)
    ap.add_argument("--low", type=int, nargs=2, default=(576, 768))
    ap.add_argument("--high", type=int, nargs=2, default=(3000, 4000))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: nothing to measure")
    from marigold_amd import _lib as L, ops as O
    from marigold_amd.guided import guided_upsample
    from marigold_amd.util.image_util import InterpolationMode, resize
    lib = L.init(0)
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0, ctypes.byref(mhz), ctypes.byref(tflops)),
            "mg_clock_probe", lib)
    (h, w), (H, W) = args.low, args.high
    lines = [f"calibration of this box (mg_clock_probe, random operands): shader clock {mhz.value:.0f} MHz under matrix load, "
             f"{tflops.value:.0f} TFLOP/s bf16 MFMA chain; torch {torch.__version__}",
             f"{args.rounds} alternating rounds after {WARM} warm-up rounds; device events; ms, median (min - max)"]
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(1, 3, 30, 40, generator=g) * 255.0   # a picture with flat regions and edges, plus noise
    picture = (torch.nn.functional.interpolate(coarse, size=(H, W), mode="nearest")[0] + torch.randn(3, H, W, generator=g) * 4.0)
    picture = picture.clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().cuda()   # [H, W, 3], as PIL holds it
    lo = resize(picture.permute(2, 0, 1).contiguous(), (h, w), InterpolationMode.BILINEAR, antialias=True).contiguous()
    for C in (1, 3):
        pred = torch.rand(C, h, w, generator=g).cuda()
        out = torch.empty((C, H, W), dtype=torch.float32, device="cuda")

        def kernel(R, pred=pred, out=out, C=C):
            L.check(lib.mg_guided_upsample(pred.data_ptr(), C, h, w, lo.data_ptr(), picture.data_ptr(), 1, H, W, R, 0.1, out.data_ptr(),
                                           O.current_stream_handle()), "mg_guided_upsample", lib)
        pairs = [("resize (bilinear)", lambda pred=pred: resize(pred, (H, W), InterpolationMode.BILINEAR, antialias=True))]
        pairs += [(f"guided kernel, radius {R}", lambda R=R: kernel(R)) for R in (1, 2, 3, 4)]
        pairs += [("guided_upsample, radius 2", lambda pred=pred: guided_upsample(pred, picture, 2, 0.1, lib=lib))]
        t = _alternate(args.rounds, pairs)
        lines.append(f"{C} x {h} x {w} -> {H} x {W}:")
        for label, _ in pairs:
            lines.append(f"  {label:30s} {_stat(t[label])}")
        mb = (C * H * W * 4 + 3 * H * W + (3 + 4 * C) * h * w) / 1e6
        lines.append(f"  (the guided kernel's compulsory traffic: {mb:.1f} MB - the output, the picture's bytes, guide and prediction once)")
    text = "\n".join(lines)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
