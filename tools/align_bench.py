#!/usr/bin/env python
"""What depth alignment costs, at 768 x 768, by device events, alternating rounds.

Part 1, the kernels on seeded data already on the device:
* ``fit, iters 0`` / ``fit, iters 4``   ``mg_depth_align_fit`` from (1, 0): 2 and 8 launches, nothing read back
* ``apply``                             ``mg_depth_align_apply``
* ``torch fp64, iters 0`` / ``iters 4``  the same fit composed from torch device ops in fp64 (masks, five sums, the solve as 0-dim
                                        tensors: no read-back either)
Part 2, ``map_video`` per frame with and without ``align=True`` under tools/sequence_bench.py's protocol: the full architecture with
synthetic weights, E = 1, frames resident in HBM, every output map on the host inside the timed region, four runs alternating - lanes 1
and 3, each with and without the alignment - T = 1 and 10, a child process each under its own time limit.  ``map_video`` without the
keyword launches nothing of the alignment: it is the measure of what the keyword adds, and of whether the extra turn costs the lanes
anything.  The first line of the log is the box's calibration (``mg_clock_probe``).  Needs an MI355X.

    python tools/align_bench.py [--rounds 50] [--log profiles/depth_align.log]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 3
RUNS = (("1", "map_video in_flight=1            ", 1, None), ("1a", "map_video in_flight=1 align=True", 1, True),
        ("3", "map_video in_flight=3            ", 3, None), ("3a", "map_video in_flight=3 align=True", 3, True))


def _stat(v):
    return f"{statistics.median(v):8.4f}  ({min(v):.4f} - {max(v):.4f})"


def _alternate(torch, rounds, pairs):
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


def _torch_fit(torch, d, ref, iters, delta):
    """The definition from torch device ops in fp64; nothing leaves the device."""
    x, g = d.double().reshape(-1), ref.double().reshape(-1)
    ok = (torch.isfinite(x) & torch.isfinite(g)).double()
    x, g = torch.nan_to_num(x, 0.0, 0.0, 0.0), torch.nan_to_num(g, 0.0, 0.0, 0.0)

    def solve(w):
        wd = w * x
        N, Sd, Sg, Sdd, Sdg = w.sum(), wd.sum(), (w * g).sum(), (wd * x).sum(), (wd * g).sum()
        s = (N * Sdg - Sd * Sg) / (N * Sdd - Sd * Sd)
        return s, (Sg - s * Sd) / N
    if iters == 0:
        return solve(ok)
    s, t = torch.ones((), dtype=torch.float64, device=d.device), torch.zeros((), dtype=torch.float64, device=d.device)
    for _ in range(iters):
        r = ((s * x + t) - g) / delta
        s, t = solve(ok / (1.0 + r * r))
    return s, t


def kernels(args):
    import torch
    from marigold_amd import _lib as L, align
    lib = L.init(0)
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0, ctypes.byref(mhz), ctypes.byref(tflops)),
            "mg_clock_probe", lib)
    n = args.res * args.res
    lines = [f"calibration of this box (mg_clock_probe, random operands): shader clock {mhz.value:.0f} MHz under matrix load, "
             f"{tflops.value:.0f} TFLOP/s bf16 MFMA chain; torch {torch.__version__}",
             f"part 1: {args.res} x {args.res}, {args.rounds} alternating rounds after {WARM} warm-up rounds; device events; ms, median (min - max)"]
    g = torch.Generator().manual_seed(0)
    ref = torch.rand(args.res, args.res, generator=g)
    d = (ref - 0.07) / 0.8 + 0.01 * torch.randn(args.res, args.res, generator=g)
    d.reshape(-1)[:n // 5] = 0.05
    d, ref = d.cuda(), ref.cuda()
    out = torch.empty_like(d)
    coef, _ = align.fit(d, ref, iters=4, lib=lib)
    pairs = [("fit, iters 0 (2 launches)", lambda: align.fit(d, ref, iters=0, lib=lib)),
             ("fit, iters 4 (8 launches)", lambda: align.fit(d, ref, iters=4, lib=lib)),
             ("apply", lambda: align.apply(d, coef, out=out, lib=lib)),
             ("torch fp64, iters 0", lambda: _torch_fit(torch, d, ref, 0, 0.05)),
             ("torch fp64, iters 4", lambda: _torch_fit(torch, d, ref, 4, 0.05))]
    t = _alternate(torch, args.rounds, pairs)
    for label, _ in pairs:
        lines.append(f"  {label:28s} {_stat(t[label])}")
    s, tt = _torch_fit(torch, d, ref, 4, 0.05)
    lines.append(f"  (kernel s, t = {coef[0].item():.12f}, {coef[1].item():.12f}; torch {s.item():.12f}, {tt.item():.12f}; compulsory traffic of a solve "
                 f"{8 * n / 1e6:.1f} MB, of the apply {8 * n / 1e6:.1f} MB)")
    return lines


def child(args):
    import torch
    import marigold_amd as M
    from marigold_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)
    T = args.steps
    frames = [syn.synthetic_image(args.res, args.res, seed=s).to(dev) for s in range(args.frames)]
    kw = dict(denoising_steps=T, ensemble_size=1, processing_res=0, color_map=None, show_progress_bar=False)

    def run(lanes, aligned, images, seed0):
        gens = [torch.Generator(device=dev).manual_seed(seed0 + i) for i in range(len(images))]
        return [o.depth_np for o in pipe.map_video(images, strength=0.1, in_flight=lanes, generators=gens, align=aligned, **kw)]

    t0 = time.perf_counter()
    for _, _, lanes, aligned in RUNS:   # warm-up, alone: the programs of every lane built and run
        run(lanes, aligned, frames[:2 * lanes], 0)
    torch.cuda.synchronize()
    print(f"T={T:2d} warm-up {time.perf_counter() - t0:.1f} s", flush=True)
    ms = {name: [] for name, *_ in RUNS}
    for r in range(args.video_rounds):
        for name, _, lanes, aligned in RUNS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs = run(lanes, aligned, frames, 1000 * (r + 1))
            e1.record()
            torch.cuda.synchronize()
            assert len(outs) == len(frames)
            ms[name].append(e0.elapsed_time(e1) / len(frames))
    for name, label, _, _ in RUNS:
        v = ms[name]
        print(f"T={T:2d} E=1 ({name:>2}) {label}  {sum(v) / len(v):7.2f} ms/frame  (min {min(v):.2f}, max {max(v):.2f}, {len(v)} rounds of "
              f"{len(frames)} frames)", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--log", type=str, default=None)
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--steps", type=int, default=None, help="part 2 for one T, in this process")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--video_rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    args = ap.parse_args()
    if args.steps is not None:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: nothing to measure")
    lines = kernels(args)
    lines.append(f"part 2: map_video per frame, {args.res} x {args.res}, E = 1, synthetic weights, {args.video_rounds} rounds of {args.frames} frames, the four "
                 "runs alternating; mean (min, max)")
    print("\n".join(lines), flush=True)
    rc = 0
    for T in (1, 10):   # each under a time limit of its own; nothing more is started after one that failed
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--steps", str(T), "--frames", str(args.frames),
               "--video_rounds", str(args.video_rounds), "--res", str(args.res)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        print(r.stdout + r.stderr[-2000:], flush=True)
        lines += r.stdout.strip().splitlines()
        if r.returncode != 0:
            lines.append(f"T={T}: exit status {r.returncode}; stopping")
            rc = r.returncode
            break
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
