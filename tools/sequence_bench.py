#!/usr/bin/env python
"""Per-frame cost of an image sequence (``map_video``: every frame starts from the denoised latent of the frame before) beside
independent maps (``map_images``), at 768 x 768, E = 1, on the full architecture with synthetic weights.

Four runs alternate within one process, round after round, so that drift of the box hits them alike:
    (i)   map_images(in_flight=1)      one map after the other, no carry
    (ii)  map_video(in_flight=1)       the same with the carry: the blend and the copy of the latent are all it adds
    (iii) map_video(in_flight=3)       only the denoise stages take turns; encode, decode and output stage overlap
    (iv)  map_images(in_flight=3)      the ceiling: no dependency between the maps at all
Each run: N frames (uint8 tensors resident in HBM, one noise generator each) timed with HIP events on the caller's stream, every
output map on the host inside the timed region, as bench.py does.  A warm-up pass of every run comes first, alone.  Reported: the
mean of the rounds in ms per frame, with their minimum and maximum.

    python tools/sequence_bench.py                 # T = 1, 4, 10: one child process per T, each under its own time limit
    python tools/sequence_bench.py --steps 4       # one T, in this process
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = (("i", "map_images in_flight=1", "images", 1), ("ii", "map_video  in_flight=1", "video", 1),
        ("iii", "map_video  in_flight=3", "video", 3), ("iv", "map_images in_flight=3", "images", 3))


def child(args):
    import torch
    import marigold_amd as M
    from marigold_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)   # binds the library to the device
    if args.calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    T = args.steps
    frames = [syn.synthetic_image(args.res, args.res, seed=s).to(dev) for s in range(args.frames)]
    assert frames[0].dtype == torch.uint8
    kw = dict(denoising_steps=T, ensemble_size=1, processing_res=0, color_map=None, show_progress_bar=False)

    def run(what, lanes, images, seed0):
        gens = [torch.Generator(device=dev).manual_seed(seed0 + i) for i in range(len(images))]
        if what == "video":
            outs = pipe.map_video(images, strength=args.strength, in_flight=lanes, generators=gens, **kw)
        else:
            outs = pipe.map_images(images, in_flight=lanes, generators=gens, **kw)
        return [o.depth_np for o in outs]

    t0 = time.perf_counter()
    for _, _, what, lanes in RUNS:   # warm-up, alone: the programs of every lane built and run
        run(what, lanes, frames[:2 * lanes], 0)
    torch.cuda.synchronize()
    print(f"T={T:2d} warm-up {time.perf_counter() - t0:.1f} s", flush=True)
    ms = {name: [] for name, *_ in RUNS}
    for r in range(args.rounds):
        for name, _, what, lanes in RUNS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs = run(what, lanes, frames, 1000 * (r + 1))
            e1.record()
            torch.cuda.synchronize()
            assert len(outs) == len(frames)
            ms[name].append(e0.elapsed_time(e1) / len(frames))
    for name, label, _, _ in RUNS:
        v = ms[name]
        print(f"T={T:2d} E=1 ({name:>3}) {label}  {sum(v) / len(v):7.2f} ms/frame  (min {min(v):.2f}, max {max(v):.2f}, {len(v)} rounds of "
              f"{len(frames)} frames)", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None, help="one T, in this process (default: 1, 4 and 10, a child process each)")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--strength", type=float, default=0.1)
    ap.add_argument("--calibration", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    args = ap.parse_args()
    if args.steps is not None:
        return child(args)
    for n, T in enumerate((1, 4, 10)):   # each step under a time limit of its own; nothing more is started after one that failed
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--steps", str(T), "--frames", str(args.frames),
               "--rounds", str(args.rounds), "--res", str(args.res), "--strength", str(args.strength)] + (["--calibration"] if n == 0 else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"T={T}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
