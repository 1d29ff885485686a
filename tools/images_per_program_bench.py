#!/usr/bin/env python
"""Per-image cost of ``map_images(images_per_program=k)``: k images' members in one denoising program (k x E members), with
``in_flight`` programs on the GPU at a time, at 768 x 768 on the full architecture with synthetic weights.

For every configuration: a warm-up pass that runs alone (every lane's programs built and run once), then N images timed with
HIP events on the caller's stream between two barriers (every output map on the host inside the timed region, as bench.py
does).  The images are resident in HBM and each has its own noise generator.  The box calibration of bench.py comes first.

    python tools/images_per_program_bench.py                       # the sweep: E = 1 at T = 10 / 4, E = 2 / 5 at T = 10
    python tools/images_per_program_bench.py --only 10,1,8,2       # one configuration: T, E, k, in_flight
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sweep():
    """(T, E, k, in_flight); in_flight 0 = maps_in_flight_for(k E)"""
    out = []
    for T in (10, 4):
        for k in (1, 2, 4, 8, 10):
            out += [(T, 1, k, n) for n in (1, 2, 3)]
    for E in (2, 5):
        for k in (1, 2, 4):
            out += [(10, E, k, n) for n in (1, 0)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=40, help="timed images per configuration")
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--only", type=str, default=None, help="T,E,k,in_flight")
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    import torch
    import marigold_amd as M
    from marigold_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe0 = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)   # binds the library to the device
    if not args.no_calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    imgs = [syn.synthetic_image(args.res, args.res, seed=s).to(dev) for s in range(args.images)]
    configs = [tuple(int(v) for v in args.only.split(","))] if args.only else sweep()
    last = None
    base = None
    for T, E, k, n in configs:
        if (T, E, k) != last:   # fresh engine replicas (own workspaces and programs) over the same weights per program shape
            base = None
            gc.collect()
            torch.cuda.empty_cache()
            base = pipe0.replicate()
            last = (T, E, k)
        lanes = n or base.maps_in_flight_for(k * E)
        kw = dict(denoising_steps=T, ensemble_size=E, processing_res=0, color_map=None, show_progress_bar=False)

        def run(images, seed0):
            gens = [torch.Generator(device=dev).manual_seed(seed0 + i) for i in range(len(images))]
            return [o.depth_np for o in base.map_images(images, in_flight=lanes, generators=gens, images_per_program=k, **kw)]
        t0 = time.perf_counter()
        run(imgs[:min(len(imgs), 2 * k * lanes)], 0)   # warm-up, alone: programs of every lane built and run
        torch.cuda.synchronize()
        warm = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        outs = run(imgs, 1000)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / len(imgs)
        assert len(outs) == len(imgs)
        print(f"T={T:2d} E={E} k={k:2d} in_flight={lanes} members/program={k * E:2d}  {ms:7.2f} ms/image  "
              f"{1e3 / ms:6.2f} images/s  (warm-up {warm:.1f} s)", flush=True)


if __name__ == "__main__":
    main()
