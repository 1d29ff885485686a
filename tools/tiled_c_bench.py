#!/usr/bin/env python
"""The tiled prediction of a large picture as ONE C call (``mg_model_predict_tiled``) beside ``pipe.predict_tiled(in_flight=1,
tiles_per_program=K)``, which strings the same programs and kernels together from Python, and the tile gather ``mg_tile_crop`` beside
the torch slicing it stands for: depth, 3 000 x 4 000, tiles of 768, overlap 192 (5 x 7 = 35 tiles, guide 576 x 768), E = 1, T = 10 on
the full architecture with synthetic weights - the workload of docs/history/tiled.md.  No quality is measured: the weights are
synthetic.

One model image of three configurations (guide, K tiles per call, and the 35 mod K tiles of the short last group) is exported to
--dir (a few GB, removed once loaded) and driven through ctypes, which is what a C host does minus the process start.  Per call: the
host clock around a call that ends in a stream synchronise and the read-back of the map and the picture, which the Python call
includes; the picture is resident in HBM as uint8 for both.  One warm-up round, then --rounds rounds that visit the forms in turn, so
that they alternate within one session on one box; median with min - max.  The box calibration of bench.py comes first.

    python tools/tiled_c_bench.py
    python tools/tiled_c_bench.py --height 1536 --width 1536 --steps 4 --rounds 3
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--tile", type=int, default=768)
    ap.add_argument("--overlap", type=int, default=192)
    ap.add_argument("--guide-res", type=int, default=768)
    ap.add_argument("--k", type=int, default=8, help="tiles per program")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ensemble", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--crop-reps", type=int, default=50, help="timed gathers per form per round")
    ap.add_argument("--dir", type=str, default=None, help="where the model image is written (default: a temporary directory)")
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import marigold_amd as M
    from marigold_amd import image, synthetic as syn, tiles as tiling
    from marigold_amd.util.image_util import colormap_lut_u8, max_res_size
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=args.guide_res).to(dev)   # binds the library to the device
    if not args.no_calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    H, W, T, E, K = args.height // 8 * 8, args.width // 8 * 8, args.steps, args.ensemble, args.k
    plan = tiling.plan((H, W), args.tile, args.overlap)
    n, (th, tw) = len(plan.origins), plan.tile_hw
    hg, wg = max_res_size((H, W), args.guide_res)
    print(f"picture {H} x {W}, {len(plan.ystarts)} x {len(plan.xstarts)} = {n} tiles of {th} x {tw}, overlap {args.overlap}, guide {hg} x {wg}, "
          f"E = {E}, T = {T}, {K} tiles per program", flush=True)
    chw = syn.synthetic_image(H, W, seed=3).to(dev)            # uint8 [1,3,H,W]: what predict_tiled takes
    hwc = chw[0].permute(1, 2, 0).contiguous()                 # uint8 [H,W,3]: what the C entry takes
    lut = torch.from_numpy(colormap_lut_u8("Spectral")).to(dev)
    seed = 1000
    cfg = lambda h, w, k: dict(ensemble_size=E, height=h, width=w, denoising_steps=T, images_per_program=k)   # noqa: E731
    configs = [cfg(hg, wg, 1), cfg(th, tw, K)] + ([cfg(th, tw, n % K)] if n % K else [])
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "tiled.mgimg")
        t0 = time.perf_counter()
        info = image.export_model_image(pipe, path, configs=configs)
        mi = image.ModelImage(path)
        os.remove(path)   # loaded: the file is no longer needed
    guide_cfg, tile_cfg = mi.find(hg, wg, E, T, 1), mi.find(th, tw, E, T, K)
    tail_cfg = mi.find(th, tw, E, T, n % K) if n % K else None
    print(f"image of {info['file_bytes'] / 1e9:.2f} GB exported and loaded in {time.perf_counter() - t0:.1f} s, "
          f"{mi.device_bytes / 1e9:.2f} GB on the device", flush=True)

    def c_call(tail):
        t0 = time.perf_counter()
        pred, _, _, pic, _, flags = mi.predict_tiled(hwc, seed, guide_cfg, tile_cfg, args.overlap, tail_config=tail, lut=lut, picture=True,
                                                     mode="bilinear")
        torch.cuda.current_stream().synchronize()
        out = (pred.cpu(), pic.cpu(), int(flags.sum().item()))
        return (time.perf_counter() - t0) * 1e3, out

    def py_call():
        t0 = time.perf_counter()
        out = pipe.predict_tiled(chw, tile_size=args.tile, tile_overlap=args.overlap, guide_res=args.guide_res, tiles_per_program=K, in_flight=1,
                                 generator=M.NativeNoise(seed), denoising_steps=T, ensemble_size=E, show_progress_bar=False)
        torch.cuda.current_stream().synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    crop_out = torch.empty(n * 3 * th * tw, dtype=torch.uint8, device=dev)

    def crop_c():
        torch.cuda.current_stream().synchronize()
        t0 = time.perf_counter()
        for _ in range(args.crop_reps):
            tiling.crop(chw, plan, 0, n, out=crop_out)
        torch.cuda.current_stream().synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.crop_reps, None

    def crop_torch():
        torch.cuda.current_stream().synchronize()
        t0 = time.perf_counter()
        for _ in range(args.crop_reps):
            crops = [chw[..., y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0 in plan.origins]
        torch.cuda.current_stream().synchronize()
        del crops
        return (time.perf_counter() - t0) * 1e3 / args.crop_reps, None

    forms = [("mg_model_predict_tiled (tail configuration)", lambda: c_call(tail_cfg)),
             ("mg_model_predict_tiled (short last group padded)", lambda: c_call(None)),
             ("pipe.predict_tiled(in_flight=1)", py_call),
             (f"mg_tile_crop, {n} tiles in one launch", crop_c),
             (f"torch slicing + contiguous, {n} tiles", crop_torch)]
    if tail_cfg is None:
        forms.pop(1)
    times, last = {name: [] for name, _ in forms}, {}
    for rnd in range(args.rounds + 1):   # round 0 warms up
        for name, run in forms:
            ms, last[name] = run()
            if rnd:
                times[name].append(ms)
    for name, _ in forms:
        t = times[name]
        print(f"{name:52s} {statistics.median(t):10.3f} ms  (min {min(t):.3f}, max {max(t):.3f}, {len(t)} rounds)", flush=True)
    # the two routes on the same bytes: the same map, picture and flag count
    c_out, py_out = last[forms[0][0]], last["pipe.predict_tiled(in_flight=1)"]
    same = bool((c_out[0][0].numpy() == py_out.depth_np).all()) and bool((c_out[1].numpy() == np.asarray(py_out.depth_colored)).all())
    print(f"C call (tail configuration) == pipe.predict_tiled, map and picture bit for bit: {same}; degenerate tiles {c_out[2]} / "
          f"{py_out.degenerate_tiles}; handle memory after the calls {mi.device_bytes / 1e9:.2f} GB", flush=True)
    mi.close()


if __name__ == "__main__":
    main()
