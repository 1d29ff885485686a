#!/usr/bin/env python
"""Per-picture cost of the one-call C prediction with K pictures per call (``mg_model_predict_many``) beside one picture per call
(``mg_model_predict_out``, the baseline) and beside ``map_images(images_per_program=K, in_flight=1)``, which runs the same three
programs from Python: depth, 768 x 768, E = 1, T = 10 on the full architecture with synthetic weights.

A model image is exported per K (to --dir, a few GB each, removed afterwards) and loaded through ctypes, which is what a C host
does minus the process start.  Per call: the host clock around a call that ends in a stream synchronise, the pictures resident in
HBM as uint8, the outputs left on the device ("+ read-back": the maps copied to the host inside the timed region as well, which is
what the Python call includes).  3 warm-up calls per image, then --rounds rounds that visit the values of K in turn, so that K = 1
and K = 8 alternate within one session on one box; --calls timed calls per visit; the median over all timed calls of a K is
reported, as ms per call and ms per picture (call / K).  The box calibration of bench.py comes first.

    python tools/predict_many_bench.py                   # K = 1, 2, 4, 8
    python tools/predict_many_bench.py --ks 1,8 --steps 4
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
    ap.add_argument("--ks", type=str, default="1,2,4,8", help="pictures per call, comma separated (1 = mg_model_predict_out)")
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ensemble", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4, help="timed calls per K per round")
    ap.add_argument("--dir", type=str, default=None, help="where the model images are written (default: a temporary directory)")
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    import torch
    import marigold_amd as M
    from marigold_amd import image, synthetic as syn
    ks = [int(v) for v in args.ks.split(",")]
    assert args.rounds * args.calls >= 10, "at least 10 timed calls per K"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)   # binds the library to the device
    if not args.no_calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    res, E, T, kmax = args.res, args.ensemble, args.steps, max(ks)
    chw = [syn.synthetic_image(res, res, seed=s).to(dev) for s in range(kmax)]            # uint8 [1,3,H,W]: what map_images takes
    hwc = [c[0].permute(1, 2, 0).contiguous() for c in chw]                               # uint8 [H,W,3]: what the C entry takes
    seeds = [1000 + i for i in range(kmax)]
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        models = {}
        for K in ks:
            path = os.path.join(d, f"k{K}.mgimg")
            t0 = time.perf_counter()
            info = image.export_model_image(pipe, path, ensemble_size=E, height=res, width=res, denoising_steps=T, images_per_program=K)
            models[K] = image.ModelImage(path)
            os.remove(path)   # loaded: the file is no longer needed
            print(f"K={K}: image of {info['file_bytes'] / 1e9:.2f} GB exported and loaded in {time.perf_counter() - t0:.1f} s, "
                  f"{models[K]._lib.mg_model_device_bytes(models[K].handle) / 1e9:.2f} GB on the device", flush=True)

        def c_call(K, read_back):
            mi = models[K]
            t0 = time.perf_counter()
            if K == 1:
                pred = mi.predict_out(hwc[0], seeds[0])[0]
            else:
                pred = mi.predict_many(hwc[:K], seeds[:K])[0]
            torch.cuda.current_stream().synchronize()
            if read_back:
                pred.cpu()
            return (time.perf_counter() - t0) * 1e3

        def py_call(K):
            kw = dict(denoising_steps=T, ensemble_size=E, processing_res=0, color_map=None, show_progress_bar=False)
            t0 = time.perf_counter()
            outs = list(pipe.map_images(chw[:K], in_flight=1, generators=[M.NativeNoise(s) for s in seeds[:K]], images_per_program=K, **kw))
            torch.cuda.current_stream().synchronize()
            assert len(outs) == K
            return (time.perf_counter() - t0) * 1e3

        rows = [("C", K, False) for K in ks] + [("C + read-back", kmax, True), ("map_images", kmax, None)]
        times = {r: [] for r in rows}
        run = lambda r: py_call(r[1]) if r[0] == "map_images" else c_call(r[1], r[2])   # noqa: E731
        for r in rows:
            for _ in range(3):
                run(r)
        for _ in range(args.rounds):
            for r in rows:
                times[r] += [run(r) for _ in range(args.calls)]
        for r in rows:
            t = times[r]
            med = statistics.median(t)
            what = {"C": "mg_model_predict_out" if r[1] == 1 else "mg_model_predict_many"}.get(r[0], r[0])
            print(f"{what:24s} K={r[1]:2d} E={E} T={T} {res}x{res}  {med:8.2f} ms/call  {med / r[1]:7.2f} ms/picture  "
                  f"(min {min(t):.2f}, max {max(t):.2f}, {len(t)} calls)", flush=True)
        for mi in models.values():
            mi.close()


if __name__ == "__main__":
    main()
