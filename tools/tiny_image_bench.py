#!/usr/bin/env python
"""C calls on a model image with the tiny autoencoder beside the same calls on an AutoencoderKL image, at 768 x 768, full UNet
architecture, synthetic weights, one process, one MI355X.

Both images are exported from one pipeline (the second with ``set_vae(AutoencoderTinyHIP)`` and ``tiny_vae=True``), each with the four
configurations the cases need, and loaded side by side.  Per case: one warm-up call on either image, then ``--rounds`` rounds in
which the two images take turns; a timed window is as many calls as fill ``--window`` seconds (sized from the warm-up, repeated
with more calls if it ended early), closed by a synchronise, and its figure is the window's wall time per call.  Printed: the
calibration line of bench.py, then mean, minimum and maximum over the rounds.

    mg_model_predict_out   E = 1, T = 1;  E = 1, T = 10;  E = 10, T = 10
    mg_model_predict_next  E = 1, T = 1   (every frame carries the one before)
    mg_model_predict_many  K = 8, E = 1, T = 10   (per call and per picture)

    python tools/tiny_image_bench.py > profiles/tiny_image_768.log
"""
import argparse
import copy
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, est_s, seconds):
    """Wall milliseconds per call over a window of at least ``seconds``, closed by a synchronise."""
    import torch
    reps = max(1, int(math.ceil(seconds / max(est_s, 1e-4))) + 1)
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / reps
        reps = int(reps * max(1.25, 1.1 * seconds / dt)) + 1


def show(label, v, extra=""):
    print(f"{label:<58} {sum(v) / len(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, {len(v)} rounds){extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, at least")
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--dir", default=None, help="where the two images are written (default: a temporary directory, removed)")
    a = ap.parse_args()
    assert a.rounds >= 3 and a.window >= 1.0, "at least three rounds of windows of at least a second"
    import torch
    import marigold_amd as M
    from marigold_amd import image, synthetic as syn
    from marigold_amd.modules import AutoencoderTinyHIP
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)
    if not a.no_calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    res = a.res
    cfg = lambda E, T, K=1: dict(ensemble_size=E, height=res, width=res, denoising_steps=T, images_per_program=K)   # noqa: E731
    # (call, E, T, K)
    cases = [("predict_out ", 1, 1, 1), ("predict_out ", 1, 10, 1), ("predict_out ", 10, 10, 1), ("predict_next", 1, 1, 1), ("predict_many", 1, 10, 8)]
    configs = [cfg(1, 1), cfg(1, 10), cfg(10, 10), cfg(1, 10, 8)]
    pipes = {"KL  ": pipe, "tiny": copy.copy(pipe).set_vae(AutoencoderTinyHIP(syn.synthetic_tiny_vae_state_dict()))}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        models = {}
        for name, p in pipes.items():
            path = os.path.join(d, name.strip() + ".mgimg")
            t0 = time.perf_counter()
            info = image.export_model_image(p, path, configs=configs, tiny_vae=name == "tiny")
            models[name] = image.ModelImage(path)
            print(f"image  {name} {info['file_bytes'] / 2 ** 20:9.1f} MiB file, shared {models[name].shared_bytes / 2 ** 20:9.1f} MiB, private "
                  f"{models[name].device_bytes / 2 ** 20:9.1f} MiB (scratch region {info['scratch_bytes'] / 2 ** 20:.1f} MiB), export + load "
                  f"{time.perf_counter() - t0:.1f} s", flush=True)
            os.remove(path)
        del pipes, pipe
        torch.cuda.empty_cache()
        u8s = [syn.synthetic_image(res, res, seed=5 + i)[0].permute(1, 2, 0).contiguous().to(dev) for i in range(8)]
        for call, E, T, K in cases:
            runs = {}
            for name, mi in models.items():
                mi.select(mi.find(res, res, E, T, K))
                if call.startswith("predict_many"):
                    fn = lambda mi=mi: mi.predict_many(u8s, range(11, 19))   # noqa: E731
                elif call.startswith("predict_next"):
                    mi.seq_reset()
                    fn = lambda mi=mi: mi.predict_next(u8s[0], 11, 0.1)   # noqa: E731
                else:
                    fn = lambda mi=mi: mi.predict_out(u8s[0], 11)   # noqa: E731
                fn()   # warm-up (the first call allocates the handle's temporaries), then an estimate for the window
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                runs[name] = (fn, time.perf_counter() - t0, [])
            for _ in range(a.rounds):
                for name, mi in models.items():
                    mi.select(mi.find(res, res, E, T, K))   # (selecting starts a new sequence: the first frame of a window carries nothing)
                    fn, est, v = runs[name]
                    v.append(window(fn, est, a.window))
            for name in models:
                v = runs[name][2]
                per = f"  {sum(v) / len(v) / K:8.3f} ms per picture" if K > 1 else ""
                show(f"C call {name} mg_model_{call} E={E:2d} T={T:2d} K={K}", v, per)
        for mi in models.values():
            mi.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
