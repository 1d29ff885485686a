#!/usr/bin/env python
"""The tiny autoencoder beside the SD AutoencoderKL at 768 x 768, full UNet architecture, synthetic weights, one process.

Three levels, every pair of runs alternating round after round so that drift of the box hits both alike; figures are the mean of
the rounds with their minimum and maximum, timed with HIP events on the caller's stream after a warm-up pass of every run:
    layer    mg_tiny_conv3x3 at the decoder's four sizes (E = 10 and E = 1), plain, the stride-2 and the nearest-x2 forms: achieved TFLOP/s
             and GB/s beside the layer's FLOP (2 * 9 * 64 * 64 per output pixel) and byte counts (input + output + residual lines)
    module   encode_rgb_latent (one image) and decode (E = 1, E = 10 members) of both VAE modules
    map      map_images at (E, T) = (10, 10), (1, 10), (1, 4), (1, 1) and map_video at E = 1, T = 1, per image / frame

    python tools/tiny_vae_bench.py > profiles/tiny_vae_768.log
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def show(label, v, extra=""):
    print(f"{label:<58} {sum(v) / len(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, {len(v)} rounds){extra}", flush=True)


def layer_level(lib, dev, rounds, res):
    import torch
    from marigold_amd import _lib as L, ops as O
    w = (torch.randn(9, 64, 64, device=dev) * (2.0 / 576) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(64, device=dev) * 0.1
    cases = [(f"stride 1  B={B} {s}x{s} +bias +res +relu", B, s, 1, 0, True) for B in (10, 1) for s in (res, res // 2, res // 4, res // 8)]
    cases += [(f"stride 1  B=10 {res}x{res} plain", 10, res, 1, 0, False)]
    cases += [(f"stride 2  B=1 {res}x{res} -> {res // 2}", 1, res, 2, 0, False), (f"nearest x2  B=10 {res // 2} -> {res}", 10, res // 2, 1, 1, False)]
    runs = []
    for label, B, s, stride, up2, full in cases:
        so = s // 2 if stride == 2 else s * (2 if up2 else 1)
        x = torch.randn(B, s, s, 64, device=dev).to(torch.bfloat16)
        r = torch.randn(B, so, so, 64, device=dev).to(torch.bfloat16) if full else None
        out = torch.empty(B, so, so, 64, device=dev, dtype=torch.bfloat16)

        def fn(x=x, r=r, out=out, B=B, s=s, stride=stride, up2=up2, full=full):
            L.check(lib.mg_tiny_conv3x3(x.data_ptr(), w.data_ptr(), bias.data_ptr() if full else None, r.data_ptr() if full else None,
                                        out.data_ptr(), B, s, s, stride, up2, int(full), O.current_stream_handle()), "mg_tiny_conv3x3", lib)
        flop = 2.0 * 9 * 64 * 64 * B * so * so
        nbytes = 128.0 * (B * s * s + B * so * so * (2 if full else 1))
        fn()
        runs.append((label, fn, flop, nbytes, []))
    for _ in range(rounds):
        for _, fn, _, _, v in runs:
            v.append(timed(fn, 10))
    for label, _, flop, nbytes, v in runs:
        ms = sum(v) / len(v)
        show("layer  " + label, v, f"  {flop / 1e9:8.2f} GFLOP {nbytes / 1e6:8.1f} MB -> {flop / ms / 1e9:7.1f} TFLOP/s {nbytes / ms / 1e6:7.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=12, help="images per map-level run at E = 1 (a third of it at E = 10)")
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--levels", default="layer,module,map")
    a = ap.parse_args()
    import torch
    import marigold_amd as M
    from marigold_amd import _lib as L, synthetic as syn
    from marigold_amd.modules import AutoencoderTinyHIP
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)
    if not a.no_calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    kl, tiny = pipe.vae, AutoencoderTinyHIP(syn.synthetic_tiny_vae_state_dict()).to(dev)
    res, levels = a.res, a.levels.split(",")
    if "layer" in levels:
        layer_level(L.load(), dev, a.rounds, res)
    if "module" in levels:
        rgb = (syn.synthetic_image(res, res)[0:1].float() / 127.5 - 1.0).to(dev)
        runs = []
        for E in (1, 10):
            z = syn.synthetic_latents(E, res // 8, res // 8).to(dev)
            for name, vae in (("KL  ", kl), ("tiny", tiny)):
                runs.append((f"module {name} decode E={E}", lambda vae=vae, z=z: vae.decode(z, post=L.POST_DEPTH), []))
        for name, vae in (("KL  ", kl), ("tiny", tiny)):
            runs.append((f"module {name} encode one image", lambda vae=vae: vae.encode_rgb_latent(rgb), []))
        for _, fn, _ in runs:
            fn()
        for _ in range(a.rounds):
            for _, fn, v in runs:
                v.append(timed(fn, 3))
        for label, _, v in runs:
            show(label, v)
    if "map" in levels:
        pipes = {"KL  ": pipe, "tiny": copy.copy(pipe).set_vae(tiny)}
        frames = [syn.synthetic_image(res, res, seed=s).to(dev) for s in range(a.images)]
        for what, E, T in (("map_images", 10, 10), ("map_images", 1, 10), ("map_images", 1, 4), ("map_images", 1, 1), ("map_video ", 1, 1)):
            imgs = frames[:max(2, a.images // 3)] if E > 1 else frames
            kw = dict(denoising_steps=T, ensemble_size=E, processing_res=0, color_map=None, show_progress_bar=False)

            def run(p, imgs=imgs, kw=kw, what=what):
                gens = [torch.Generator(device=dev).manual_seed(7 + i) for i in range(len(imgs))]
                outs = p.map_video(imgs, generators=gens, **kw) if what.startswith("map_video") else p.map_images(imgs, generators=gens, **kw)
                return [o.depth_np for o in outs]
            ms = {n: [] for n in pipes}
            for n, p in pipes.items():
                run(p)
            for _ in range(a.rounds):
                for n, p in pipes.items():
                    ms[n].append(timed(lambda p=p: run(p), 1) / len(imgs))
            for n in pipes:
                show(f"map    {n} {what} E={E:2d} T={T:2d} per image ({len(imgs)} images)", ms[n])
    return 0


if __name__ == "__main__":
    sys.exit(main())
