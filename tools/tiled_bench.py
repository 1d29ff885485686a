#!/usr/bin/env python
"""Times the stitch of a tiled prediction on the GPU box: 35 depth tiles of 768 x 768 (5 x 7, overlap 192) over a
3 000 x 4 000 canvas, fitted to a 576 x 768 guide and blended - three ways, alternating, on the same seeded data:

* kernels: ``tiles.fit`` + ``tiles.blend`` (csrc/tiles.hip), the tiles resident on the device;
* torch: the same stitch composed from torch device ops (``F.interpolate`` of the guide, masked sums per tile in fp64, a loop of
  slice updates for the feathered sums), the tiles resident on the device;
* numpy: 35 read-backs, then the stitch on the host (torch's CPU ``F.interpolate`` for the guide, numpy for the rest).

Host clock around work that ends with the stream drained (the device forms leave the canvas on the device; its read-back, which
every form's caller pays once, is timed on its own line).  Then, once (``--pipeline``): the whole ``predict_tiled`` call at E = 1,
T = 10 on the full architecture with synthetic weights beside ``map_images(images_per_program=8)`` over the same 35 crops - the
difference is what the guide, the fit and the blend cost.  The first line of the log is the box's calibration (``mg_clock_probe``).
Needs an MI355X.

    python tools/tiled_bench.py [--rounds 5] [--pipeline] [--log profiles/tiled_stage.log]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WARM = 1
CANVAS, TILE, OVERLAP, GUIDE = (3000, 4000), 768, 192, (576, 768)


def _stat(v):
    return f"{statistics.median(v):9.3f}  ({min(v):.3f} - {max(v):.3f})"


def _alternate(rounds, pairs):
    """pairs: [(label, fn)] -> {label: [ms]}; fn() does the work and returns when it is complete."""
    times = {label: [] for label, _ in pairs}
    for r in range(rounds + WARM):
        for label, fn in pairs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[label].append(dt)
    return times


def _ramp(T, O, before, behind, xp, **kw):
    u = xp.arange(T, **kw)
    lo = xp.minimum(1.0, (u + 0.5) / O) if before else xp.ones(T, **kw)
    hi = xp.minimum(1.0, (T - u - 0.5) / O) if behind else xp.ones(T, **kw)
    return xp.minimum(lo, hi)


def _torch_ramp(T, O, before, behind, device):
    u = torch.arange(T, dtype=torch.float32, device=device)
    one = torch.ones(T, device=device)
    lo = torch.clamp((u + 0.5) / O, max=1.0) if before else one
    hi = torch.clamp((T - u - 0.5) / O, max=1.0) if behind else one
    return torch.minimum(lo, hi)


def stitch_torch(tiles, plan, guide):
    """The stitch from torch ops on the tiles' device -> the canvas [H,W] fp32."""
    H, W = CANVAS
    full = F.interpolate(guide[None, None], (H, W), mode="bilinear", align_corners=False)[0, 0]
    ny, nx = len(plan.ystarts), len(plan.xstarts)
    num, den = torch.zeros(H, W, device=tiles.device), torch.zeros(H, W, device=tiles.device)
    crops = torch.stack([full[y0:y0 + TILE, x0:x0 + TILE] for y0, x0 in plan.origins]).double()
    d = tiles.double()
    ok = torch.isfinite(d) & torch.isfinite(crops)
    d0, g0 = torch.where(ok, d, 0.0), torch.where(ok, crops, 0.0)
    N, Sd, Sg = ok.sum((1, 2)).double(), d0.sum((1, 2)), g0.sum((1, 2))
    Sdd, Sdg = (d0 * d0).sum((1, 2)), (d0 * g0).sum((1, 2))
    det = N * Sdd - Sd * Sd
    s = (N * Sdg - Sd * Sg) / det
    good = (N >= 2) & (det > 1e-12 * N * N) & (s > 0)
    s = torch.where(good, s, 0.0)
    t = torch.where(good, (Sg - s * Sd) / N, Sg / N.clamp(min=1))
    s, t = s.float(), t.float()
    for i, (y0, x0) in enumerate(plan.origins):
        iy, ix = divmod(i, nx)
        w = torch.outer(_torch_ramp(TILE, OVERLAP, iy > 0, iy < ny - 1, tiles.device), _torch_ramp(TILE, OVERLAP, ix > 0, ix < nx - 1, tiles.device))
        num[y0:y0 + TILE, x0:x0 + TILE] += w * (s[i] * tiles[i] + t[i])
        den[y0:y0 + TILE, x0:x0 + TILE] += w
    return num / den


def stitch_numpy(tiles_dev, plan, guide_dev):
    """35 read-backs, then the stitch on the host -> the canvas [H,W] fp32."""
    H, W = CANVAS
    host = [tiles_dev[i].cpu().numpy() for i in range(tiles_dev.shape[0])]
    full = F.interpolate(guide_dev.cpu()[None, None], (H, W), mode="bilinear", align_corners=False)[0, 0].numpy()
    ny, nx = len(plan.ystarts), len(plan.xstarts)
    num, den = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for i, (y0, x0) in enumerate(plan.origins):
        iy, ix = divmod(i, nx)
        d = host[i].astype(np.float64)
        G = full[y0:y0 + TILE, x0:x0 + TILE].astype(np.float64)
        ok = np.isfinite(d) & np.isfinite(G)
        N = float(ok.sum())
        d0, g0 = np.where(ok, d, 0.0), np.where(ok, G, 0.0)
        Sd, Sg, Sdd, Sdg = d0.sum(), g0.sum(), (d0 * d0).sum(), (d0 * g0).sum()
        det = N * Sdd - Sd * Sd
        s = (N * Sdg - Sd * Sg) / det if N >= 2 and det > 1e-12 * N * N else 0.0
        s, t = (s, (Sg - s * Sd) / N) if s > 0 else (0.0, Sg / max(N, 1.0))
        w = np.outer(_ramp(TILE, OVERLAP, iy > 0, iy < ny - 1, np, dtype=np.float32), _ramp(TILE, OVERLAP, ix > 0, ix < nx - 1, np, dtype=np.float32))
        num[y0:y0 + TILE, x0:x0 + TILE] += w * (np.float32(s) * host[i] + np.float32(t))
        den[y0:y0 + TILE, x0:x0 + TILE] += w
    return num / den


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pipeline", action="store_true", help="also time the whole predict_tiled call once (full architecture, E = 1, T = 10)")
    ap.add_argument("--pipeline-rounds", type=int, default=3)
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: nothing to measure")
    from marigold_amd import _lib as L, tiles as T
    from marigold_amd.util.host import usable_cores
    torch.set_num_threads(min(16, usable_cores()))
    lib = L.init(0)
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0, ctypes.byref(mhz), ctypes.byref(tflops)),
            "mg_clock_probe", lib)
    lines = [f"calibration of this box (mg_clock_probe, random operands): shader clock {mhz.value:.0f} MHz under matrix load, "
             f"{tflops.value:.0f} TFLOP/s bf16 MFMA chain; torch {torch.__version__}, {usable_cores()} usable host cores, "
             f"{torch.get_num_threads()} torch threads",
             f"{args.rounds} alternating rounds after {WARM} warm-up round; ms, median (min - max)"]
    dev = torch.device("cuda:0")
    plan = T.plan(CANVAS, TILE, OVERLAP)
    n = len(plan.origins)
    H, W = CANVAS
    # a smooth map, its low-resolution copy as the guide, and per tile an affinely distorted crop
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(1, 1, 12, 16, generator=g)
    truth = F.interpolate(coarse, (H, W), mode="bicubic", align_corners=False).clamp(0, 1)[0, 0]
    guide = F.interpolate(truth[None, None], GUIDE, mode="bilinear", align_corners=False, antialias=True)[0, 0].contiguous().to(dev)
    s = 0.5 + torch.rand(n, generator=g)
    t = torch.rand(n, generator=g) * 0.4 - 0.2
    tiles = torch.stack([(truth[y0:y0 + TILE, x0:x0 + TILE] - t[i]) / s[i] for i, (y0, x0) in enumerate(plan.origins)]).contiguous().to(dev)

    def kernels():
        coef, _ = T.fit(tiles, plan.origins, guide, CANVAS)
        out = T.blend(tiles, plan.origins, CANVAS, OVERLAP, coef=coef)
        torch.cuda.synchronize()
        return out

    def torch_ops():
        out = stitch_torch(tiles, plan, guide)
        torch.cuda.synchronize()
        return out

    a, b, c = kernels().cpu().numpy(), torch_ops().cpu().numpy(), stitch_numpy(tiles, plan, guide)
    times = _alternate(args.rounds, [("kernels", kernels), ("torch", torch_ops), ("numpy", lambda: stitch_numpy(tiles, plan, guide))])
    canvas = kernels()
    readback = _alternate(args.rounds, [("readback", lambda: canvas.cpu())])["readback"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fit_ms, blend_ms = [], []
    for r in range(args.rounds + WARM):
        ev[0].record()
        coef, _ = T.fit(tiles, plan.origins, guide, CANVAS)
        ev[1].record()
        T.blend(tiles, plan.origins, CANVAS, OVERLAP, coef=coef)
        ev[2].record()
        ev[2].synchronize()
        if r >= WARM:
            fit_ms.append(ev[0].elapsed_time(ev[1]))
            blend_ms.append(ev[1].elapsed_time(ev[2]))
    tile_bytes, canvas_bytes = n * TILE * TILE * 4, H * W * 4
    lines += [f"stitch of {n} depth tiles of {TILE} x {TILE} (overlap {OVERLAP}) over {H} x {W}, guide {GUIDE[0]} x {GUIDE[1]}; fit + blend, stream drained:",
              f"  {'kernels (tiles.fit + tiles.blend)':40s} {_stat(times['kernels'])}",
              f"  {'torch device ops':40s} {_stat(times['torch'])}",
              f"  {'numpy after 35 read-backs':40s} {_stat(times['numpy'])}",
              f"  {'read-back of the canvas (any form)':40s} {_stat(readback)}",
              f"  {'mg_tile_fit launches (device events)':40s} {_stat(fit_ms)}   ({tile_bytes / 1e6:.0f} MB read: "
              f"{tile_bytes / 1e6 / statistics.median(fit_ms):.0f} GB/s)",
              f"  {'mg_tile_blend launch (device events)':40s} {_stat(blend_ms)}   ({(tile_bytes + canvas_bytes) / 1e6:.0f} MB read and written: "
              f"{(tile_bytes + canvas_bytes) / 1e6 / statistics.median(blend_ms):.0f} GB/s)",
              f"  largest difference to the truth: kernels {np.abs(a - truth.numpy()).max():.2e}, torch {np.abs(b - truth.numpy()).max():.2e}, "
              f"numpy {np.abs(c - truth.numpy()).max():.2e}; kernels against torch {np.abs(a - b).max():.2e}"]
    print("\n".join(lines), flush=True)

    if args.pipeline:
        import marigold_amd as M
        from marigold_amd import NativeNoise, synthetic as syn
        pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=768).to(dev)
        image = syn.synthetic_image(H, W, seed=3)
        crops = [image[..., y0:y0 + TILE, x0:x0 + TILE].contiguous().to(dev) for y0, x0 in plan.origins]
        kw = dict(denoising_steps=10, ensemble_size=1)
        seeds = lambda: [NativeNoise(100 + 1 + i) for i in range(n)]   # noqa: E731

        def tiled():
            out = pipe.predict_tiled(image, tile_size=TILE, tile_overlap=OVERLAP, generator=NativeNoise(100), **kw)
            torch.cuda.synchronize()
            return out

        def plain():
            outs = list(pipe.map_images(crops, generators=seeds(), images_per_program=8, processing_res=0, match_input_res=False, **kw))
            torch.cuda.synchronize()
            return outs
        out = tiled()
        pt = _alternate(args.pipeline_rounds, [("map_images", plain), ("predict_tiled", tiled)])
        lines2 = [f"whole call, full architecture with synthetic weights, E = 1, T = 10, {args.pipeline_rounds} alternating rounds after {WARM} warm-up round:",
                  f"  {'map_images(images_per_program=8), 35 crops':44s} {_stat(pt['map_images'])}   (35 maps read back)",
                  f"  {'predict_tiled (guide at 768, 35 tiles)':44s} {_stat(pt['predict_tiled'])}   (one {H} x {W} map and its picture read back)",
                  f"  degenerate tiles: {out.degenerate_tiles} of {n} (synthetic weights: the tiles need not follow the guide)"]
        print("\n".join(lines2), flush=True)
        lines += lines2
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
