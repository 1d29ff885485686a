#!/usr/bin/env python
"""What depth to 3D costs, at 768 x 768 and 3000 x 4000, with a random half of the pixels kept and with everything kept,
by device events, alternating rounds, median with min - max.  Per size and mask, on seeded data already on the device:
* ``mg_depth_points``            xyz and colours, three launches, nothing read back
* ``mg_depth_points + normals``  the same with the normal of every record
* ``torch ops``                  the same cloud from torch device ops in fp64: unprojection, the mask, ``torch.nonzero``, gathers of the
                                 points and the colours - including the synchronisation ``nonzero`` forces to size its result
* ``HBM time``                   the compulsory traffic at the copy rate measured on this box just before: two passes over the depths
                                 (4 n bytes each), the mask (n each) where there is one, and per kept record 3 bytes of colour read and
                                 15 (27 with normals) written; the torch composition moves several times that
The first line of the log is the box's calibration (``mg_clock_probe`` and a device-to-device copy of 256 MiB).  Needs an MI355X.

    python tools/points_bench.py [--rounds 30] [--log profiles/points.log]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 3


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


def _torch_cloud(torch, depth, K, colors, mask, coef):
    """The same records from torch device ops (no flying-pixel rule, no normals): what a caller would write without the kernel."""
    h, w = depth.shape
    z = depth.double() * coef[0] + coef[1]
    keep = torch.isfinite(z) & (z > 0)
    if mask is not None:
        keep &= mask != 0
    xs = torch.arange(w, device=depth.device, dtype=torch.float64)[None, :]
    ys = torch.arange(h, device=depth.device, dtype=torch.float64)[:, None]
    xyz = torch.stack([((xs - K.cx) * z) / K.fx, ((ys - K.cy) * z) / K.fy, z], dim=-1).float()
    index = torch.nonzero(keep.reshape(-1)).reshape(-1)   # synchronises: the host must learn the count
    return xyz.reshape(-1, 3)[index], colors.reshape(-1, 3)[index], index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "points.log"))
    args = ap.parse_args()
    import torch
    from marigold_amd import _lib as L, points as P
    lib = L.init(0)
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0, ctypes.byref(mhz), ctypes.byref(tflops)),
            "mg_clock_probe", lib)
    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    copy = _alternate(torch, 10, [("copy", lambda: b.copy_(a))])["copy"]
    gbs = 2 * a.numel() / (statistics.median(copy) * 1e-3) / 1e9   # read + write
    del a, b
    lines = [f"calibration of this box: shader clock {mhz.value:.0f} MHz under matrix load (mg_clock_probe), {tflops.value:.0f} TFLOP/s bf16 MFMA "
             f"chain; device-to-device copy of 256 MiB {gbs:.0f} GB/s (read + write); torch {torch.__version__}",
             f"{args.rounds} alternating rounds after {WARM} warm-up rounds; device events; ms, median (min - max)"]
    coef = (9.0, 1.0)
    for h, w in ((768, 768), (3000, 4000)):
        g = torch.Generator().manual_seed(h)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        depth = (0.5 + 0.3 * torch.sin(xs / 97.0) * torch.cos(ys / 61.0) + 0.001 * torch.randn(h, w, generator=g)).cuda()
        colors = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda()
        K = P.intrinsics_from_fov(h, w, 60.0)
        n = h * w
        for what, mask in (("everything kept", None), ("a random half kept", (torch.rand(h, w, generator=g) < 0.5).cuda())):
            kw = dict(colors=colors, mask=mask, coef=coef, lib=lib)
            kept = int(P.depth_to_points(depth, K, **kw).count[0])
            pairs = [("mg_depth_points          ", lambda: P.depth_to_points(depth, K, **kw)),
                     ("mg_depth_points + normals", lambda: P.depth_to_points(depth, K, normals=True, **kw)),
                     ("torch ops (with the sync)", lambda: _torch_cloud(torch, depth, K, colors, mask, coef))]
            times = _alternate(torch, args.rounds, pairs)
            lines.append(f"{h} x {w}, {what}: {kept} of {n} records")
            for label, _ in pairs:
                lines.append(f"  {label}  {_stat(times[label])}")
            for label, rec in (("HBM time                 ", 15), ("HBM time, with normals   ", 27)):
                traffic = 2 * (4 * n + (n if mask is not None else 0)) + kept * (3 + rec)
                lines.append(f"  {label}  {traffic / (gbs * 1e9) * 1e3:8.4f}  ({traffic / 1e6:.1f} MB at the copy rate)")
    text = "\n".join(lines)
    print(text)
    with open(args.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
