#!/usr/bin/env python
"""What depth to focus costs at 768 x 768: the scene of tools/mesh_bench.py (tests/test_gpu_mesh.py: a smooth surface
with two steps, non-finite and out-of-range values planted) and its colours, already on the device, refocused in lens space on the flat
patch of its nearest quarter, at max_radius 8, 16 and 32 with the gain that caps about a tenth of the usable pixels, and once with
gain = 0, where every tile is in focus and the window of every target is one tap.  Alternating rounds, ms, median with min - max:
* ``mg_depth_focus``  the device call with its outputs allocated once, ``--calls`` of them queued back to back between two device
                      events, per call; nothing read back; with the contributions of ``count[3]`` and the tap tests per second, a tap
                      test being one offset of the (2 max_radius + 1)^2 window of one usable target
* ``mg_depth_view``   a view of the same map (6j) from a shifted camera, the same way, in the same session, for scale
Before anything is timed, every setting at ``--check`` x ``--check`` is held to the bytes of the numpy restatement
(tests/focus_reference.py), a size it can afford.  The first line of the log is the box's calibration (``mg_clock_probe`` and a
device-to-device copy of 256 MiB).  Needs an MI355X.
Not measured: other sizes, linear space, masks, the prepare and gather launches apart, examples/host_focus.cpp as a process; the
checkpoints of this project are synthetic, so nothing here says anything about the quality of a refocused picture.

    python tools/focus_bench.py [--rounds 10] [--calls 10] [--log profiles/focus_768.log]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 2
SIZE, RADII, EDGE, BASELINE, FILL, Z_NEAR = (768, 768), (8, 16, 32), 0.05, 0.24, 8, 1e-6


def _stat(v):
    return f"{statistics.median(v):9.4f}  ({min(v):.4f} - {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", type=int, default=192)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "focus_768.log"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from marigold_amd import _lib as L
    from tests.focus_reference import focus_reference, LENS
    from tests.points_reference import points_reference
    from tests.test_gpu_mesh import Z_RANGE, _camera, _mesh_scene
    from tests.view_reference import IDENTITY
    lib = L.init(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(stream(), 0, ctypes.byref(mhz), ctypes.byref(tflops)), "mg_clock_probe", lib)
    a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copy = []
    for r in range(10 + WARM):
        ev[0].record()
        b.copy_(a)
        ev[1].record()
        ev[1].synchronize()
        copy.append(ev[0].elapsed_time(ev[1]))
    gbs = 2 * a.numel() / (statistics.median(copy[WARM:]) * 1e-3) / 1e9   # read + write
    del a, b

    class Scene:
        def __init__(self, h, w):
            self.h, self.w, self.n = h, w, h * w
            self.d_host, self.c_host = _mesh_scene(h, w, None)
            self.focus_at = ((h // 2 - 3) // 2 + 1, (w // 2 - 3) // 2 + 1)   # the middle of the scene's flat patch, in its nearest quarter
            usable = points_reference(self.d_host, (1.0, 1.0, 0.0, 0.0), z_range=Z_RANGE).usable
            assert usable[self.focus_at]
            z = self.d_host.astype(np.float64)
            with np.errstate(all="ignore"):
                spread = np.abs(1.0 / z - 1.0 / z[self.focus_at])[usable]
            self.tenth = float(np.quantile(spread, 0.9))     # gain = max_radius / this caps about a tenth of the usable pixels
            self.depth, self.colors = torch.from_numpy(self.d_host).cuda(), torch.from_numpy(self.c_host).cuda()
            self.need = lib.mg_depth_focus_workspace_bytes(self.n)
            self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")
            self.rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
            self.valid = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            self.count = torch.empty(5, dtype=torch.int64, device="cuda")

        def gain(self, R):
            return 0.0 if R == 0 else R / self.tenth

        def focus(self, R, max_radius):
            """``R``: the radius the gain is made for (0: gain = 0)"""
            rc = lib.mg_depth_focus(self.depth.data_ptr(), self.colors.data_ptr(), 1, None, None, self.h, self.w, Z_RANGE[0], Z_RANGE[1], 0, self.gain(R),
                                    max_radius, self.focus_at[1], self.focus_at[0], 0.0, self.rgb.data_ptr(), self.valid.data_ptr(), None,
                                    self.count.data_ptr(), self.ws.data_ptr(), self.need, stream())
            L.check(rc, "mg_depth_focus", lib)

    settings = [(R, R) for R in RADII] + [(0, RADII[-1])]
    # the call against the restatement, at a size the restatement can afford
    small = Scene(args.check, args.check)
    for R, max_radius in settings:
        small.focus(R, max_radius)
        want = focus_reference(small.d_host, small.c_host, z_range=Z_RANGE, space=LENS, gain=small.gain(R), max_radius=max_radius, focus_at=small.focus_at)
        assert small.count.cpu().tolist() == list(want.count) and want.bad is None and (R == 0 or want.count[3] > 10 * want.count[0])
        for got, ref in ((small.rgb, want.rgb), (small.valid, want.valid)):
            assert np.array_equal(got.cpu().numpy(), ref)

    big = Scene(*SIZE)
    h, w, n = big.h, big.w, big.n
    K = _camera(h, w)
    pose = IDENTITY.copy()
    pose[0, 3] = BASELINE / 2.0
    pose = np.ascontiguousarray(pose)
    need_view = lib.mg_depth_view_workspace_bytes(n)
    ws_view = torch.empty(need_view, dtype=torch.uint8, device="cuda")
    rgb_view = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    out_view = torch.empty((h, w), dtype=torch.float32, device="cuda")
    valid_view = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    count_view = torch.empty(8, dtype=torch.int64, device="cuda")

    def view_call():
        rc = lib.mg_depth_view(big.depth.data_ptr(), big.colors.data_ptr(), 1, None, None, h, w, *K, Z_RANGE[0], Z_RANGE[1], EDGE, pose.ctypes.data, *K,
                               h, w, Z_NEAR, FILL, rgb_view.data_ptr(), out_view.data_ptr(), valid_view.data_ptr(), None, count_view.data_ptr(),
                               ws_view.data_ptr(), need_view, stream())
        L.check(rc, "mg_depth_view", lib)

    counts = {}
    for R, max_radius in settings:
        big.focus(R, max_radius)
        counts[(R, max_radius)] = big.count.cpu().tolist()
    view_call()
    torch.cuda.synchronize()

    labels = [f"mg_depth_focus max_radius {m:2d}, gain {big.gain(R):8.2f}" for R, m in settings] + ["mg_depth_view, for scale             "]
    calls = [(lambda R=R, m=m: big.focus(R, m)) for R, m in settings] + [view_call]
    times = {label: [] for label in labels}
    for r in range(args.rounds + WARM):
        for label, fn in zip(labels, calls):
            ev[0].record()
            for _ in range(args.calls):
                fn()
            ev[1].record()
            ev[1].synchronize()
            if r >= WARM:
                times[label].append(ev[0].elapsed_time(ev[1]) / args.calls)
    lines = [f"calibration of this box: shader clock {mhz.value:.0f} MHz under matrix load (mg_clock_probe), {tflops.value:.0f} TFLOP/s bf16 MFMA "
             f"chain; device-to-device copy of 256 MiB {gbs:.0f} GB/s (read + write); torch {torch.__version__}",
             f"{args.rounds} alternating rounds after {WARM} warm-up rounds; {args.calls} device calls back to back per round; ms, median (min - max)",
             f"{h} x {w}, lens space, the focus on pixel {big.focus_at}; every setting at {args.check} x {args.check} equals the numpy restatement "
             "byte for byte"]
    for (R, m), label in zip(settings, labels):
        c = counts[(R, m)]
        med = statistics.median(times[label])
        tests = c[0] * (2 * m + 1) ** 2
        lines.append(f"  {label}  {_stat(times[label])}   usable {c[0]}, sharp {c[1]}, capped {c[2]} ({100.0 * c[2] / c[0]:.1f} %), contributions {c[3]}, "
                     f"{tests / (med * 1e-3) / 1e9:.1f} G tap tests/s of the full window")
    lines.append(f"  {labels[-1]}  {_stat(times[labels[-1]])}")
    text = "\n".join(lines)
    print(text)
    with open(args.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
