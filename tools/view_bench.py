#!/usr/bin/env python
"""What depth to views costs at 768 x 768 with edge_rel = 0.05: a stereo pair with fill on the scene of
tests/test_gpu_mesh.py (a smooth surface with two steps, non-finite and out-of-range values planted) and its colours, already on the
device, the target as large as the map.  Alternating rounds, ms, median with min - max:
* ``mg_depth_view``   the device call with its outputs allocated once, ``--calls`` of them queued back to back between two device
                      events - the left eye and the right eye in turn - per call; nothing read back
* ``mg_depth_mesh``   the mesh of the same map (6i), the same way, in the same session: what building the triangles costs where they are
                      written out and not drawn
and a floor: the bytes one call must move - the map and the colours read, the key buffer written, offered and read, the outputs
written - at the copy rate this box shows.  Before anything is timed, both eyes at ``--check`` x ``--check`` are held to the bytes of the
numpy restatement (tests/view_reference.py), a size it can afford.  The first line of the log is the box's calibration
(``mg_clock_probe`` and a device-to-device copy of 256 MiB).  Needs an MI355X.
Not measured: other sizes, zoomed targets, other poses, examples/host_view.cpp as a process; the checkpoints of this project are
synthetic, so nothing here says anything about the quality of a view.

    python tools/view_bench.py [--rounds 20] [--calls 20] [--log profiles/view_768.log]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 2
SIZE, EDGE, BASELINE, FILL, Z_NEAR = (768, 768), 0.05, 0.24, 8, 1e-6


def _stat(v):
    return f"{statistics.median(v):9.4f}  ({min(v):.4f} - {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--check", type=int, default=192)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "view_768.log"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from marigold_amd import _lib as L
    from tests.test_gpu_mesh import Z_RANGE, _camera, _mesh_scene
    from tests.view_reference import IDENTITY, view_reference
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
    poses = []
    for tx in (BASELINE / 2.0, -BASELINE / 2.0):
        m = IDENTITY.copy()
        m[0, 3] = tx
        poses.append(np.ascontiguousarray(m))

    class Scene:
        def __init__(self, h, w):
            self.h, self.w, self.n = h, w, h * w
            self.d_host, self.c_host = _mesh_scene(h, w, None)
            self.K = _camera(h, w)
            self.depth, self.colors = torch.from_numpy(self.d_host).cuda(), torch.from_numpy(self.c_host).cuda()
            self.need = lib.mg_depth_view_workspace_bytes(self.n)
            self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")
            self.rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
            self.out = torch.empty((h, w), dtype=torch.float32, device="cuda")
            self.valid = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            self.count = torch.empty(8, dtype=torch.int64, device="cuda")

        def view(self, eye):
            rc = lib.mg_depth_view(self.depth.data_ptr(), self.colors.data_ptr(), 1, None, None, self.h, self.w, *self.K, Z_RANGE[0], Z_RANGE[1], EDGE,
                                   poses[eye].ctypes.data, *self.K, self.h, self.w, Z_NEAR, FILL, self.rgb.data_ptr(), self.out.data_ptr(),
                                   self.valid.data_ptr(), None, self.count.data_ptr(), self.ws.data_ptr(), self.need, stream())
            L.check(rc, "mg_depth_view", lib)

    # the call against the restatement, at a size the restatement can afford
    small = Scene(args.check, args.check)
    for eye in range(2):
        small.view(eye)
        want = view_reference(small.d_host, small.K, small.c_host, z_range=Z_RANGE, edge_rel=EDGE, pose=poses[eye], z_near=Z_NEAR, fill_radius=FILL)
        assert small.count.cpu().tolist() == list(want.count) and want.count[5] == 0 and want.count[7] > 0
        for got, ref in ((small.rgb, want.rgb), (small.out, want.depth), (small.valid, want.valid)):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))

    big = Scene(*SIZE)
    h, w, n = big.h, big.w, big.n
    cap_f = 2 * (h - 1) * (w - 1)
    need_mesh = lib.mg_depth_mesh_workspace_bytes(n)
    ws_mesh = torch.empty(need_mesh, dtype=torch.uint8, device="cuda")
    xyz = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    rgb_v = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    faces = torch.empty((cap_f, 3), dtype=torch.int32, device="cuda")
    count_mesh = torch.empty(4, dtype=torch.int64, device="cuda")

    def mesh_call():
        rc = lib.mg_depth_mesh(big.depth.data_ptr(), big.colors.data_ptr(), 1, None, None, h, w, *big.K, Z_RANGE[0], Z_RANGE[1], EDGE, 0, n, cap_f,
                               xyz.data_ptr(), rgb_v.data_ptr(), None, None, faces.data_ptr(), count_mesh.data_ptr(), ws_mesh.data_ptr(), need_mesh,
                               stream())
        L.check(rc, "mg_depth_mesh", lib)

    counts = []
    for eye in range(2):
        big.view(eye)
        counts.append(big.count.cpu().tolist())
    mesh_call()
    assert counts[0][0] == counts[1][0] == int(count_mesh.cpu()[2])   # the faces that are drawn are the mesh's

    times = {"mg_depth_view (events, per call)": [], "mg_depth_mesh (events, per call)": []}
    for r in range(args.rounds + WARM):
        got = []
        for fn in (lambda k: big.view(k % 2), lambda k: mesh_call()):
            ev[0].record()
            for k in range(args.calls):
                fn(k)
            ev[1].record()
            ev[1].synchronize()
            got.append(ev[0].elapsed_time(ev[1]) / args.calls)
        if r >= WARM:
            for label, v in zip(times, got):
                times[label].append(v)
    covered = max(c[6] for c in counts)
    # the map and the colours read; the key buffer cleared, one 8-byte offer per covered pixel at the least, read by the resolve; rgb,
    # depth and valid written
    floor = 4 * n + 3 * n + 8 * n + 8 * covered + 8 * n + 8 * n
    t_floor = floor / (gbs * 1e9) * 1e3
    med = statistics.median(times["mg_depth_view (events, per call)"])
    lines = [f"calibration of this box: shader clock {mhz.value:.0f} MHz under matrix load (mg_clock_probe), {tflops.value:.0f} TFLOP/s bf16 MFMA "
             f"chain; device-to-device copy of 256 MiB {gbs:.0f} GB/s (read + write); torch {torch.__version__}",
             f"{args.rounds} alternating rounds after {WARM} warm-up rounds; {args.calls} device calls back to back per round; ms, median (min - max)",
             f"{h} x {w} -> {h} x {w}, edge_rel = {EDGE}, a stereo pair of baseline {BASELINE} with fill_radius = {FILL}, the eyes in turn; "
             f"both eyes at {args.check} x {args.check} equal the numpy restatement byte for byte"]
    lines += [f"  {side} eye: " + ", ".join(f"{k} {v}" for k, v in zip(("faces", "drawn", "near", "off", "back", "span", "covered", "filled"), c))
              for side, c in zip(("left", "right"), counts)]
    lines += [f"  {label}  {_stat(v)}" for label, v in times.items()]
    lines.append(f"  the bytes one view must move: {floor / 1e6:.1f} MB, {t_floor:.4f} ms at the copy rate; the call's median is {med / t_floor:.1f} times that")
    text = "\n".join(lines)
    print(text)
    with open(args.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
