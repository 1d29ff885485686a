#!/usr/bin/env python
"""What depth to mesh costs at 768 x 768 with edge_rel = 0.05, on the scene of tests/test_gpu_mesh.py (a smooth surface
with two steps, non-finite and out-of-range values planted) and its colours, already on the device.  Alternating rounds, ms, median
with min - max:
* ``mg_depth_mesh``          the device call with its outputs allocated once, ``--calls`` of them queued back to back between two
                             device events, per call; nothing read back
* ``torch ops``              the same mesh composed from torch device ops in fp64 - the cells' forms and faces, boolean indexing for
                             the faces, a flag per pixel, a cumulative sum for the ranks, ``nonzero`` and gathers for the records -
                             by the wall clock, the synchronisations that boolean indexing forces included
* ``numpy after read-back``  the depth map copied to the host and the float64 restatement of tests/mesh_reference.py, by the wall clock
Before anything is timed, the torch composition and the restatement are held to the device call's counts, faces, indices and xyz bits.
The first line of the log is the box's calibration (``mg_clock_probe`` and a device-to-device copy of 256 MiB).  Needs an MI355X.
Not measured: other sizes, other edge rules, normals, examples/host_mesh.cpp as a process; the checkpoints of this project are
synthetic, so nothing here says anything about the quality of a mesh.

    python tools/mesh_bench.py [--rounds 20] [--calls 20] [--log profiles/mesh_768.log]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 2
SIZE, EDGE = (768, 768), 0.05


def _stat(v):
    return f"{statistics.median(v):9.4f}  ({min(v):.4f} - {max(v):.4f})"


def _torch_mesh(torch, depth, K, colors, z_range, edge):
    """The same mesh from torch device ops (no normals): what a caller would write without the kernel -> (xyz, rgb, index, faces)."""
    h, w = depth.shape
    dev = depth.device
    z = depth.double()
    usable = torch.isfinite(z) & (z > z_range[0]) & (z <= z_range[1])
    corner = ((slice(0, -1), slice(0, -1)), (slice(0, -1), slice(1, None)), (slice(1, None), slice(0, -1)), (slice(1, None), slice(1, None)))
    u, zc = [usable[c] for c in corner], [z[c] for c in corner]
    n_usable = u[0].int() + u[1].int() + u[2].int() + u[3].int()
    four, three = n_usable == 4, n_usable == 3
    ad = (zc[0] - zc[3]).abs() <= (zc[1] - zc[2]).abs()
    form = torch.full_like(n_usable, -1)
    form[four & ad] = 0
    form[four & ~ad] = 1
    for missing, name in ((3, 2), (0, 3), (1, 4), (2, 5)):
        form[three & ~u[missing]] = name
    acd, adb, acb, bcd = (0, 2, 3), (0, 3, 1), (0, 2, 1), (1, 2, 3)
    table = torch.tensor([(acd, adb), (acb, bcd), (acb, acb), (bcd, bcd), (acd, acd), (adb, adb)], device=dev)
    cand = table[form.clamp(min=0).long()]                                        # [h - 1, w - 1, 2, 3]
    zt = torch.gather(torch.stack(zc, dim=-1)[:, :, None, :].expand(-1, -1, 2, -1), -1, cand)

    def joined(p, q):
        return (p - q).abs() <= edge * torch.minimum(p, q)

    is_face = joined(zt[..., 0], zt[..., 1]) & joined(zt[..., 1], zt[..., 2]) & joined(zt[..., 2], zt[..., 0]) & (form >= 0)[..., None]
    is_face[..., 1] &= four
    pixel = torch.arange(h * w, device=dev).reshape(h, w)
    tri = torch.gather(torch.stack([pixel[c] for c in corner], dim=-1)[:, :, None, :].expand(-1, -1, 2, -1), -1, cand)
    face_pixels = tri[is_face]                                                    # boolean indexing: the host must learn the count
    vertex = torch.zeros(h * w, dtype=torch.bool, device=dev)
    vertex[face_pixels.reshape(-1)] = True
    rank = torch.cumsum(vertex, 0) - 1
    index = torch.nonzero(vertex).reshape(-1)                                     # and once more
    xs = torch.arange(w, device=dev, dtype=torch.float64)[None, :]
    ys = torch.arange(h, device=dev, dtype=torch.float64)[:, None]
    xyz = torch.stack([((xs - K[2]) * z) / K[0], ((ys - K[3]) * z) / K[1], z], dim=-1).float()
    return xyz.reshape(-1, 3)[index], colors.reshape(-1, 3)[index], index.int(), rank[face_pixels].int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mesh_768.log"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from marigold_amd import _lib as L
    from tests.mesh_reference import mesh_reference
    from tests.test_gpu_mesh import Z_RANGE, _camera, _mesh_scene
    lib = L.init(0)
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0, ctypes.byref(mhz), ctypes.byref(tflops)),
            "mg_clock_probe", lib)
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
    h, w = SIZE
    n, cap_f = h * w, 2 * (h - 1) * (w - 1)
    d_host, c_host = _mesh_scene(h, w, None)
    K = _camera(h, w)
    depth, colors = torch.from_numpy(d_host).cuda(), torch.from_numpy(c_host).cuda()
    need = lib.mg_depth_mesh_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    xyz = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    rgb = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    faces = torch.empty((cap_f, 3), dtype=torch.int32, device="cuda")
    count = torch.empty(4, dtype=torch.int64, device="cuda")

    def device_call():
        rc = lib.mg_depth_mesh(depth.data_ptr(), colors.data_ptr(), 1, None, None, h, w, *K, Z_RANGE[0], Z_RANGE[1], EDGE, 0, n, cap_f, xyz.data_ptr(),
                               rgb.data_ptr(), None, idx.data_ptr(), faces.data_ptr(), count.data_ptr(), ws.data_ptr(), need,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "mg_depth_mesh", lib)

    def numpy_after_read_back():
        return mesh_reference(depth.cpu().numpy(), K, colors=colors.cpu().numpy(), z_range=Z_RANGE, edge_rel=EDGE)

    # the three contenders make the same mesh
    device_call()
    V, Vw, F, Fw = (int(v) for v in count.cpu())
    want = numpy_after_read_back()
    assert (V, Vw, F, Fw) == want.count
    t_xyz, t_rgb, t_idx, t_faces = _torch_mesh(torch, depth, K, colors, Z_RANGE, EDGE)
    for got, ref, dev in ((t_xyz, want.xyz, xyz[:V]), (t_rgb, want.rgb, rgb[:V]), (t_idx, want.index, idx[:V]), (t_faces, want.faces, faces[:F])):
        assert np.array_equal(got.cpu().numpy().view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))
        assert np.array_equal(dev.cpu().numpy().view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))

    times = {"mg_depth_mesh (events, per call)": [], "torch ops (wall, with the syncs)": [], "numpy after read-back (wall)   ": []}
    for r in range(args.rounds + WARM):
        ev[0].record()
        for _ in range(args.calls):
            device_call()
        ev[1].record()
        ev[1].synchronize()
        t_dev = ev[0].elapsed_time(ev[1]) / args.calls
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _torch_mesh(torch, depth, K, colors, Z_RANGE, EDGE)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        numpy_after_read_back()
        t2 = time.perf_counter()
        if r >= WARM:
            for label, v in zip(times, (t_dev, (t1 - t0) * 1e3, (t2 - t1) * 1e3)):
                times[label].append(v)
    traffic = 4 * 4 * n + 5 * n + 4 * n + V * (3 + 19) + F * 12 + 4 * 3 * F   # four passes over d; codes and ranks; records; faces and their ranks
    lines = [f"calibration of this box: shader clock {mhz.value:.0f} MHz under matrix load (mg_clock_probe), {tflops.value:.0f} TFLOP/s bf16 MFMA "
             f"chain; device-to-device copy of 256 MiB {gbs:.0f} GB/s (read + write); torch {torch.__version__}",
             f"{args.rounds} alternating rounds after {WARM} warm-up rounds; {args.calls} device calls back to back per round; ms, median (min - max)",
             f"{h} x {w}, edge_rel = {EDGE}: {V} of {n} pixels are vertices, {F} of {cap_f} candidate faces; xyz, colours and indices, no normals"]
    lines += [f"  {label}  {_stat(v)}" for label, v in times.items()]
    lines.append(f"  a rough count of the call's traffic: {traffic / 1e6:.1f} MB, {traffic / (gbs * 1e9) * 1e3:.4f} ms at the copy rate")
    text = "\n".join(lines)
    print(text)
    with open(args.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
