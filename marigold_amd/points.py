"""Depth to 3D on the device: camera-space points and surface normals from a depth map - ``mg_depth_points`` /
``mg_depth_normals`` (csrc/points.hip; the definitions - usable, joined, kept, point, normal - are in include/marigold_hip.h).
``depth_to_points`` compacts the kept pixels into a ``PointCloud`` in row-major order without the host learning how many there are:
the records, and their count, stay on the device until ``to_host()`` / ``write_ply()`` asks for them.  ``depth_to_normals`` is the dense
map, in the layout ``score_normals`` takes.  Everything takes CUDA tensors and runs on the current stream; nothing but ``to_host`` reads
back or synchronises.  The camera is a pinhole: x right, y down, z forward, integer coordinates at pixel centres."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L, ops as O

Intrinsics = namedtuple("Intrinsics", "fx fy cx cy")   # in pixels of the map's own grid
FRAMES = tuple(L.NORMALS_FRAME)


def intrinsics_from_fov(h, w, fov_x_deg):
    """A pinhole with square pixels from the horizontal field of view in degrees: the principal point at the picture's centre,
    ``((w - 1) / 2, (h - 1) / 2)``, the focal length ``(w / 2) / tan(fov / 2)``."""
    fov = float(fov_x_deg)
    if not (int(h) >= 1 and int(w) >= 1 and 0.0 < fov < 180.0):
        raise ValueError(f"intrinsics_from_fov: a size of {h} x {w} and a field of view of {fov_x_deg!r} degrees; sizes >= 1 and an angle "
                         "inside (0, 180) are expected")
    f = (w / 2.0) / math.tan(math.radians(fov) / 2.0)
    return Intrinsics(f, f, (w - 1) / 2.0, (h - 1) / 2.0)


def scale_intrinsics(K, from_hw, to_hw):
    """``K`` of a picture of ``from_hw`` = (h0, w0) for the same picture resampled to ``to_hw`` = (h1, w1), under the pixel-centre
    rule: the focal lengths scale, ``cx' = (cx + 0.5) * w1 / w0 - 0.5`` and ``cy`` likewise."""
    K = Intrinsics(*(float(v) for v in K))
    (h0, w0), (h1, w1) = from_hw, to_hw
    if min(h0, w0, h1, w1) < 1:
        raise ValueError(f"scale_intrinsics: sizes must be >= 1 (got {from_hw!r} -> {to_hw!r})")
    return Intrinsics(K.fx * w1 / w0, K.fy * h1 / h0, (K.cx + 0.5) * w1 / w0 - 0.5, (K.cy + 0.5) * h1 / h0 - 0.5)


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------

def _ply_dtype(normals, colours):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colours:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields)   # (packed: 12, 15, 24 or 27 bytes per record)


def _ply_vertices(xyz, normals, rgb):
    """-> (the header up to the vertex properties, as lines; the packed vertex records) - what ``write_ply`` and ``write_mesh_ply`` share"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    dt = _ply_dtype(normals is not None, rgb is not None)
    rec = np.empty(len(xyz), dt)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(len(xyz), 3)
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8).reshape(len(xyz), 3)
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}"]
    head += [f"property {'uchar' if dt[name] == np.uint8 else 'float'} {name}" for name in dt.names]
    return head, rec


def write_ply(path, xyz, normals=None, rgb=None):
    """Binary little-endian PLY: ``x y z`` float, then ``nx ny nz`` float when given, then ``red green blue`` uchar when given."""
    head, rec = _ply_vertices(xyz, normals, rgb)
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """A PLY that ``write_ply`` (or examples/host_points.cpp) wrote -> ``HostPointCloud`` (``index`` None, ``kept`` = the records)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_ply: {path} has no PLY header")
    lines = data[:end].decode("ascii").split("\n")
    if lines[1] != "format binary_little_endian 1.0" or not lines[2].startswith("element vertex "):
        raise ValueError(f"read_ply: {path}: only the binary little-endian vertex files of write_ply are understood")
    count = int(lines[2].split()[2])
    names = tuple(ln.split()[2] for ln in lines[3:] if ln.startswith("property "))
    dt = _ply_dtype("nx" in names, "red" in names)
    if names != dt.names:
        raise ValueError(f"read_ply: {path}: unexpected properties {names}")
    body = data[end + len(b"end_header\n"):]
    if len(body) != count * dt.itemsize:
        raise ValueError(f"read_ply: {path}: {len(body)} bytes of records, {count} x {dt.itemsize} expected")
    rec = np.frombuffer(body, dt)
    cols = lambda *k: np.stack([rec[n] for n in k], axis=1)   # noqa: E731
    return HostPointCloud(cols("x", "y", "z"), cols("red", "green", "blue") if "red" in names else None,
                          cols("nx", "ny", "nz") if "nx" in names else None, None, count, count)


class HostPointCloud(namedtuple("HostPointCloud", "xyz rgb normals index kept written")):
    """A cloud on the host: numpy arrays cut to the ``written`` records (``rgb``, ``normals``, ``index``: None where absent);
    ``kept``: how many pixels were kept, which exceeds ``written`` when the capacity was smaller."""
    __slots__ = ()

    def write_ply(self, path):
        write_ply(path, self.xyz, self.normals, self.rgb)


class PointCloud:
    """The cloud on the device: ``xyz`` fp32 [capacity, 3], ``rgb`` uint8 [capacity, 3] | None, ``normals`` fp32 [capacity, 3] | None,
    ``index`` int32 [capacity] | None (the source pixel's row-major index), ``count`` int64 [2]: the kept pixels and the records
    written = min(kept, capacity).  Rows at and past ``count[1]`` are uninitialised memory.  Nothing here has been read back."""

    def __init__(self, xyz, rgb, normals, index, count):
        self.xyz, self.rgb, self.normals, self.index, self.count = xyz, rgb, normals, index, count

    def to_host(self):
        """The one read-back -> ``HostPointCloud``, every array cut to the records written."""
        kept, written = (int(v) for v in self.count.cpu())
        cut = lambda t: None if t is None else t[:written].cpu().numpy()   # noqa: E731
        return HostPointCloud(cut(self.xyz), cut(self.rgb), cut(self.normals), cut(self.index), kept, written)

    def write_ply(self, path):
        self.to_host().write_ply(path)


# ---- the device calls --------------------------------------------------------------------------------------------------------------

def _number(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"{who}: {name} must be a number (got {v!r})")
    return float(v)


def _common(who, depth, K, coef, mask, z_range, edge_rel, frame):
    """The arguments both calls share, checked -> (depth [h, w] contiguous, h, w, K, coef tensor | None, mask | None, z_min, z_max,
    edge_rel, frame word)."""
    if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32 and depth.dim() >= 2 and depth.numel() >= 1
            and depth.numel() == depth.shape[-2] * depth.shape[-1]):
        raise ValueError(f"{who}: depth must be a non-empty fp32 CUDA tensor [h, w] (leading axes of length 1 are allowed)")
    h, w = (int(v) for v in depth.shape[-2:])
    depth = depth.reshape(h, w).contiguous()
    try:
        K = Intrinsics(*(_number(who, "the camera", v) for v in K))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: K must be Intrinsics(fx, fy, cx, cy) (got {K!r})") from None
    if not (all(math.isfinite(v) for v in K) and K.fx > 0.0 and K.fy > 0.0):
        raise ValueError(f"{who}: the camera needs finite values and focal lengths > 0 (got {K!r})")
    if coef is not None:
        if isinstance(coef, torch.Tensor):
            if not (coef.dtype == torch.float64 and coef.numel() == 2 and coef.device == depth.device and coef.is_contiguous()):
                raise ValueError(f"{who}: coef must be a contiguous fp64 [2] tensor on the map's device, or a pair of numbers")
        else:
            try:
                s, t = (_number(who, "coef", v) for v in coef)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: coef must be a contiguous fp64 [2] tensor on the map's device, or a pair of numbers") from None
            coef = torch.tensor([s, t], dtype=torch.float64, device=depth.device)
    if mask is not None:
        if not (isinstance(mask, torch.Tensor) and mask.dtype in (torch.bool, torch.uint8) and mask.numel() == h * w
                and tuple(mask.shape[-2:]) == (h, w) and mask.device == depth.device):
            raise ValueError(f"{who}: mask must be a bool or uint8 tensor of the map's shape on its device")
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    try:
        z_min, z_max = (_number(who, "z_range", v) for v in z_range)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: z_range must be a pair (z_min, z_max) (got {z_range!r})") from None
    if not (math.isfinite(z_min) and z_min >= 0.0 and z_max > z_min):
        raise ValueError(f"{who}: z_range must be (z_min, z_max) with 0 <= z_min < z_max, z_min finite (got {z_range!r})")
    edge_rel = _number(who, "edge_rel", edge_rel)
    if not (math.isfinite(edge_rel) and edge_rel >= 0.0):
        raise ValueError(f"{who}: edge_rel must be finite and >= 0 (got {edge_rel!r})")
    if frame not in L.NORMALS_FRAME:
        raise ValueError(f'{who}: frame must be "camera" or "marigold" (got {frame!r})')
    return depth, h, w, K, coef, mask, z_min, z_max, edge_rel, L.NORMALS_FRAME[frame]


def _ptr(t):
    return None if t is None else t.data_ptr()


def depth_to_normals(depth, K, *, coef=None, mask=None, z_range=(0.0, math.inf), edge_rel=0.0, frame="marigold", lib=None):
    """The surface normals a depth map implies -> (normals fp32 [3, h, w], valid bool [h, w]), device tensors.  ``depth``: fp32 CUDA
    [h, w]; ``K``: its ``Intrinsics``; ``coef``: None, or (s, t) - a device fp64 [2] tensor such as ``align_depth`` returns, or two
    numbers - for z = s * depth + t; ``mask``: bool / uint8, True where a pixel may count; ``z_range`` = (z_min, z_max): a pixel
    counts when z_min < z <= z_max; ``edge_rel``: neighbours whose depths differ by more than this fraction of the nearer one are not
    joined, and a pixel with such a neighbour gets no normal (0: no rule).  ``frame``: "marigold" - x right, y up, z toward the viewer,
    how this model family's normal maps are published and what ``score_normals`` takes - or "camera" - x right, y down, z forward.
    A pixel without a normal holds zeros and is False in ``valid``."""
    who = "depth_to_normals"
    depth, h, w, K, coef, mask, z_min, z_max, edge_rel, word = _common(who, depth, K, coef, mask, z_range, edge_rel, frame)
    lib = lib if lib is not None else L.init(depth.device.index or 0)
    with torch.cuda.device(depth.device):
        out = torch.empty((3, h, w), dtype=torch.float32, device=depth.device)
        valid = torch.empty((h, w), dtype=torch.uint8, device=depth.device)
        L.check(lib.mg_depth_normals(depth.data_ptr(), _ptr(mask), _ptr(coef), h, w, K.fx, K.fy, K.cx, K.cy, z_min, z_max, edge_rel, word,
                                     out.data_ptr(), valid.data_ptr(), O.current_stream_handle()), "mg_depth_normals", lib)
    return out, valid.view(torch.bool)


def depth_to_points(depth, K, *, colors=None, mask=None, coef=None, z_range=(0.0, math.inf), edge_rel=0.0, normals=False, frame="camera",
                    index=False, capacity=None, lib=None):
    """The kept pixels of a depth map as camera-space points -> ``PointCloud``, records in row-major pixel order, everything on the
    device and nothing read back.  ``depth``, ``K``, ``coef``, ``mask``, ``z_range``, ``edge_rel``: as in ``depth_to_normals``; with
    ``edge_rel`` > 0 a pixel is dropped when a usable neighbour's depth differs by more than that fraction of the nearer one - the
    flying pixels of a depth edge.  ``colors``: the picture at the map's size, uint8 on the map's device, [h, w, 3] or planes
    [3, h, w] ([3, 3, 3] is read as [h, w, 3]).  ``normals=True`` adds the normal of every record in ``frame`` ((0, 0, 0) where a kept
    pixel has none); ``index=True`` the source pixel's row-major index.  ``capacity``: the records the outputs hold, default h * w;
    with fewer than are kept, the first ``capacity`` are written and ``count[0]`` still tells how many were kept."""
    who = "depth_to_points"
    depth, h, w, K, coef, mask, z_min, z_max, edge_rel, word = _common(who, depth, K, coef, mask, z_range, edge_rel, frame)
    n = h * w
    hwc = 0
    if colors is not None:
        if not (isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 and colors.device == depth.device
                and tuple(colors.shape) in ((h, w, 3), (3, h, w))):
            raise ValueError(f"{who}: colors must be a uint8 tensor [{h}, {w}, 3] or [3, {h}, {w}] on the map's device")
        hwc = int(tuple(colors.shape) == (h, w, 3))
        colors = colors.contiguous()
    capacity = n if capacity is None else capacity
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
        raise ValueError(f"{who}: capacity must be an integer >= 1 (got {capacity!r})")
    lib = lib if lib is not None else L.init(depth.device.index or 0)
    dev = depth.device
    with torch.cuda.device(dev):
        need = lib.mg_depth_points_workspace_bytes(n)
        if need < 0:
            L.check(1, "mg_depth_points_workspace_bytes", lib)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        xyz = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((capacity, 3), dtype=torch.uint8, device=dev) if colors is not None else None
        nrm = torch.empty((capacity, 3), dtype=torch.float32, device=dev) if normals else None
        idx = torch.empty((capacity,), dtype=torch.int32, device=dev) if index else None
        count = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(lib.mg_depth_points(depth.data_ptr(), _ptr(colors), hwc, _ptr(mask), _ptr(coef), h, w, K.fx, K.fy, K.cx, K.cy, z_min, z_max,
                                    edge_rel, word, capacity, xyz.data_ptr(), _ptr(rgb), _ptr(nrm), _ptr(idx), count.data_ptr(), ws.data_ptr(),
                                    need, O.current_stream_handle()), "mg_depth_points", lib)
    return PointCloud(xyz, rgb, nrm, idx, count)
