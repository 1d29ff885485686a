"""Depth to mesh on the device: a depth map as a triangle mesh - ``mg_depth_mesh`` (csrc/mesh.hip; the definitions - cell,
candidate, face, vertex - are in include/marigold_hip.h, beside those of the point clouds).  ``depth_to_mesh`` compacts vertices and
faces into a ``Mesh`` without the host learning how many there are: the records and the four counts stay on the device until
``to_host()`` / ``write_ply()`` asks for them.  Everything takes CUDA tensors and runs on the current stream.  The camera is the point
clouds': a pinhole, x right, y down, z forward; every face is ordered so that it looks at the camera."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L, ops as O
from . import points as P

_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])   # (packed: 13 bytes per face)


def write_mesh_ply(path, xyz, faces, normals=None, rgb=None):
    """Binary little-endian PLY: the vertex element of ``write_ply``, then ``element face`` with ``property list uchar int
    vertex_indices`` - a count byte of 3 and three int32 per face."""
    head, rec = P._ply_vertices(xyz, normals, rgb)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    tri = np.empty(len(faces), _FACE_DTYPE)
    tri["n"], tri["v"] = 3, faces
    head += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(tri.tobytes())


def read_mesh_ply(path):
    """A PLY that ``write_mesh_ply`` (or examples/host_mesh.cpp) wrote -> ``HostMesh`` (``index`` None, the totals = what the file
    holds)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_mesh_ply: {path} has no PLY header")
    lines = data[:end].decode("ascii").split("\n")
    if (len(lines) < 7 or lines[1] != "format binary_little_endian 1.0" or not lines[2].startswith("element vertex ")
            or not lines[-3].startswith("element face ") or lines[-2] != "property list uchar int vertex_indices" or lines[-1] != ""):
        raise ValueError(f"read_mesh_ply: {path}: only the binary little-endian mesh files of write_mesh_ply are understood")
    count, total = int(lines[2].split()[2]), int(lines[-3].split()[2])
    names = tuple(ln.split()[2] for ln in lines[3:-3])
    dt = P._ply_dtype("nx" in names, "red" in names)
    if names != dt.names or not all(ln.startswith("property ") for ln in lines[3:-3]):
        raise ValueError(f"read_mesh_ply: {path}: unexpected properties {names}")
    body = data[end + len(b"end_header\n"):]
    if len(body) != count * dt.itemsize + total * _FACE_DTYPE.itemsize:
        raise ValueError(f"read_mesh_ply: {path}: {len(body)} bytes of records, {count} x {dt.itemsize} + {total} x {_FACE_DTYPE.itemsize} "
                         "expected")
    rec = np.frombuffer(body, dt, count)
    tri = np.frombuffer(body, _FACE_DTYPE, total, count * dt.itemsize)
    if total and not (tri["n"] == 3).all():
        raise ValueError(f"read_mesh_ply: {path}: a face that is no triangle")
    cols = lambda *k: np.stack([rec[n] for n in k], axis=1)   # noqa: E731
    return HostMesh(cols("x", "y", "z"), cols("red", "green", "blue") if "red" in names else None,
                    cols("nx", "ny", "nz") if "nx" in names else None, None, np.ascontiguousarray(tri["v"]).reshape(-1, 3), count, count, total,
                    total)


class HostMesh(namedtuple("HostMesh", "xyz rgb normals index faces vertices vertices_written faces_total faces_written")):
    """A mesh on the host: numpy arrays cut to what was written (``rgb``, ``normals``, ``index``: None where absent; ``faces`` int32
    [faces_written, 3], ranks into the vertex arrays).  ``vertices`` and ``faces_total``: how many the map has, which exceed the written
    counts when a capacity was smaller; with cut vertices no face is written."""
    __slots__ = ()

    def write_ply(self, path):
        write_mesh_ply(path, self.xyz, self.faces, self.normals, self.rgb)


class Mesh:
    """The mesh on the device: ``xyz`` fp32 [capacity, 3], ``rgb`` uint8 [capacity, 3] | None, ``normals`` fp32 [capacity, 3] | None,
    ``index`` int32 [capacity] | None (the source pixel's row-major index), ``faces`` int32 [face_capacity, 3], ``count`` int64 [4]:
    the vertices, the vertex records written, the faces, the faces written.  Rows at and past the written counts are uninitialised
    memory.  Nothing here has been read back."""

    def __init__(self, xyz, rgb, normals, index, faces, count):
        self.xyz, self.rgb, self.normals, self.index, self.faces, self.count = xyz, rgb, normals, index, faces, count

    def to_host(self):
        """The one read-back -> ``HostMesh``, every array cut to what was written."""
        v, vw, f, fw = (int(c) for c in self.count.cpu())
        cut = lambda t, k: None if t is None else t[:k].cpu().numpy()   # noqa: E731
        return HostMesh(cut(self.xyz, vw), cut(self.rgb, vw), cut(self.normals, vw), cut(self.index, vw), cut(self.faces, fw), v, vw, f, fw)

    def write_ply(self, path):
        self.to_host().write_ply(path)


def depth_to_mesh(depth, K, *, colors=None, mask=None, coef=None, z_range=(0.0, math.inf), edge_rel=0.0, normals=False, frame="camera",
                  index=False, capacity=None, face_capacity=None, lib=None):
    """A depth map as a triangle mesh -> ``Mesh``: vertices in row-major pixel order, faces in row-major cell order, everything on the
    device and nothing read back.  ``depth``, ``K``, ``colors``, ``mask``, ``coef``, ``z_range``, ``frame``, ``index``: as in
    ``depth_to_points``.  Every 2 x 2 cell of usable pixels is split along the diagonal with the smaller depth difference; a cell with
    three usable corners gives one triangle; with ``edge_rel`` > 0 a triangle is dropped when two of its corners' depths differ by
    more than that fraction of the nearer one, so the surface stops at depth edges.  A usable pixel no triangle names is no vertex.
    ``normals=True`` adds every vertex's normal in ``frame`` ((0, 0, 0) where it has none).  ``capacity`` / ``face_capacity``: the
    records the outputs hold, default h * w and 2 (h - 1) (w - 1); with fewer faces than the map has, the first are written; with
    fewer vertices, the first vertices and no face.  ``count`` tells all four numbers."""
    who = "depth_to_mesh"
    depth, h, w, K, coef, mask, z_min, z_max, edge_rel, word = P._common(who, depth, K, coef, mask, z_range, edge_rel, frame)
    n = h * w
    hwc = 0
    if colors is not None:
        if not (isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 and colors.device == depth.device
                and tuple(colors.shape) in ((h, w, 3), (3, h, w))):
            raise ValueError(f"{who}: colors must be a uint8 tensor [{h}, {w}, 3] or [3, {h}, {w}] on the map's device")
        hwc = int(tuple(colors.shape) == (h, w, 3))
        colors = colors.contiguous()
    capacity = n if capacity is None else capacity
    face_capacity = max(1, 2 * (h - 1) * (w - 1)) if face_capacity is None else face_capacity
    for name, v in (("capacity", capacity), ("face_capacity", face_capacity)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{who}: {name} must be an integer >= 1 (got {v!r})")
    lib = lib if lib is not None else L.init(depth.device.index or 0)
    dev = depth.device
    with torch.cuda.device(dev):
        need = lib.mg_depth_mesh_workspace_bytes(n)
        if need < 0:
            L.check(1, "mg_depth_mesh_workspace_bytes", lib)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        xyz = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((capacity, 3), dtype=torch.uint8, device=dev) if colors is not None else None
        nrm = torch.empty((capacity, 3), dtype=torch.float32, device=dev) if normals else None
        idx = torch.empty((capacity,), dtype=torch.int32, device=dev) if index else None
        faces = torch.empty((face_capacity, 3), dtype=torch.int32, device=dev)
        count = torch.empty(4, dtype=torch.int64, device=dev)
        L.check(lib.mg_depth_mesh(depth.data_ptr(), P._ptr(colors), hwc, P._ptr(mask), P._ptr(coef), h, w, K.fx, K.fy, K.cx, K.cy, z_min, z_max,
                                  edge_rel, word, capacity, face_capacity, xyz.data_ptr(), P._ptr(rgb), P._ptr(nrm), P._ptr(idx), faces.data_ptr(),
                                  count.data_ptr(), ws.data_ptr(), need, O.current_stream_handle()), "mg_depth_mesh", lib)
    return Mesh(xyz, rgb, nrm, idx, faces, count)
