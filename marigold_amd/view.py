"""Depth to views on the device: the picture seen from a moved camera - ``mg_depth_view`` (csrc/view.hip; the definitions -
target camera, transform, dropped faces, coverage, key, colour, fill - are in include/marigold_hip.h, beside those of the meshes it
draws).  ``render_view`` gives a ``View`` of device tensors without a read-back; ``stereo_pair`` gives the two eyes of a stereo
picture.  Everything takes CUDA tensors and runs on the current stream.  The cameras are the point clouds': pinholes, x right, y down,
z forward; ``pose`` maps a point of the source camera's frame into the target camera's, X' = R X + t."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L, ops as O
from . import points as P

COUNT_NAMES = ("faces", "drawn", "near", "off", "back", "span", "covered", "filled")


def write_ppm(path, rgb):
    """uint8 [h, w, 3] -> a binary PPM (P6)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"write_ppm: a uint8 picture [h, w, 3] is expected (got {rgb.shape})")
    with open(path, "wb") as f:
        f.write(f"P6\n{rgb.shape[1]} {rgb.shape[0]}\n255\n".encode("ascii"))
        f.write(rgb.tobytes())


class HostView(namedtuple("HostView", "rgb depth valid face count")):
    """A view on the host: ``rgb`` uint8 [h2, w2, 3], ``depth`` fp32 [h2, w2], ``valid`` uint8 [h2, w2] (1: a face covers the pixel,
    2: filled, 0: neither), ``face`` int32 [h2, w2] | None, ``count``: a dict of the eight counts (``COUNT_NAMES``)."""
    __slots__ = ()

    def write_ppm(self, path):
        write_ppm(path, self.rgb)


class View(namedtuple("View", "rgb depth valid face count")):
    """The view on the device: ``rgb`` uint8 in the layout of the colours it was drawn from ([h2, w2, 3] or [3, h2, w2]), ``depth`` fp32
    [h2, w2], ``valid`` uint8 [h2, w2], ``face`` int32 [h2, w2] | None (the winning face id, -1 where no face covers the pixel),
    ``count`` int64 [8]: faces, drawn, near, off, back, span, pixels covered, pixels filled.  Nothing here has been read back."""
    __slots__ = ()

    def to_host(self):
        """The one read-back -> ``HostView``, the picture as [h2, w2, 3]."""
        h2, w2 = self.depth.shape
        rgb = self.rgb if tuple(self.rgb.shape) == (h2, w2, 3) else self.rgb.permute(1, 2, 0)
        count = dict(zip(COUNT_NAMES, (int(c) for c in self.count.cpu())))
        return HostView(rgb.contiguous().cpu().numpy(), self.depth.cpu().numpy(), self.valid.cpu().numpy(),
                        None if self.face is None else self.face.cpu().numpy(), count)

    def write_ppm(self, path):
        self.to_host().write_ppm(path)


def _pose(who, pose):
    """``(R, t)`` or a 3 x 4 array -> the 12 doubles of [R | t], rows first, or None for the identity"""
    if pose is None:
        return None
    try:
        if isinstance(pose, (tuple, list)) and len(pose) == 2:
            R, t = np.asarray(pose[0], np.float64).reshape(3, 3), np.asarray(pose[1], np.float64).reshape(3, 1)
            m = np.hstack([R, t])
        else:
            m = np.asarray(pose.cpu() if isinstance(pose, torch.Tensor) else pose, np.float64).reshape(3, 4)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: pose must be (R [3, 3], t [3]) or a 3 x 4 array") from None
    if not np.isfinite(m).all():
        raise ValueError(f"{who}: pose must be finite")
    return np.ascontiguousarray(m)


def render_view(depth, K, colors, *, pose=None, K_out=None, size=None, coef=None, mask=None, z_range=(0.0, math.inf), edge_rel=0.05,
                z_near=1e-6, fill_radius=0, faces=False, lib=None):
    """The picture ``colors`` over the surface of ``depth``, seen from a second pinhole camera -> ``View``, everything on the device and
    nothing read back.  ``depth``, ``K``, ``coef``, ``mask``, ``z_range``, ``edge_rel``: as in ``depth_to_mesh``, whose faces are what
    is drawn; ``colors``: uint8 [h, w, 3] or [3, h, w] on the map's device.  ``pose``: ``(R, t)`` or a 3 x 4 array, the source
    camera's frame into the target's (default: the identity); ``K_out``: the target camera (default ``K``); ``size``: the target's
    (h2, w2) (default the map's).  A face with a corner nearer than ``z_near`` in the target camera, one that leaves the snapping
    range, one seen from behind and one that spans more than 64 target pixels is not drawn; ``count`` tells how many of each.
    ``fill_radius`` r > 0 fills a pixel no face covers from the nearest covered pixels of its row within r, the farther one of the
    two: the background shows through a disocclusion.  ``faces=True`` adds the map of winning face ids."""
    who = "render_view"
    depth, h, w, K, coef, mask, z_min, z_max, edge_rel, _ = P._common(who, depth, K, coef, mask, z_range, edge_rel, "camera")
    if not (isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 and colors.device == depth.device
            and tuple(colors.shape) in ((h, w, 3), (3, h, w))):
        raise ValueError(f"{who}: colors must be a uint8 tensor [{h}, {w}, 3] or [3, {h}, {w}] on the map's device")
    hwc = int(tuple(colors.shape) == (h, w, 3))
    colors = colors.contiguous()
    if K_out is None:
        K_out = K
    else:
        try:
            K_out = P.Intrinsics(*(P._number(who, "the target camera", v) for v in K_out))
        except (TypeError, ValueError):
            raise ValueError(f"{who}: K_out must be Intrinsics(fx, fy, cx, cy) (got {K_out!r})") from None
        if not (all(math.isfinite(v) for v in K_out) and K_out.fx > 0.0 and K_out.fy > 0.0):
            raise ValueError(f"{who}: the target camera needs finite values and focal lengths > 0 (got {K_out!r})")
    h2, w2 = (h, w) if size is None else tuple(size)
    for v in (h2, w2):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{who}: size must be (h2, w2), integers >= 1 (got {size!r})")
    z_near = P._number(who, "z_near", z_near)
    if not (math.isfinite(z_near) and z_near > 0.0):
        raise ValueError(f"{who}: z_near must be finite and > 0 (got {z_near!r})")
    if isinstance(fill_radius, bool) or not isinstance(fill_radius, int) or not 0 <= fill_radius <= L.VIEW_MAX_FILL:
        raise ValueError(f"{who}: fill_radius must be an integer from 0 to {L.VIEW_MAX_FILL} (got {fill_radius!r})")
    pose = _pose(who, pose)
    lib = lib if lib is not None else L.init(depth.device.index or 0)
    dev = depth.device
    with torch.cuda.device(dev):
        need = lib.mg_depth_view_workspace_bytes(h2 * w2)
        if need < 0:
            L.check(1, "mg_depth_view_workspace_bytes", lib)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rgb = torch.empty((h2, w2, 3) if hwc else (3, h2, w2), dtype=torch.uint8, device=dev)
        out = torch.empty((h2, w2), dtype=torch.float32, device=dev)
        valid = torch.empty((h2, w2), dtype=torch.uint8, device=dev)
        face = torch.empty((h2, w2), dtype=torch.int32, device=dev) if faces else None
        count = torch.empty(8, dtype=torch.int64, device=dev)
        L.check(lib.mg_depth_view(depth.data_ptr(), colors.data_ptr(), hwc, P._ptr(mask), P._ptr(coef), h, w, K.fx, K.fy, K.cx, K.cy, z_min, z_max,
                                  edge_rel, None if pose is None else pose.ctypes.data, K_out.fx, K_out.fy, K_out.cx, K_out.cy, h2, w2, z_near,
                                  fill_radius, rgb.data_ptr(), out.data_ptr(), valid.data_ptr(), P._ptr(face), count.data_ptr(), ws.data_ptr(),
                                  need, O.current_stream_handle()), "mg_depth_view", lib)
    return View(rgb, out, valid, face, count)


def stereo_pair(depth, K, colors, baseline, **kw):
    """The two eyes of a stereo picture -> ``(left, right)``, two ``View``: cameras at x = -baseline / 2 and x = +baseline / 2 of the
    source camera, looking the same way, so their poses are t = (+baseline / 2, 0, 0) and t = (-baseline / 2, 0, 0).  ``baseline`` is
    in the units of the distances (``coef``); the other arguments are ``render_view``'s."""
    baseline = P._number("stereo_pair", "baseline", baseline)
    if not math.isfinite(baseline):
        raise ValueError(f"stereo_pair: baseline must be finite (got {baseline!r})")
    if "pose" in kw:
        raise ValueError("stereo_pair: the poses are the pair's own; use render_view for another")
    eye = lambda tx: (np.eye(3), (tx, 0.0, 0.0))   # noqa: E731
    return render_view(depth, K, colors, pose=eye(baseline / 2.0), **kw), render_view(depth, K, colors, pose=eye(-baseline / 2.0), **kw)
