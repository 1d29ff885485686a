"""Depth to focus on the device: the picture refocused from its depth map, a synthetic shallow depth of field -
``mg_depth_focus`` (csrc/focus.hip; the definitions - focus distance, blur radius, order, contribution, weight, result - are in
include/marigold_hip.h, beside those of the depth they read).  ``refocus`` gives a ``Refocus`` of device tensors without a read-back.
Everything takes CUDA tensors and runs on the current stream.  Every byte is a function of the inputs alone: after the blur radius,
which is fp64, all arithmetic is integer."""
import math
from collections import namedtuple

import torch

from . import _lib as L, ops as O
from . import points as P
from .view import write_ppm

COUNT_NAMES = ("usable", "sharp", "capped", "contributions", "bad_focus")
SPACES = tuple(L.FOCUS_SPACE)


class HostRefocus(namedtuple("HostRefocus", "rgb valid radius count")):
    """A refocused picture on the host: ``rgb`` uint8 [h, w, 3], ``valid`` uint8 [h, w] (1: the pixel is usable), ``radius`` uint16
    [h, w] | None (the blur radius in sixteenths of a pixel, 0xFFFF where the pixel is not usable), ``count``: a dict of the five counts
    (``COUNT_NAMES``)."""
    __slots__ = ()

    def write_ppm(self, path):
        write_ppm(path, self.rgb)


class Refocus(namedtuple("Refocus", "rgb valid radius count")):
    """The refocused picture on the device: ``rgb`` uint8 in the layout of the colours it was made from ([h, w, 3] or [3, h, w]),
    ``valid`` uint8 [h, w], ``radius`` uint16 [h, w] | None, ``count`` int64 [5]: usable pixels, sharp pixels, capped pixels,
    contributions, and 1 where the focus was bad (the picture is then the source).  Nothing here has been read back."""
    __slots__ = ()

    def to_host(self):
        """The one read-back -> ``HostRefocus``, the picture as [h, w, 3]."""
        h, w = self.valid.shape
        rgb = self.rgb if tuple(self.rgb.shape) == (h, w, 3) else self.rgb.permute(1, 2, 0)
        count = dict(zip(COUNT_NAMES, (int(c) for c in self.count.cpu())))
        return HostRefocus(rgb.contiguous().cpu().numpy(), self.valid.cpu().numpy(), None if self.radius is None else self.radius.cpu().numpy(), count)

    def write_ppm(self, path):
        self.to_host().write_ppm(path)


def refocus(depth, colors, *, focus=None, focus_at=None, gain=None, space="lens", K=None, aperture=None, max_radius=16, coef=None, mask=None,
            z_range=(0.0, math.inf), radius=False, lib=None):
    """The picture ``colors`` with a shallow depth of field around a focus distance -> ``Refocus``, everything on the device and
    nothing read back.  ``depth``, ``coef``, ``mask``, ``z_range``: as in ``depth_to_points``; ``colors``: uint8 [h, w, 3] or
    [3, h, w] on the map's device.  Exactly one of ``focus``, the focus distance in the units of z, and ``focus_at`` = (y, x), a
    pixel whose distance is read on the device.  A usable pixel at distance z is blurred over a disc of radius
    ``gain * |1 / z - 1 / focus|`` pixels in ``space`` "lens" - the thin lens, for which ``K`` and ``aperture`` (in the units of z)
    are shorthand: ``gain = 0.5 * K.fx * aperture`` - and ``gain * |z - focus|`` pixels in ``space`` "linear", capped at
    ``max_radius`` (0 to 32).  A near, blurred surface spreads over what is behind it; a far one shows on a pixel only as far as that
    pixel is blurred itself.  A pixel that is not usable keeps its bytes.  With a focus that is not usable, not finite, or <= 0 in
    lens space, the picture is the source and ``count[4]`` is 1.  ``radius=True`` adds the map of blur radii."""
    who = "refocus"
    # what can be judged without the map comes first, so that it is judged the same with and without a device
    if space not in L.FOCUS_SPACE:
        raise ValueError(f'{who}: space must be "lens" or "linear" (got {space!r})')
    if (focus is None) == (focus_at is None):
        raise ValueError(f"{who}: exactly one of focus and focus_at is expected (got {focus!r} and {focus_at!r})")
    fx = fy = -1
    z_focus = 0.0
    if focus is not None:
        z_focus = P._number(who, "focus", focus)
    else:
        try:
            fy, fx = focus_at
        except (TypeError, ValueError):
            raise ValueError(f"{who}: focus_at must be (y, x), a pixel of the map (got {focus_at!r})") from None
        if any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in (fy, fx)):
            raise ValueError(f"{who}: focus_at must be (y, x), a pixel of the map (got {focus_at!r})")
    if (K is None) != (aperture is None) or (gain is None) == (K is None):
        raise ValueError(f"{who}: either gain, or K with aperture, is expected")
    if gain is None:
        if space != "lens":
            raise ValueError(f'{who}: K and aperture describe a thin lens: space must be "lens" (got {space!r})')
        try:
            K = P.Intrinsics(*(P._number(who, "the camera", v) for v in K))
        except (TypeError, ValueError):
            raise ValueError(f"{who}: K must be Intrinsics(fx, fy, cx, cy) (got {K!r})") from None
        gain = 0.5 * K.fx * P._number(who, "aperture", aperture)
    gain = P._number(who, "gain", gain)
    if not (math.isfinite(gain) and gain >= 0.0):
        raise ValueError(f"{who}: gain must be finite and >= 0 (got {gain!r})")
    if isinstance(max_radius, bool) or not isinstance(max_radius, int) or not 0 <= max_radius <= L.FOCUS_MAX_RADIUS:
        raise ValueError(f"{who}: max_radius must be an integer from 0 to {L.FOCUS_MAX_RADIUS} (got {max_radius!r})")
    depth, h, w, _, coef, mask, z_min, z_max, _, _ = P._common(who, depth, (1.0, 1.0, 0.0, 0.0), coef, mask, z_range, 0.0, "camera")
    if not (isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 and colors.device == depth.device
            and tuple(colors.shape) in ((h, w, 3), (3, h, w))):
        raise ValueError(f"{who}: colors must be a uint8 tensor [{h}, {w}, 3] or [3, {h}, {w}] on the map's device")
    hwc = int(tuple(colors.shape) == (h, w, 3))
    colors = colors.contiguous()
    if focus_at is not None and not (fy < h and fx < w):
        raise ValueError(f"{who}: focus_at {focus_at!r} is outside the map of {h} x {w}")
    lib = lib if lib is not None else L.init(depth.device.index or 0)
    dev = depth.device
    with torch.cuda.device(dev):
        need = lib.mg_depth_focus_workspace_bytes(h * w)
        if need < 0:
            L.check(1, "mg_depth_focus_workspace_bytes", lib)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rgb = torch.empty((h, w, 3) if hwc else (3, h, w), dtype=torch.uint8, device=dev)
        valid = torch.empty((h, w), dtype=torch.uint8, device=dev)
        rad = torch.empty((h, w), dtype=torch.uint16, device=dev) if radius else None
        count = torch.empty(5, dtype=torch.int64, device=dev)
        L.check(lib.mg_depth_focus(depth.data_ptr(), colors.data_ptr(), hwc, P._ptr(mask), P._ptr(coef), h, w, z_min, z_max, L.FOCUS_SPACE[space],
                                   gain, max_radius, fx, fy, z_focus, rgb.data_ptr(), valid.data_ptr(), P._ptr(rad), count.data_ptr(),
                                   ws.data_ptr(), need, O.current_stream_handle()), "mg_depth_focus", lib)
    return Refocus(rgb, valid, rad, count)
