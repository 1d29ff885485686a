"""Tiled predictions of a large picture: the plan of overlapping tiles, the gather of the tiles out of the uint8
picture, the scale-and-shift fit of depth tiles to a low-resolution guide and the feathered blend over the full-size canvas -
``mg_tile_plan`` / ``mg_tile_crop`` / ``mg_tile_fit`` / ``mg_tile_blend`` (csrc/tiles.hip; the contract is in include/marigold_hip.h).
``crop``, ``fit`` and ``blend`` take CUDA tensors and run on the current stream; nothing here synchronises or reads a tile back.
``MarigoldDepthPipeline.predict_tiled`` / ``MarigoldNormalsPipeline.predict_tiled`` are built on ``plan``, ``fit`` and ``blend``;
``mg_model_predict_tiled`` on all four."""
import ctypes
from collections import namedtuple

import torch

from . import _lib as L, ops as O

TilePlan = namedtuple("TilePlan", "ystarts xstarts tile_hw origins")
TilePlan.__doc__ = """``ystarts`` / ``xstarts``: the tile starts along either axis; ``tile_hw``: the extent of every tile (the picture's
where it is smaller than the tile size); ``origins``: [(y0, x0)] of the len(ystarts) * len(xstarts) tiles, row-major."""


def _pair(v, name):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be an int or (h, w), got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _plan_axis(lib, length, tile, overlap):
    starts = (ctypes.c_int * L.TILE_MAX_PER_AXIS)()
    n = lib.mg_tile_plan(int(length), int(tile), int(overlap), starts, L.TILE_MAX_PER_AXIS)
    if n < 1:
        raise L.MarigoldHipError(lib.mg_last_error().decode(errors="replace") or "mg_tile_plan: error")
    return tuple(starts[:n])


def plan(hw, tile_size, overlap) -> TilePlan:
    """The tiles of a picture of ``hw`` = (H, W): ``tile_size`` and ``overlap`` (the minimum, along either axis) are ints or (h, w);
    all lengths are multiples of 8.  Host only (``mg_tile_plan``, once per axis)."""
    lib = L.load()
    (H, W), (th, tw), (oy, ox) = _pair(hw, "hw"), _pair(tile_size, "tile_size"), _pair(overlap, "overlap")
    ys, xs = _plan_axis(lib, H, th, oy), _plan_axis(lib, W, tw, ox)
    return TilePlan(ys, xs, (min(th, H), min(tw, W)), tuple((y, x) for y in ys for x in xs))


def _grid(origins, n, what):
    """[(y0, x0)] of n tiles in row-major order -> (ystarts, xstarts) as ctypes arrays; the origins must be a grid's"""
    origins = [(int(y), int(x)) for y, x in origins]
    if len(origins) != n:
        raise ValueError(f"{what}: {len(origins)} origins for {n} tiles")
    ys, xs = sorted({y for y, _ in origins}), sorted({x for _, x in origins})
    if origins != [(y, x) for y in ys for x in xs]:
        raise ValueError(f"{what}: the origins must be those of a grid of tiles in row-major order (tiles.plan(...).origins)")
    if max(len(ys), len(xs)) > L.TILE_MAX_PER_AXIS:
        raise ValueError(f"{what}: {len(ys)} x {len(xs)} tiles, at most {L.TILE_MAX_PER_AXIS} along an axis are supported")
    return (ctypes.c_int * len(ys))(*ys), len(ys), (ctypes.c_int * len(xs))(*xs), len(xs)


def _lib_and_tiles(tiles, what, dims, lib):
    if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.dtype == torch.float32 and tiles.dim() == dims):
        raise ValueError(f"{what}: the tiles must be a {dims}-dimensional fp32 CUDA tensor")
    return lib if lib is not None else L.init(tiles.device.index or 0), tiles.contiguous()


def crop(picture_u8, plan, first=0, count=None, out=None, lib=None):
    """``count`` tiles of ``plan`` (a ``TilePlan``; default: all from ``first`` on), starting at tile ``first`` in row-major order,
    gathered out of the uint8 CUDA picture in ONE launch (``mg_tile_crop``) -> uint8 CUDA [count, th, tw, 3] for a picture [H, W, 3],
    [count, 3, th, tw] for a picture [3, H, W] or [1, 3, H, W]: what ``picture[..., y0:y0 + th, x0:x0 + tw]`` gives tile by tile.  The
    picture may start at any byte.  ``out``: a contiguous uint8 CUDA tensor of count * 3 * th * tw elements to write into (any
    alignment); the result is a view of it.  Runs on the current stream, does not synchronise."""
    p = picture_u8
    if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.uint8):
        raise ValueError("tiles.crop: the picture must be a uint8 CUDA tensor")
    if p.dim() == 4 and p.shape[0] == 1:
        p = p[0]
    if p.dim() != 3 or 3 not in (p.shape[0], p.shape[-1]):
        raise ValueError(f"tiles.crop: the picture must be [H, W, 3], [3, H, W] or [1, 3, H, W], got {tuple(picture_u8.shape)}")
    hwc = p.shape[-1] == 3
    p = p.contiguous()
    Hw, Ww = (p.shape[0], p.shape[1]) if hwc else (p.shape[1], p.shape[2])
    th, tw = plan.tile_hw
    n = len(plan.origins)
    first = int(first)
    count = n - first if count is None else int(count)
    ys, ny, xs, nx = _grid(plan.origins, n, "tiles.crop")
    shape = (max(count, 0), th, tw, 3) if hwc else (max(count, 0), 3, th, tw)
    lib = lib if lib is not None else L.init(p.device.index or 0)
    with torch.cuda.device(p.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=p.device)
        elif not (isinstance(out, torch.Tensor) and out.device == p.device and out.dtype == torch.uint8 and out.is_contiguous()
                  and out.numel() == max(count, 0) * 3 * th * tw):
            raise ValueError(f"tiles.crop: out must be a contiguous uint8 tensor of {max(count, 0) * 3 * th * tw} elements on the picture's device")
        L.check(lib.mg_tile_crop(p.data_ptr(), int(hwc), Hw, Ww, th, tw, ys, ny, xs, nx, first, count, out.data_ptr(),
                                 O.current_stream_handle()), "mg_tile_crop", lib)
    return out.view(shape)


def fit(tiles, origins, guide, canvas_hw, lib=None):
    """Per tile the scale and shift that carry it onto ``guide``, least squares over the pixels where both are finite.
    ``tiles`` [n, th, tw] fp32 CUDA; ``origins`` [(y0, x0)] on the working canvas ``canvas_hw`` (a grid's, row-major); ``guide``
    [hg, wg] fp32 CUDA, read bilinearly at every pixel's canvas position.  -> (``coef`` [n, 2] fp64 CUDA: (s, t) per tile,
    ``flags`` [n] int32 CUDA: 1 marks a degenerate tile - constant, fewer than two valid pixels or a slope <= 0 - which gets s = 0
    and the guide's mean as t).  Deterministic: fixed chunks, no atomics.  ``lib``: the loaded library to call (default: the bf16-operand
    one; the entry points are the same in both)."""
    lib, tiles = _lib_and_tiles(tiles, "tiles.fit", 3, lib)
    n, th, tw = tiles.shape
    if not (isinstance(guide, torch.Tensor) and guide.device == tiles.device and guide.dtype == torch.float32 and guide.dim() == 2):
        raise ValueError("tiles.fit: the guide must be a [hg, wg] fp32 tensor on the tiles' device")
    guide = guide.contiguous()
    ys, ny, xs, nx = _grid(origins, n, "tiles.fit")
    Hw, Ww = _pair(canvas_hw, "canvas_hw")
    need = lib.mg_tiles_workspace_bytes(n, th, tw)
    L.check(0 if need >= 0 else 1, "mg_tiles_workspace_bytes", lib)
    with torch.cuda.device(tiles.device):
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=tiles.device)
        coef = torch.empty((n, 2), dtype=torch.float64, device=tiles.device)
        flags = torch.empty((n,), dtype=torch.int32, device=tiles.device)
        L.check(lib.mg_tile_fit(tiles.data_ptr(), th, tw, ys, ny, xs, nx, Hw, Ww, guide.data_ptr(), guide.shape[0], guide.shape[1],
                                coef.data_ptr(), flags.data_ptr(), ws.data_ptr(), need, O.current_stream_handle()), "mg_tile_fit", lib)
    return coef, flags


def blend(tiles, origins, canvas_hw, overlap, coef=None, normalize=False, lib=None):
    """The tiles, each mapped by its (s, t) of ``coef`` (``fit``'s; None: as they are), blended over the canvas with feathered weights
    -> [C, H, W] fp32 CUDA ([H, W] for tiles given without a channel axis).  ``tiles`` [n, C, th, tw] or [n, th, tw] fp32 CUDA, C = 1
    or 3; ``origins`` as for ``fit``, covering ``canvas_hw``; ``overlap``: the minimum overlap the plan was made with (int or (h, w)) -
    the length of every feather.  ``normalize`` (C = 3): unit vectors out."""
    squeeze = isinstance(tiles, torch.Tensor) and tiles.dim() == 3
    lib, tiles = _lib_and_tiles(tiles.unsqueeze(1) if squeeze else tiles, "tiles.blend", 4, lib)
    n, C, th, tw = tiles.shape
    ys, ny, xs, nx = _grid(origins, n, "tiles.blend")
    (Hw, Ww), (oy, ox) = _pair(canvas_hw, "canvas_hw"), _pair(overlap, "overlap")
    if coef is not None:
        if not (isinstance(coef, torch.Tensor) and coef.device == tiles.device and coef.dtype == torch.float64 and tuple(coef.shape) == (n, 2)):
            raise ValueError(f"tiles.blend: coef must be a [{n}, 2] fp64 tensor on the tiles' device")
        coef = coef.contiguous()
    if min(Hw, Ww) < 1:
        raise ValueError(f"tiles.blend: bad canvas {Hw} x {Ww}")
    with torch.cuda.device(tiles.device):
        out = torch.empty((C, Hw, Ww), dtype=torch.float32, device=tiles.device)
        L.check(lib.mg_tile_blend(tiles.data_ptr(), C, th, tw, ys, ny, xs, nx, Hw, Ww, oy, ox, None if coef is None else coef.data_ptr(),
                                  int(bool(normalize)), out.data_ptr(), O.current_stream_handle()), "mg_tile_blend", lib)
    return out[0] if squeeze else out
