"""Image helpers with the reference's semantics (marigold/util/image_util.py), restated on
torch.nn.functional because torchvision is not a dependency here.

``resize`` reproduces torchvision.transforms.functional.resize(img, size, mode, antialias=True)
(SURVEY.md App. C.8): == F.interpolate(..., align_corners=False, antialias=True); uint8 inputs are
computed in float, rounded and cast back; the input is returned unchanged when the size already
matches; NEAREST_EXACT == mode "nearest-exact".  CUDA tensors (uint8 / fp32) go through the HIP
resampling kernels (csrc/resize.hip, MG_OP_RESIZE); host tensors use torch's CPU implementation,
which is also the parity reference of the kernels.
"""
import enum

import numpy as np
import torch


class InterpolationMode(enum.Enum):
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"
    NEAREST_EXACT = "nearest-exact"


_HIP_MODES = {"bilinear": 0, "bicubic": 1, "nearest-exact": 2}   # (= ops.RESIZE_MODES)


def _resize_hip(img, h, w, mode):
    """Device path (csrc/resize.hip): uint8 or fp32 CUDA tensors [..., H, W]."""
    from .. import ops as O
    src = img.contiguous()
    planes = src.numel() // (src.shape[-2] * src.shape[-1])
    Hin, Win = src.shape[-2:]
    dst = torch.empty(src.shape[:-2] + (h, w), dtype=src.dtype, device=src.device)
    tmp = None
    if mode != "nearest-exact" and Hin != h and Win != w:
        tmp = torch.empty(planes * Hin * w, dtype=torch.float32, device=src.device)
    O.launch(O.resize(src, dst, tmp, planes=planes, Hin=Hin, Win=Win, Hout=h, Wout=w, mode=_HIP_MODES[mode],
                      u8=src.dtype == torch.uint8))
    return dst


def resize(img: torch.Tensor, size, interpolation=InterpolationMode.BILINEAR, antialias=True):
    h, w = int(size[0]), int(size[1])
    if tuple(img.shape[-2:]) == (h, w):
        return img
    mode = interpolation.value
    if img.is_cuda and antialias and img.dtype in (torch.uint8, torch.float32):
        return _resize_hip(img, h, w, mode)
    if mode == "nearest-exact":
        return torch.nn.functional.interpolate(img, size=(h, w), mode=mode)
    x = img
    is_int = not torch.is_floating_point(img)
    if is_int or img.dtype in (torch.bfloat16, torch.float16):
        x = img.to(torch.float32)
    y = torch.nn.functional.interpolate(x, size=(h, w), mode=mode, align_corners=False, antialias=antialias)
    if is_int:
        if mode == "bicubic":
            y = y.clamp(0, 255)
        y = y.round().to(img.dtype)
    elif y.dtype != img.dtype:
        y = y.to(img.dtype)
    return y


def resize_max_res(img: torch.Tensor, max_edge_resolution: int,
                   resample_method: InterpolationMode = InterpolationMode.BILINEAR) -> torch.Tensor:
    """Resize so the longer edge equals ``max_edge_resolution`` (may up-scale; no rounding to a
    multiple of 8) - reference :90-120."""
    assert 4 == img.dim(), f"Invalid input shape {img.shape}"
    return resize(img, max_res_size(img.shape[-2:], max_edge_resolution), resample_method, antialias=True)


def max_res_size(hw, max_edge_resolution: int):
    """(height, width) that ``resize_max_res`` resizes an image of size ``hw`` to."""
    original_height, original_width = hw
    downscale_factor = min(max_edge_resolution / original_width, max_edge_resolution / original_height)
    new_width = int(original_width * downscale_factor)
    new_height = int(original_height * downscale_factor)
    return new_height, new_width


def get_tv_resample_method(method_str: str) -> InterpolationMode:
    table = {"bilinear": InterpolationMode.BILINEAR, "bicubic": InterpolationMode.BICUBIC,
             "nearest": InterpolationMode.NEAREST_EXACT, "nearest-exact": InterpolationMode.NEAREST_EXACT}
    m = table.get(method_str, None)
    if m is None:
        raise ValueError(f"Unknown resampling method: {m}")
    return m


def colorize_depth_maps(depth_map, min_depth, max_depth, cmap="Spectral", valid_mask=None):
    """matplotlib colormap lookup -> float [ (B,) 3, H, W ] in (0, 1) - reference :38-76."""
    import matplotlib

    assert len(depth_map.shape) >= 2, "Invalid dimension"
    if isinstance(depth_map, torch.Tensor):
        depth = depth_map.detach().squeeze().numpy()
    else:
        depth = np.asarray(depth_map).copy().squeeze()
    if depth.ndim < 3:
        depth = depth[np.newaxis, :, :]
    cm = matplotlib.colormaps[cmap]
    depth = ((depth - min_depth) / (max_depth - min_depth)).clip(0, 1)
    img = cm(depth, bytes=False)[:, :, :, 0:3]
    img = np.rollaxis(img, 3, 1)
    if valid_mask is not None:
        if isinstance(valid_mask, torch.Tensor):
            valid_mask = valid_mask.detach().numpy()
        valid_mask = valid_mask.squeeze()
        valid_mask = valid_mask[np.newaxis, np.newaxis] if valid_mask.ndim < 3 else valid_mask[:, np.newaxis]
        img[~np.repeat(valid_mask, 3, axis=1)] = 0
    if isinstance(depth_map, torch.Tensor):
        return torch.from_numpy(img).float()
    return img


_LUT_CACHE = {}


def colormap_lut_u8(cmap):
    """matplotlib's 256-entry table of ``cmap`` as the uint8 RGB values the reference ends up with:
    (cm(k / 256 + eps)[:3] * 255).astype(uint8) for table entry k."""
    import matplotlib
    cm = matplotlib.colormaps[cmap]
    idx = (np.arange(256, dtype=np.float64) + 0.5) / 256.0          # x with int(x * 256) == k
    return (cm(idx, bytes=False)[:, 0:3] * 255).astype(np.uint8)


def colorize_depth_device(depth: torch.Tensor, min_depth=0.0, max_depth=1.0, cmap="Spectral") -> torch.Tensor:
    """Device form of ``(colorize_depth_maps(depth, lo, hi, cmap) * 255).astype(uint8)`` in HWC order: fp32 CUDA map
    [H, W] -> uint8 CUDA image [H, W, 3] (csrc/resize.hip, MG_OP_COLORIZE: one table look-up pass)."""
    from .. import ops as O
    assert depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 2
    key = (cmap, depth.device)
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = torch.from_numpy(colormap_lut_u8(cmap)).to(depth.device).contiguous()
    d = depth.contiguous()
    out = torch.empty(d.shape + (3,), dtype=torch.uint8, device=d.device)
    O.launch(O.colorize(d, _LUT_CACHE[key], out, n=d.numel(), lo=min_depth, hi=max_depth))
    return out


def depth_output_device(depth: torch.Tensor, cmap="Spectral", in_place=False):
    """The depth pipeline's output stage in one launch (csrc/resize.hip, MG_OP_COLORIZE with its optional outputs): fp32 CUDA map
    [H, W] -> (clipped fp32 [H, W] = ``clip(depth, 0, 1)`` keeping NaN, u16 uint16 [H, W] = ``(clipped * 65535).astype(uint16)`` - what
    the command line writes as the 16-bit PNG; NaN gives 0 -, picture uint8 [H, W, 3] | None when ``cmap`` is None).  ``in_place``:
    the clipped values overwrite ``depth`` (which must be contiguous) and are returned as it."""
    from .. import ops as O
    assert depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 2
    assert not in_place or depth.is_contiguous(), "depth_output_device: in place needs a contiguous map"
    with torch.cuda.device(depth.device):
        d = depth.contiguous()
        lut = pic = None
        if cmap is not None:
            key = (cmap, d.device)
            if key not in _LUT_CACHE:
                _LUT_CACHE[key] = torch.from_numpy(colormap_lut_u8(cmap)).to(d.device).contiguous()
            lut = _LUT_CACHE[key]
            pic = torch.empty(d.shape + (3,), dtype=torch.uint8, device=d.device)
        clipped = d if in_place else torch.empty_like(d)
        u16 = torch.empty(d.shape, dtype=torch.uint16, device=d.device)
        O.launch(O.colorize(d, lut, pic, n=d.numel(), clipped=clipped, u16=u16))
    return clipped, u16, pic


def iid_visualization_device(pred: torch.Tensor, linear, up_to_scale) -> torch.Tensor:
    """Device form of the images ``MarigoldIIDOutput.fill_entry`` builds, for all targets of one image at once: fp32 CUDA
    ``pred`` [n, 3, H, W] (or [3, H, W]) -> uint8 CUDA [n, H, W, 3].  Per target t: ``linear[t]`` = its prediction space is
    linear (display gamma 1 / 2.2), ``up_to_scale[t]`` = a linear target is divided by max(its maximum, 1e-6) first; then
    ``(x * 255).astype(uint8)``.  csrc/resize.hip, MG_OP_IID_VIS: at most two launches on the caller's current stream."""
    from .. import _lib as L, ops as O
    if pred.dim() == 3:
        pred = pred[None]
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 4 and pred.shape[1] == 3, \
        f"iid_visualization_device: fp32 CUDA [n, 3, H, W] expected, got {pred.dtype} {tuple(pred.shape)} on {pred.device}"
    n, _, h, w = pred.shape
    linear, up_to_scale = [bool(v) for v in linear], [bool(v) for v in up_to_scale]
    if len(linear) != n or len(up_to_scale) != n:
        raise ValueError(f"iid_visualization_device: {n} target(s), {len(linear)} linear and {len(up_to_scale)} up_to_scale flag(s)")
    with torch.cuda.device(pred.device):
        src = pred.contiguous()
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=src.device)
        ws = None
        if any(a and b for a, b in zip(linear, up_to_scale)):
            ws = torch.empty((n, L.IID_VIS_PARTS), dtype=torch.float32, device=src.device)
        O.launch(O.iid_vis(src, out, ws, n=n, H=h, W=w, linear=linear, up_to_scale=up_to_scale))
    return out


def prepare_rgb_device(image_u8: torch.Tensor, size=None, interpolation=InterpolationMode.BILINEAR, io_dtype=torch.float32, hwc=True,
                       device=None, reciprocal=None) -> torch.Tensor:
    """Device form of the pipelines' input stage: the uint8 picture ``image_u8`` - [H, W, 3] as PIL holds it (``hwc``) or [(1,) 3, H, W]
    - is uploaded as it is (a CUDA tensor stays where it is; ``device`` names the GPU of a host tensor) and one MG_OP_RGB_PREP
    (csrc/resize.hip) produces ``(resize(x, size, interpolation) / 255.0 * 2.0 - 1.0).to(io_dtype)`` as [1, 3, h, w]: one launch
    for the same size (``size`` None or the picture's own), else the resampling launches with the uint8 rounding and the
    normalisation in the last one's store.  ``io_dtype``: fp32, or bf16 / fp16 through the library of that operand type.
    ``reciprocal``: round like torch's DEVICE kernel, which multiplies by fp32(1 / 255) where the host kernel divides (111 of the
    256 byte values come out one ulp apart) - by default what a pipeline's ``_preprocess`` ran before this stage existed: the
    device chain after a device resample, the host chain otherwise."""
    from .. import _lib as L, ops as O
    assert image_u8.dtype == torch.uint8, f"prepare_rgb_device: uint8 expected, got {image_u8.dtype}"
    if io_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"prepare_rgb_device: io_dtype {io_dtype} is not fp32, bf16 or fp16")
    x = image_u8
    if hwc:
        assert x.dim() == 3 and x.shape[-1] == 3, f"prepare_rgb_device: [H, W, 3] expected, got {tuple(x.shape)}"
        Hin, Win = x.shape[:2]
    else:
        assert x.dim() in (3, 4) and x.shape[-3] == 3 and x.numel() == 3 * x.shape[-2] * x.shape[-1], \
            f"prepare_rgb_device: [(1,) 3, H, W] expected, got {tuple(x.shape)}"
        Hin, Win = x.shape[-2:]
    h, w = (Hin, Win) if size is None else (int(size[0]), int(size[1]))
    if reciprocal is None:
        reciprocal = (h, w) != (Hin, Win)
    if not x.is_cuda:
        x = x.to(device if device is not None else "cuda")
    assert x.is_cuda, "prepare_rgb_device: a CUDA device is required"
    mode = interpolation.value
    with torch.cuda.device(x.device):
        src = x.contiguous()
        dst = torch.empty((1, 3, h, w), dtype=io_dtype, device=src.device)
        tmp = None
        if mode != "nearest-exact" and Hin != h and Win != w:
            tmp = torch.empty(3 * Hin * w, dtype=torch.float32, device=src.device)
        O.launch(O.rgb_prep(src, dst, tmp, Hin=Hin, Win=Win, Hout=h, Wout=w, mode=mode, hwc=hwc, out16=io_dtype != torch.float32,
                            reciprocal=reciprocal), lib=L.load(io_dtype == torch.float16))
    return dst


def normals_visualization_device(pred: torch.Tensor) -> torch.Tensor:
    """Device form of the normals picture ``chw2hwc(((pred.clip(-1, 1) + 1) * 127.5).astype(uint8))``: fp32 CUDA ``pred`` [3, H, W] ->
    uint8 CUDA [H, W, 3] (csrc/resize.hip, MG_OP_NORMALS_VIS: one launch on the caller's current stream; NaN gives 0)."""
    from .. import ops as O
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 3 and pred.shape[0] == 3, \
        f"normals_visualization_device: fp32 CUDA [3, H, W] expected, got {pred.dtype} {tuple(pred.shape)} on {pred.device}"
    with torch.cuda.device(pred.device):
        src = pred.contiguous()
        out = torch.empty(tuple(src.shape[1:]) + (3,), dtype=torch.uint8, device=src.device)
        O.launch(O.normals_vis(src, out, H=src.shape[1], W=src.shape[2]))
    return out


def normals_output_device(pred: torch.Tensor, in_place=False):
    """The normals pipeline's output stage in one launch (``mg_normals_finish``, MG_OP_NORMALS_VIS's kernel): fp32 CUDA ``pred``
    [3, H, W] -> (clipped fp32 [3, H, W] = ``clip(pred, -1, 1)`` keeping NaN, picture uint8 [H, W, 3]).  ``in_place``: the clipped
    values overwrite ``pred`` (contiguous)."""
    from .. import _lib as L, ops as O
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 3 and pred.shape[0] == 3, \
        f"normals_output_device: fp32 CUDA [3, H, W] expected, got {pred.dtype} {tuple(pred.shape)} on {pred.device}"
    assert not in_place or pred.is_contiguous(), "normals_output_device: in place needs a contiguous map"
    with torch.cuda.device(pred.device):
        src = pred.contiguous()
        clipped = src if in_place else torch.empty_like(src)
        out = torch.empty(tuple(src.shape[1:]) + (3,), dtype=torch.uint8, device=src.device)
        lib = L.load()
        L.check(lib.mg_normals_finish(src.data_ptr(), src.shape[1], src.shape[2], clipped.data_ptr(), out.data_ptr(), O.current_stream_handle()),
                "mg_normals_finish", lib)
    return clipped, out


def chw2hwc(chw):
    assert 3 == len(chw.shape)
    if isinstance(chw, torch.Tensor):
        return torch.permute(chw, (1, 2, 0))
    if isinstance(chw, np.ndarray):
        return np.moveaxis(chw, 0, -1)
    raise TypeError("img should be np.ndarray or torch.Tensor")


def pil_to_tensor(img):
    """PIL RGB -> uint8 [3,H,W] (no scaling), like torchvision's pil_to_tensor."""
    arr = np.asarray(img)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def float2int(img):
    """[0,1] float -> uint8 by truncation (reference image_util.py:137-141)."""
    if isinstance(img, np.ndarray):
        return (img * 255.0).astype(np.uint8)
    return (img * 255.0).to(torch.uint8)


def srgb2linear(img):
    """gamma-2.2 decode (reference image_util.py:144-145)."""
    return img ** 2.2


def linear2srgb(img):
    return img ** (1.0 / 2.2)
