"""Edge-guided upsampling of a prediction to the input picture's size: joint bilateral upsampling, ``mg_guided_upsample``
(csrc/guided.hip; the definition is in include/marigold_hip.h).  The low-resolution prediction is enlarged while the full-size picture,
as uint8, decides which low-resolution neighbours a pixel may borrow from, so depth discontinuities, normal creases and albedo borders
follow the picture's edges instead of being smeared by a bilinear enlargement.  ``guided_upsample`` takes CUDA tensors and runs on the
current stream; nothing here synchronises.  ``pipe(image, guided_upsample=True)`` is built on it."""
import math

import torch

from . import _lib as L, ops as O
from .util.image_util import InterpolationMode, resize

DEFAULT_RADIUS, DEFAULT_SIGMA = 2, 0.1


def settings(value):
    """The pipelines' ``guided_upsample=`` keyword -> None (off) | (radius, sigma): ``True`` means the defaults, a dict carries
    ``radius`` and / or ``sigma``.  ``False`` is off, like ``None``."""
    if value is None or value is False:
        return None
    if value is True:
        return DEFAULT_RADIUS, DEFAULT_SIGMA
    if not isinstance(value, dict):
        raise ValueError(f"guided_upsample must be None, True or a dict with radius and / or sigma (got {value!r})")
    unknown = set(value) - {"radius", "sigma"}
    if unknown:
        raise ValueError(f"guided_upsample: unknown keys {sorted(unknown)} (radius and sigma are understood)")
    return _check(value.get("radius", DEFAULT_RADIUS), value.get("sigma", DEFAULT_SIGMA))


def _check(radius, sigma):
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= 4:
        raise ValueError(f"guided_upsample: radius must be an integer from 1 to 4 (got {radius!r})")
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"guided_upsample: sigma must be finite and > 0 (got {sigma!r})")
    return int(radius), sigma


def guided_upsample(pred, picture_u8, radius=DEFAULT_RADIUS, sigma=DEFAULT_SIGMA, hwc=None, lib=None):
    """``pred`` - fp32 CUDA [C, h, w] (1 <= C <= 16) or [h, w] - enlarged to the size of ``picture_u8`` -> fp32 CUDA [C, H, W] ([H, W]
    for a prediction given without a channel axis).  ``picture_u8``: the uint8 picture on the prediction's device, [H, W, 3] as PIL
    holds it or [3, H, W] / [1, 3, H, W]; ``hwc`` says which where the shape leaves it open ([3, W, 3]; default: channels first then).
    The low-resolution guide is the picture resampled to (h, w) by the uint8 ``resize(..., bilinear, antialias=True)``; then one launch of
    ``mg_guided_upsample`` with ``radius`` (1 .. 4) and ``sigma`` (> 0, on the 0 .. 1 colour scale).  ``lib``: the loaded library to call
    (default: the bf16-operand one; the kernel is fp32 and gives the same bits in both)."""
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() in (2, 3)):
        raise ValueError("guided_upsample: the prediction must be an fp32 CUDA tensor [C, h, w] or [h, w]")
    squeeze = pred.dim() == 2
    pred = (pred.unsqueeze(0) if squeeze else pred).contiguous()
    C, h, w = pred.shape
    if not 1 <= C <= 16 or min(h, w) < 1:
        raise ValueError(f"guided_upsample: a prediction of {C} channels of {h} x {w}; 1 to 16 channels of at least 1 x 1 are supported")
    p = picture_u8
    if not (isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and p.device == pred.device):
        raise ValueError("guided_upsample: the picture must be a uint8 tensor on the prediction's device")
    if p.dim() == 4 and p.shape[0] == 1:
        p = p[0]
    if p.dim() != 3 or 3 not in (p.shape[0], p.shape[-1]) or p.numel() == 0:
        raise ValueError(f"guided_upsample: the picture must be [H, W, 3], [3, H, W] or [1, 3, H, W], got {tuple(picture_u8.shape)}")
    if hwc is None:
        hwc = p.shape[0] != 3
    elif p.shape[-1 if hwc else 0] != 3:
        raise ValueError(f"guided_upsample: hwc={hwc!r} does not fit a picture of shape {tuple(picture_u8.shape)}")
    radius, sigma = _check(radius, sigma)
    p = p.contiguous()
    planes = p.permute(2, 0, 1) if hwc else p   # the resize reads planes; the full-size picture itself goes to the kernel as it lies
    H, W = planes.shape[-2:]
    lib = lib if lib is not None else L.init(pred.device.index or 0)
    with torch.cuda.device(pred.device):
        lo = resize(planes, (h, w), InterpolationMode.BILINEAR, antialias=True).contiguous()
        out = torch.empty((C, H, W), dtype=torch.float32, device=pred.device)
        L.check(lib.mg_guided_upsample(pred.data_ptr(), C, h, w, lo.data_ptr(), p.data_ptr(), int(bool(hwc)), H, W, radius, sigma,
                                       out.data_ptr(), O.current_stream_handle()), "mg_guided_upsample", lib)
    return out[0] if squeeze else out
