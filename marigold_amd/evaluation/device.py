"""The scores of ``metrics.py`` / ``alignment.py`` on the GPU (csrc/evalscore.hip): what the reference's validation loop
does per image (src/trainer/marigold_depth_trainer.py:510-601) - fit, clip and score in one pass on the accelerator, with
no prediction file in between.  One library call and one synchronisation (on the 13- or 9-double result) per image.

Same definitions as the host functions: fp32 element arithmetic, fp64 sums; the sums are reduced in a fixed order, so a
score is the same bits on every call.  There is no host fallback: without the library or a GPU these functions raise.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from . import metrics as M

_workspaces = {}


def _device_of(device, *arrays):
    if device is not None:
        return torch.device(device)
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _on_device(a, device, dtype):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def _setup(device, f16):
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: the device scorer has no CPU fallback (use evaluation.metrics on the host)")
    index = device.index if device.index is not None else torch.cuda.current_device()
    lib = L.init(index, f16)
    stream = torch.cuda.current_stream(device)
    key = (index, bool(f16), stream.cuda_stream)   # the workspace belongs to the calls of one stream
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(L.EVAL_WS_BYTES, dtype=torch.uint8, device=device)
    return lib, ws, ctypes.c_void_p(stream.cuda_stream)


def score_depth(pred, gt, valid_mask, *, alignment=None, alignment_max_res=None, min_depth=None, max_depth=None, device=None,
                f16=False):
    """harness.align_and_clip_depth + the ten functions of ``metrics.DEPTH_METRICS`` for one image -> {name: float} in that
    order, then ``scale``, ``shift`` (1, 0 without alignment) and ``n`` (valid pixels).  ``pred`` / ``gt`` [H,W] (or with leading 1s),
    ``valid_mask`` bool; numpy arrays are uploaded, CUDA tensors used in place.  ``f16``: run the fp16-operand build of the library
    (the same fp32 / fp64 kernels)."""
    if alignment not in L.EVAL_ALIGN:
        raise ValueError(f"unknown alignment '{alignment}'")
    device = _device_of(device, pred, gt, valid_mask)
    with torch.cuda.device(device):
        lib, ws, stream = _setup(device, f16)
        p, g = _on_device(pred, device, torch.float32).squeeze(), _on_device(gt, device, torch.float32).squeeze()
        m = _on_device(valid_mask, device, torch.bool).squeeze().view(torch.uint8)
        if p.ndim != 2 or p.shape != g.shape or p.shape != m.shape:
            raise ValueError(f"score_depth: shapes {tuple(p.shape)}, {tuple(g.shape)}, {tuple(m.shape)}")
        out = torch.empty(13, dtype=torch.float64, device=device)
        nan = float("nan")
        L.check(lib.mg_eval_depth(p.data_ptr(), g.data_ptr(), m.data_ptr(), p.shape[0], p.shape[1], L.EVAL_ALIGN[alignment],
                                  int(alignment_max_res or 0), nan if min_depth is None else float(min_depth),
                                  nan if max_depth is None else float(max_depth), out.data_ptr(), ws.data_ptr(), stream),
                "mg_eval_depth", lib)
        values = out.cpu().tolist()   # the one synchronisation
    res = dict(zip(M.DEPTH_METRICS, values[:10]))
    res.update(scale=values[10], shift=values[11], n=int(values[12]))
    return res


def score_normals(pred, gt, masked=True, return_error_map=False, *, rounded=True, device=None, f16=False):
    """metrics.compute_cosine_error + the functions of ``metrics.NORMALS_METRICS`` (+ ``rmse_angular_error``) for one image
    -> {name: float}, rounded to 4 decimals like the host functions (``rounded=False``: as computed), and ``n``; no scored
    pixel: NaN.  ``pred`` / ``gt`` [3,H,W] (or [1,3,H,W]).  With ``return_error_map`` -> (dict, the flat fp32 error map of the kept pixels as a numpy array)."""
    device = _device_of(device, pred, gt)
    with torch.cuda.device(device):
        lib, ws, stream = _setup(device, f16)
        p, g = _on_device(pred, device, torch.float32), _on_device(gt, device, torch.float32)
        p, g = (p[0] if p.ndim == 4 else p), (g[0] if g.ndim == 4 else g)
        assert p.shape[0] == 3 and g.shape[0] == 3, "Channel dim should be the first dimension!"
        p, g = p.reshape(3, -1), g.reshape(3, -1)
        if p.shape != g.shape:
            raise ValueError(f"score_normals: shapes {tuple(p.shape)}, {tuple(g.shape)}")
        hw = p.shape[1]
        out = torch.empty(9, dtype=torch.float64, device=device)
        err = torch.empty(hw, dtype=torch.float32, device=device) if return_error_map else None
        L.check(lib.mg_eval_normals(p.data_ptr(), g.data_ptr(), hw, int(bool(masked)), out.data_ptr(),
                                    err.data_ptr() if err is not None else None, ws.data_ptr(), stream), "mg_eval_normals", lib)
        values = out.cpu().tolist()
        err = err.cpu().numpy() if err is not None else None
    if rounded:
        values[:8] = [round(v, 4) for v in values[:8]]
    res = dict(zip(M.NORMALS_METRICS, values[:7]))
    res.update(rmse_angular_error=values[7], n=int(values[8]))
    if return_error_map:
        return res, err[err != -1.0]   # dropped pixels hold -1 (an angle is >= 0 or NaN)
    return res
