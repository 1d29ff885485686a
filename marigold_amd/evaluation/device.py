"""The scores of ``metrics.py`` / ``alignment.py`` on the GPU (csrc/evalscore.hip): what the reference's validation loop
does per image (src/trainer/marigold_depth_trainer.py:510-601) - fit, clip and score in one pass on the accelerator, with
no prediction file in between.  One library call and one synchronisation (on the 13- or 9-double result) per image; for
intrinsic images one call per target and one synchronisation per sample (``score_iid_sample``).

Same definitions as the host functions: fp32 element arithmetic, fp64 sums; the sums are reduced in a fixed order, so a
score is the same bits on every call.  There is no host fallback: without the library or a GPU these functions raise.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from . import metrics as M

_workspaces = {}
_act_workspaces = {}   # LPIPS activations: one buffer per (device, library, stream), grown on demand


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


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: the device scorer has no CPU fallback (use evaluation.metrics on the host)")


def _setup(device, f16):
    _require_gpu()
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


_UP_TO_SCALE = ("shading", "residual")   # metrics.compute_iid_metric


def _act_workspace(ws, device, nbytes):
    """The stream's activation buffer of at least ``nbytes`` (a larger image replaces it; the allocator keeps the old one alive for
    the launches already queued on the stream).  It only grows and is never freed: one buffer of the largest image scored, per
    stream that scored one."""
    key = ws.data_ptr()   # one evaluation workspace per (device, library, stream): the same key
    act = _act_workspaces.get(key)
    if act is None or act.numel() < nbytes:
        act = _act_workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return act


def _lpips_launch(lib, ws, stream, device, net, p, g, m, up_to_scale, mode, out8):
    """One mg_eval_iid_lpips call on ``out8`` for the tensors ``_iid_launch`` uploaded."""
    h, w = p.shape[-2:]
    nbytes = lib.mg_lpips_workspace_bytes(h, w)
    if nbytes < 0:
        L.check(1, "mg_lpips_workspace_bytes", lib)
    net.to(device)
    act = _act_workspace(ws, device, nbytes)
    L.check(lib.mg_eval_iid_lpips(ctypes.byref(net._struct), p.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else None, h, w,
                                  int(up_to_scale), mode, out8.data_ptr(), ws.data_ptr(), act.data_ptr(), act.numel(), stream),
            "mg_eval_iid_lpips", lib)


def _lpips_value(values):
    """LPIPS of an out8 row read back; a non-zero out-of-range count is the host function's ValueError."""
    if values[1] != 0:
        raise ValueError(f"lpips: {int(values[1])} element(s) outside [0, 1] (NaN counts): the metric is defined on images in [0, 1]")
    return values[0]


def _iid_launch(lib, ws, stream, device, pred, gt, valid_mask, up_to_scale, gamma, metrics, out8, keep, lpips=None, lpips_out8=None):
    """One mg_eval_iid call on ``out8`` (a row of a device tensor); the uploaded tensors go to ``keep`` until the read-back.  With a
    network in ``lpips``: ``"lpips"`` may be among ``metrics`` and mg_eval_iid_lpips follows on ``lpips_out8``."""
    if lpips is not None:
        metrics = [m for m in metrics if m != "lpips"]
    unknown = [m for m in metrics if m not in L.IID_METRICS]
    if unknown:
        raise NotImplementedError(f"IID metric '{unknown[0]}' (LPIPS needs pretrained network weights that are not part of this engine)")
    mode = L.iid_gamma_mode(gamma)
    p, g = _on_device(pred, device, torch.float32), _on_device(gt, device, torch.float32)
    if p.ndim < 3 or tuple(p.shape[-3:]) != (3,) + tuple(p.shape[-2:]) or p.numel() != 3 * p.shape[-2] * p.shape[-1] \
            or p.shape[-3:] != g.shape[-3:] or p.numel() != g.numel():
        raise ValueError(f"score_iid: shapes {tuple(p.shape)}, {tuple(g.shape)} (want [3,H,W], leading 1s allowed)")
    h, w = p.shape[-2:]
    m = None
    if valid_mask is not None:
        m = _on_device(valid_mask, device, torch.bool)
        if m.numel() != p.numel() or m.shape[-3:] != p.shape[-3:]:
            raise ValueError(f"score_iid: mask shape {tuple(m.shape)} for images {tuple(p.shape)}")
        m = m.view(torch.uint8)
    keep += [p, g, m]
    L.check(lib.mg_eval_iid(p.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else None, h, w, int(up_to_scale),
                            mode, sum(L.IID_METRICS[k] for k in set(metrics)), out8.data_ptr(), ws.data_ptr(), stream),
            "mg_eval_iid", lib)
    if lpips is not None:
        _lpips_launch(lib, ws, stream, device, lpips, p, g, m, up_to_scale, mode, lpips_out8)


def _iid_result(values):
    return dict(psnr=values[0], ssim=values[1], scale=values[2], quantile=values[3], n=int(values[5]))


def score_iid(pred, gt, target_name, valid_mask=None, *, metrics=("psnr", "ssim"), gamma=None, device=None, f16=False, lpips=None):
    """metrics.compute_iid_metric for one target of one image -> ``{"psnr", "ssim", "scale", "quantile", "n"}`` (a metric not in
    ``metrics``: NaN; ``scale``: the least-squares scale, 1 for a plain target; ``quantile``: the 0.9 brightness quantile, NaN for
    a plain target; ``n``: valid elements, 0 -> every score NaN).  ``target_name`` "shading" / "residual" are up to scale: aligned
    and brightness-mapped first.  ``pred`` / ``gt`` [3,H,W] (or [1,3,H,W]), H, W >= 11; ``valid_mask`` bool of the same shape or
    None; ``gamma``: None, 2.2, 1 / 2.2 or (2.2, 1 / 2.2), a number within 1e-3 of one of them counting as it - ``x ** gamma`` in fp32 on both images first, as script/iid/eval.py does
    for linear-space targets and Hypersim's albedo.  Numpy arrays are uploaded, CUDA tensors used in place; one read-back.
    ``metrics`` with ``"lpips"`` needs ``lpips``, an ``evaluation.LpipsNet`` (H, W >= 31): the result gains the key ``"lpips"``
    (``metrics.lpips`` of the same images, fp32 on the device) and the call raises ``ValueError`` when an element of either image,
    as scored, is outside [0, 1]; without a network it is refused as before."""
    _require_gpu()
    device = _device_of(device, pred, gt, valid_mask)
    with torch.cuda.device(device):
        lib, ws, stream = _setup(device, f16)
        net = lpips if "lpips" in metrics else None   # (asked for without a network: _iid_launch refuses it)
        out, keep = torch.empty(8 if net is None else 16, dtype=torch.float64, device=device), []
        _iid_launch(lib, ws, stream, device, pred, gt, valid_mask, target_name in _UP_TO_SCALE, gamma, metrics, out[:8], keep, net, out[8:])
        values = out.cpu().tolist()   # the one synchronisation
    res = _iid_result(values)
    if net is not None:
        res["lpips"] = _lpips_value(values[8:])
    return res


def score_iid_sample(preds, data, target_names, *, metrics=("psnr", "ssim"), use_mask=False, linear_targets=(), dataset_name="",
                     device=None, f16=False, lpips=None):
    """The value row of harness._score_iid for one sample, scored on the GPU: ``preds`` {target: [3,H,W] prediction} (a target that
    is absent or None leaves ``None`` cells), ``data`` the dataset sample (``data[target]``, ``data["mask_" + target]``); values
    metric-major per target; the 2.2 gamma for ``linear_targets`` and the Hypersim three-target albedo rule of
    script/iid/eval.py:166-174.  Every target is launched before the one read-back.  ``lpips``: an ``evaluation.LpipsNet`` - every
    target's values are followed by its LPIPS (the reference's order: psnr, ssim, lpips)."""
    present = [t for t in target_names if preds.get(t) is not None]
    rows = {}
    if present:
        _require_gpu()
        device = _device_of(device, *[preds[t] for t in present])
        with torch.cuda.device(device):
            lib, ws, stream = _setup(device, f16)
            out, keep = torch.empty((len(present), 8 if lpips is None else 16), dtype=torch.float64, device=device), []
            for k, t in enumerate(present):
                gamma = (2.2,) if t in linear_targets else ()
                if "hypersim" in dataset_name and len(target_names) == 3 and t == "albedo":
                    gamma += (1.0 / 2.2,)
                gamma = None if not gamma else gamma[0] if len(gamma) == 1 else gamma
                _iid_launch(lib, ws, stream, device, preds[t], data[t], data["mask_" + t] if use_mask else None,
                            t in _UP_TO_SCALE, gamma, metrics, out[k, :8], keep, lpips, out[k, 8:])   # (the calls share the stream's workspace, in stream order)
            values = out.cpu().tolist()
        rows = {t: _iid_result(v) for t, v in zip(present, values)}
        if lpips is not None:
            for t, v in zip(present, values):
                rows[t]["lpips"] = _lpips_value(v[8:])
    names = list(metrics) if lpips is None else [m for m in metrics if m != "lpips"] + ["lpips"]
    row = []
    for t in target_names:
        row += [rows[t][m] for m in names] if t in rows else [None] * len(names)
    return row
