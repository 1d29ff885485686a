"""Depth alignment on the device: the scale and shift that carry one affine-invariant depth map into the range of
another, fitted robustly - ``mg_depth_align_fit`` / ``mg_depth_align_apply`` (csrc/align.hip; the definitions are in
include/marigold_hip.h).  ``align_depth`` fits a prediction to a reference - a map with trusted values at some pixels, or another
prediction - and hands the aligned map back; ``DepthAlignState`` is what ``pipe(frame, align=state)`` and ``map_video(align=True)``
keep between the frames of a video, so that a frame's range follows the frame before.  Everything takes CUDA tensors and runs on the
current stream; nothing here reads back or synchronises."""
import math

import torch

from . import _lib as L, ops as O

DEFAULT_ITERS, DEFAULT_DELTA = 4, 0.05   # (not tuned on real weights: the checkpoints this project is built with are synthetic)


def _check_fit(who, iters, delta, fit_shift=True):
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= L.ALIGN_MAX_ITERS:
        raise ValueError(f"{who}: iters must be an integer from 0 to {L.ALIGN_MAX_ITERS} (got {iters!r})")
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not (math.isfinite(delta) and delta > 0.0):
        raise ValueError(f"{who}: delta must be finite and > 0 (got {delta!r})")
    return iters, float(delta), bool(fit_shift)


def _check_start(who, start):
    if isinstance(start, str):
        if start != "ls":
            raise ValueError(f'{who}: start must be a pair (s, t) or "ls" (got {start!r})')
        return L.ALIGN_START_LS, 1.0, 0.0
    try:
        s, t = (float(v) for v in start)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: start must be a pair (s, t) or "ls" (got {start!r})') from None
    if not (math.isfinite(s) and math.isfinite(t)):
        raise ValueError(f"{who}: the start values must be finite (got {start!r})")
    return L.ALIGN_START_GIVEN, s, t


def _device_map(who, name, x, like=None):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.numel() >= 1):
        raise ValueError(f"{who}: {name} must be a non-empty fp32 CUDA tensor")
    if like is not None and (tuple(x.shape) != tuple(like.shape) or x.device != like.device):
        raise ValueError(f"{who}: {name} has the shape {tuple(x.shape)} on {x.device}, the prediction {tuple(like.shape)} on {like.device}")
    return x.contiguous()


def fit(pred, ref, mask=None, *, iters=DEFAULT_ITERS, delta=DEFAULT_DELTA, fit_shift=True, start=(1.0, 0.0), lib=None):
    """The fit alone -> (coef, flag): device fp64 [2] (s, t) and device int32 [1] (1: degenerate, the coefficients are (1, 0))."""
    who = "align_depth"
    pred = _device_map(who, "pred", pred)
    ref = _device_map(who, "ref", ref, pred)
    if mask is not None:
        if not (isinstance(mask, torch.Tensor) and mask.dtype in (torch.bool, torch.uint8) and tuple(mask.shape) == tuple(pred.shape)
                and mask.device == pred.device):
            raise ValueError(f"{who}: mask must be a bool or uint8 tensor of the prediction's shape on its device")
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    iters, delta, fit_shift = _check_fit(who, iters, delta, fit_shift)
    mode, s0, t0 = _check_start(who, start)
    lib = lib if lib is not None else L.init(pred.device.index or 0)
    n = pred.numel()
    with torch.cuda.device(pred.device):
        need = lib.mg_depth_align_workspace_bytes(n)
        if need < 0:
            L.check(1, "mg_depth_align_workspace_bytes", lib)
        ws = torch.empty(need, dtype=torch.uint8, device=pred.device)
        coef = torch.empty(2, dtype=torch.float64, device=pred.device)
        flag = torch.empty(1, dtype=torch.int32, device=pred.device)
        L.check(lib.mg_depth_align_fit(pred.data_ptr(), ref.data_ptr(), None if mask is None else mask.data_ptr(), n, int(fit_shift), iters,
                                       mode, s0, t0, delta, coef.data_ptr(), flag.data_ptr(), ws.data_ptr(), need, O.current_stream_handle()),
                "mg_depth_align_fit", lib)
    return coef, flag


def apply(x, coef, *, use_shift=True, clip=None, out=None, lib=None):
    """``s * x + t`` (``use_shift=False``: ``s * x``, how an uncertainty map follows its depth map) with the device coefficients of a
    fit -> fp32 tensor of ``x``'s shape; ``clip`` = (lo, hi) clamps, ``out`` (may be ``x``) receives the result."""
    who = "align_depth"
    x = _device_map(who, "the map", x)
    if not (isinstance(coef, torch.Tensor) and coef.dtype == torch.float64 and coef.numel() == 2 and coef.device == x.device
            and coef.is_contiguous()):
        raise ValueError(f"{who}: coef must be the contiguous fp64 [2] tensor of a fit, on the map's device")
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == x.device and out.is_contiguous()
              and tuple(out.shape) == tuple(x.shape)):
        raise ValueError(f"{who}: out must be a contiguous fp32 tensor of the map's shape on its device")
    lo, hi = (1.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
    if clip is not None and not lo <= hi:
        raise ValueError(f"{who}: clip must be (lo, hi) with lo <= hi (got {clip!r})")
    lib = lib if lib is not None else L.init(x.device.index or 0)
    with torch.cuda.device(x.device):
        L.check(lib.mg_depth_align_apply(x.data_ptr(), x.numel(), coef.data_ptr(), int(bool(use_shift)), lo, hi, out.data_ptr(),
                                         O.current_stream_handle()), "mg_depth_align_apply", lib)
    return out


def align_depth(pred, ref, mask=None, *, iters=DEFAULT_ITERS, delta=DEFAULT_DELTA, fit_shift=True, start=(1.0, 0.0), clip=None, out=None,
                lib=None):
    """``pred`` expressed in the range of ``ref``: the robust fit of ``s * pred + t`` to ``ref`` and its application ->
    (aligned, coef, flag) - the aligned fp32 map, the device fp64 [2] coefficients (s, t) and the device int32 [1] flag (1: the fit was
    degenerate - fewer than two usable pixels, a constant ``pred``, a slope <= 0 - and ``aligned`` is ``pred``).  ``pred``, ``ref``: fp32
    CUDA tensors of one shape; ``mask``: bool / uint8 of that shape, True where a pixel may count; pixels where either map is not finite
    never count.  ``iters`` reweighted solves with Cauchy weights 1 / (1 + (residual / delta)^2) - 0: plain least squares - the first
    weighted from ``start``: a pair (s, t), or "ls" for an unweighted solve done first.  ``fit_shift=False`` fits the scale alone.
    ``clip`` = (lo, hi) clamps the aligned map; ``out`` (may be ``pred``) receives it.  Nothing is read back: look at ``flag`` when you
    choose to.

    Sparse anchors - a few trusted depths (LiDAR returns, SfM points) in ``ref``, anything elsewhere::

        valid = torch.zeros_like(pred, dtype=torch.bool); valid[ys, xs] = True      # where ref holds a measurement
        metric, coef, flag = align_depth(pred, ref, valid, start="ls", delta=0.1)  # delta in ref's units, here 0.1 m

    ``start="ls"`` because the prediction's own range says nothing about the reference's; ``delta`` is the residual, in the units of
    ``ref``, at which a pixel's weight has fallen to a half."""
    coef, flag = fit(pred, ref, mask, iters=iters, delta=delta, fit_shift=fit_shift, start=start, lib=lib)
    return apply(pred, coef, clip=clip, out=out, lib=lib), coef, flag


class DepthAlignState:
    """What ``pipe(frame, align=state)`` / ``map_video(align=True)`` keep from one frame of a video to the next: the depth map later
    frames are fitted to.  Frame 0 of a state passes unchanged and becomes the reference; frame k is fitted to the reference
    (``iters`` Cauchy solves from (1, 0), ``delta`` in depth units) and replaced by ``s * pred + t``.  ``reference="previous"``: the
    aligned, unclipped map of frame k is the next reference; ``"first"``: frame 0's stays.  A frame whose fit is degenerate passes
    unchanged.

    ``reference_map``: None, or the fp32 device tensor [h, w] the next frame is fitted to - the state's own memory, one of the two
    buffers it writes in turn (clone it to keep it).  ``coef`` / ``flag``: the device tensors of the last frame's fit ((1, 0) and 0 for
    frame 0).  ``frames``: how many frames have passed.  ``reset()`` starts a new video.

    Buffer lifetime, as ``SequenceState``'s: frame k reads the reference and writes buffer k % 2 on the stream it runs on, and records
    an event behind its write; frame k + 1, on whichever stream, makes its stream wait for that event first."""

    def __init__(self, iters=DEFAULT_ITERS, delta=DEFAULT_DELTA, reference="previous", fit_shift=True):
        self.iters, self.delta, self.fit_shift = _check_fit("DepthAlignState", iters, delta, fit_shift)
        if reference not in ("previous", "first"):
            raise ValueError(f'DepthAlignState: reference must be "previous" or "first" (got {reference!r})')
        self.reference = reference
        self.reference_map = self.coef = self.flag = None
        self.frames = 0
        self._sig = None             # (processed size, device): what the next frame must match
        self._ring = [None, None]
        self._event = None           # recorded behind the last frame's work (kept over a reset: the buffers are reused)

    def reset(self):
        self.reference_map = self.coef = self.flag = None
        self.frames, self._sig = 0, None

    def _check(self, sig):
        if self._sig is not None and self._sig != sig:
            raise ValueError(f"align: the state holds a reference of {self._sig[0][0]} x {self._sig[0][1]} on {self._sig[1]}, this frame is "
                             f"processed at {sig[0][0]} x {sig[0][1]} on {sig[1]} (reset() starts a new video)")

    def _step(self, pred, uncert, lib, turn=None):
        """One frame's turn, on the current stream: ``pred`` fp32 [..., h, w] with h w elements (the ensembled prediction at the
        processed size), ``uncert`` likewise or None -> (aligned prediction, scaled uncertainty, coef, flag).  ``turn``: (turnstile,
        frame index) where lanes take turns (``map_video``); the host waits there for the frames before to have been QUEUED, never for
        the GPU."""
        if turn is not None:
            turn[0].wait(turn[1])
        device = pred.device
        sig = (tuple(int(v) for v in pred.shape[-2:]), device)
        self._check(sig)
        stream = torch.cuda.current_stream(device)
        if self._event is not None:
            stream.wait_event(self._event)
        flat = pred.float().contiguous()
        keeps = self.frames == 0 or self.reference == "previous"   # this frame's map becomes the reference
        buf = None
        if keeps:
            slot = self.frames % 2
            buf = self._ring[slot]
            if buf is None or tuple(buf.shape) != sig[0] or buf.device != device:
                buf = self._ring[slot] = torch.empty(sig[0], dtype=torch.float32, device=device)
            buf.record_stream(stream)   # (should the state be dropped with work of this stream still queued)
        if self.frames == 0:
            coef = torch.zeros(2, dtype=torch.float64, device=device)   # the identity, made on the device: no upload to wait for
            coef[0].fill_(1.0)
            flag = torch.zeros(1, dtype=torch.int32, device=device)
            buf.copy_(flat.reshape(sig[0]))
            out = pred
        else:
            ref = self.reference_map
            ref.record_stream(stream)
            coef, flag = fit(flat.reshape(sig[0]), ref, iters=self.iters, delta=self.delta, fit_shift=self.fit_shift, lib=lib)
            out = apply(flat, coef, lib=lib)
            if keeps:
                buf.copy_(out.reshape(sig[0]))
            if uncert is not None:
                uncert = apply(uncert.float().contiguous(), coef, use_shift=False, lib=lib)
        if keeps:
            self.reference_map = buf
        self.coef, self.flag, self._sig, self.frames = coef, flag, sig, self.frames + 1
        self._event = torch.cuda.Event()
        self._event.record(stream)
        if turn is not None:
            turn[0].done(turn[1])
        return out, uncert, coef, flag


def settings(value):
    """``map_video``'s ``align=`` keyword -> None (off) | a fresh ``DepthAlignState``: ``True`` means the defaults, a dict carries
    ``iters``, ``delta``, ``reference`` and / or ``fit_shift``.  ``False`` is off, like ``None``."""
    if value is None or value is False:
        return None
    if value is True:
        return DepthAlignState()
    if not isinstance(value, dict):
        raise ValueError(f"map_video: align must be None, True or a dict with iters, delta, reference and / or fit_shift (got {value!r})")
    unknown = set(value) - {"iters", "delta", "reference", "fit_shift"}
    if unknown:
        raise ValueError(f"map_video: align has unknown keys {sorted(unknown)} (iters, delta, reference and fit_shift are understood)")
    return DepthAlignState(**value)
