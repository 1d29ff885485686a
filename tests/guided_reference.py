"""A numpy restatement of ``mg_guided_upsample`` (include/marigold_hip.h), the yardstick of the guided-upsampling tests.  Every step
is evaluated in ``dtype``: float64 is the reference, float32 the same restatement at the kernel's precision - the distance between the
two sets the tests' tolerance.  Helper module, no tests of its own."""
import numpy as np


def guided_reference(pred, guide_lo, guide_hi, hwc, radius=2, sigma=0.1, dtype=np.float64):
    """``pred`` [C, h, w]; ``guide_lo`` uint8 [3, h, w]; ``guide_hi`` uint8 [H, W, 3] (``hwc``) or [3, H, W] -> [C, H, W] in ``dtype``."""
    f = np.dtype(dtype).type
    pred = np.asarray(pred, dtype=dtype)
    C, h, w = pred.shape
    lo = np.asarray(guide_lo).astype(dtype) / f(255)                                     # [3, h, w]
    hi = np.asarray(guide_hi)
    hi = (hi.transpose(2, 0, 1) if hwc else hi).astype(dtype) / f(255)                   # [3, H, W]
    H, W = hi.shape[1:]
    R = int(radius)

    def axis(n_in, n_out):
        """-> (tap indices before the clamp [2R, n_out], their tent weights)"""
        scale = f(n_in) / f(n_out)
        s = scale * (np.arange(n_out).astype(dtype) + f(0.5)) - f(0.5)
        first = np.floor(s).astype(np.int64) - R + 1
        taps = first[None, :] + np.arange(2 * R)[:, None]
        wgt = np.maximum(f(0), f(1) - np.abs(s[None, :] - taps.astype(dtype)) / f(R))
        return taps, wgt.astype(dtype)

    (ti, wy), (tj, wx) = axis(h, H), axis(w, W)
    ic, jc = np.clip(ti, 0, h - 1), np.clip(tj, 0, w - 1)
    two_sigma2 = f(2) * f(sigma) * f(sigma)
    weights, values = [], []
    for a in range(2 * R):
        for b in range(2 * R):
            rows, cols = ic[a][:, None], jc[b][None, :]
            d = hi - lo[:, rows, cols]
            d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            rng = np.exp(-d2 / two_sigma2) + f(1e-4)
            weights.append((wy[a][:, None] * wx[b][None, :]) * rng)
            values.append(pred[:, rows, cols])
    den = np.zeros((H, W), dtype=dtype)
    for wt in weights:
        den = den + wt
    out = np.zeros((C, H, W), dtype=dtype)
    for wt, v in zip(weights, values):
        out = out + (wt / den)[None] * v
    assert out.dtype == np.dtype(dtype)
    return out
