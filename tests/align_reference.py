"""The depth alignment of include/marigold_hip.h (``mg_depth_align_fit`` / ``mg_depth_align_apply``) restated in numpy float64: what the
GPU tests measure the kernels against.  Every product and sum is a separate numpy operation, so it rounds as the definition says; only
the ORDER of the sums differs from the kernels' (numpy's pairwise sum here, chunks and shuffle trees there) - ``reverse=True`` sums the
pixels in the opposite order, which is how a test sees whether a case is conditioned well enough for the 1e-9 bound."""
import numpy as np

START_GIVEN, START_LS = 0, 1
MAX_ITERS = 32


def _solve(d, g, w, fit_shift):
    """One solve over the pixels that count (d, g float64, w their weights) -> (s, t) | None where the fit is degenerate."""
    if d.size < 2:
        return None
    wd = w * d
    N, Sd, Sg, Sdd, Sdg = w.sum(), wd.sum(), (w * g).sum(), (wd * d).sum(), (wd * g).sum()
    with np.errstate(all="ignore"):
        if fit_shift:
            det = N * Sdd - Sd * Sd
            if not det > 1e-12 * N * N:
                return None
            s = (N * Sdg - Sd * Sg) / det
            t = (Sg - s * Sd) / N
        else:
            if not Sdd > 1e-12 * N:
                return None
            s, t = Sdg / Sdd, np.float64(0.0)
    if not (s > 0.0 and np.isfinite(s) and np.isfinite(t)):
        return None
    return float(s), float(t)


def align_fit_reference(d, ref, mask=None, fit_shift=True, iters=4, start=(1.0, 0.0), delta=0.05, reverse=False):
    """-> (s, t, flag).  ``start``: a pair (MG_ALIGN_START_GIVEN) or "ls" (MG_ALIGN_START_LS).  ``reverse``: sum in reversed pixel order."""
    d32, g32 = np.asarray(d, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    counts = np.isfinite(d32) & np.isfinite(g32)
    if mask is not None:
        counts &= np.asarray(mask).reshape(-1) != 0
    x, g = d32[counts].astype(np.float64), g32[counts].astype(np.float64)
    if reverse:
        x, g = x[::-1].copy(), g[::-1].copy()
    one = np.ones_like(x)
    coef = None
    if iters == 0 or (isinstance(start, str) and start == "ls"):
        coef = _solve(x, g, one, fit_shift)
        if coef is None:
            return 1.0, 0.0, 1
    elif iters >= 1:
        coef = (float(start[0]), float(start[1]))
    for _ in range(iters):
        with np.errstate(all="ignore"):
            r = ((coef[0] * x + coef[1]) - g) / delta
            w = 1.0 / (1.0 + r * r)
        coef = _solve(x, g, w, fit_shift)
        if coef is None:
            return 1.0, 0.0, 1
    return coef[0], coef[1], 0


def align_apply_reference(x, coef, use_shift=True, clip=None):
    """fp32 in, fp32 out: (float)((double)x * s + (t | 0)), then the clamp v < lo ? lo : (v > hi ? hi : v) where ``clip`` = (lo, hi) has
    lo <= hi."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        v = (x.astype(np.float64) * np.float64(coef[0]) + (np.float64(coef[1]) if use_shift else np.float64(0.0))).astype(np.float32)
    if clip is not None and clip[0] <= clip[1]:
        lo, hi = np.float32(clip[0]), np.float32(clip[1])
        v = np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(np.float32)
    return v


def robustness_scene(n=12293, seed=0):
    """A map that is the reference under a known scale and shift (ref = 0.8 d + 0.07, up to 1 % noise) with its first fifth disturbed -
    an object that moved: (d, ref, the true s).  Plain least squares misses s by more than 0.2, four Cauchy solves from (1, 0) with
    delta = 0.05 recover it within 0.03."""
    g = np.random.default_rng(seed)
    ref = g.random(n).astype(np.float32)
    d = ((ref.astype(np.float64) - 0.07) / 0.8 + 0.01 * g.standard_normal(n)).astype(np.float32)
    d[:n // 5] = 0.05
    return d, ref, 0.8
