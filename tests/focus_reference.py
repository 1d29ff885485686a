"""The numpy restatement of depth to focus (include/marigold_hip.h, "DEPTH TO FOCUS"; csrc/focus.hip): the blur radius in float64, every
operation a numpy operation of its own, then a loop over the (2 R + 1)^2 offsets of the window, vectorised over the pixels, with uint64
sums - on top of the usable rule tests/points_reference.py restates.  What the GPU tests are held against; no part of the package."""
from types import SimpleNamespace

import numpy as np

from tests.points_reference import points_reference

MAX_RADIUS = 32
LENS, LINEAR = 0, 1
UNUSABLE = 0xFFFF


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], ``fill`` outside the picture - for offsets larger than the picture too"""
    h, w = a.shape
    out = np.full_like(a, fill)
    if abs(dy) < h and abs(dx) < w:
        out[max(0, -dy):min(h, h - dy), max(0, -dx):min(w, w - dx)] = a[max(0, dy):min(h, h + dy), max(0, dx):min(w, w + dx)]
    return out


def disc_counts():
    """N[e], e = 0 .. 512: the integer offsets of the whole plane with 256 (dx^2 + dy^2) <= e^2"""
    off = np.arange(-MAX_RADIUS, MAX_RADIUS + 1, dtype=np.int64)
    k = 256 * (off[:, None] ** 2 + off[None, :] ** 2)
    return np.array([int((k <= e * e).sum()) for e in range(16 * MAX_RADIUS + 1)], np.int64)


N = disc_counts()
W = (1 << 24) // N


def focus_reference(d, colors, *, hwc=True, mask=None, coef=None, z_range=(0.0, np.inf), space=LENS, gain=0.0, max_radius=16, focus_at=None,
                    focus=None):
    """``d`` fp32 [h, w], ``colors`` uint8 [h, w, 3] (``hwc``) or [3, h, w], ``focus_at`` = (y, x) or ``focus`` = a distance -> a
    namespace: ``rgb`` in the layout of the colours, ``valid`` uint8 [h, w], ``radius`` uint16 [h, w], ``count`` (5 integers), and the
    report: ``front``, ``behind_q``, ``behind_p`` - the contributions of taps in front of or level with the target, and of taps behind
    it with e = r16_q and with e = r16_p < r16_q; ``no_usable``, ``no_inside``, ``no_disc`` - the rejected taps of usable targets;
    ``capped``, ``sharp``, ``unusable`` pixels; ``bad`` - None, "pixel", "nonfinite" or "behind"; ``peak_bits`` of the sums."""
    d = np.asarray(d, np.float32)
    h, w = d.shape
    R = int(max_radius)
    assert 0 <= R <= MAX_RADIUS and space in (LENS, LINEAR) and (focus_at is None) != (focus is None)
    colors = np.asarray(colors, np.uint8)
    src = colors if hwc else colors.transpose(1, 2, 0)
    usable = points_reference(d, (1.0, 1.0, 0.0, 0.0), mask=mask, coef=coef, z_range=z_range).usable
    gain = np.float64(gain)
    with np.errstate(all="ignore"):
        z = d.astype(np.float64)
        if coef is not None:
            z = z * np.float64(coef[0]) + np.float64(coef[1])
        bad = None
        if focus_at is not None:
            zf = z[focus_at]
            if not usable[focus_at]:
                bad = "pixel"
        else:
            zf = np.float64(focus)
        if bad is None and not np.isfinite(zf):
            bad = "nonfinite"
        if bad is None and space == LENS and zf <= 0.0:
            bad = "behind"
        if bad is None:
            b = gain * np.abs(1.0 / z - 1.0 / zf) if space == LENS else gain * np.abs(z - zf)
            r16 = np.where(~(b < np.float64(R)), 16 * R, np.rint(16.0 * np.where(b < np.float64(R), b, 0.0))).astype(np.int64)
        else:
            r16 = np.zeros((h, w), np.int64)
        r16 = np.where(usable, r16, 0)
        z32 = np.where(usable, z, 0.0).astype(np.float32)
    D = np.zeros((h, w), np.uint64)
    C = np.zeros((h, w, 3), np.uint64)
    report = dict(front=0, behind_q=0, behind_p=0, no_usable=0, no_inside=0, no_disc=0)
    inside_all = np.ones((h, w), bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            inside = usable & _shift(inside_all, dy, dx, False)
            q_usable = inside & _shift(usable, dy, dx, False)
            rq, zq = _shift(r16, dy, dx, 0), _shift(z32, dy, dx, np.float32(0.0))
            front = zq <= z32
            e = np.where(front, rq, np.minimum(rq, r16))
            hit = q_usable & (256 * (dx * dx + dy * dy) <= e * e)
            report["no_inside"] += int((usable & ~inside).sum())
            report["no_usable"] += int((inside & ~q_usable).sum())
            report["no_disc"] += int((q_usable & ~hit).sum())
            report["front"] += int((hit & front).sum())
            report["behind_q"] += int((hit & ~front & (rq <= r16)).sum())
            report["behind_p"] += int((hit & ~front & (rq > r16)).sum())
            wq = np.where(hit, W[e], 0).astype(np.uint64)
            D += wq
            for ch in range(3):
                C[..., ch] += wq * _shift(src[..., ch], dy, dx, 0).astype(np.uint64)
    assert (D[usable] > 0).all()                      # a usable pixel contributes to itself
    out = src.copy()
    Dsafe = np.where(usable, D, np.uint64(1))
    mixed = ((C + (Dsafe // np.uint64(2))[..., None]) // Dsafe[..., None]).astype(np.uint8)
    out[usable] = mixed[usable]
    capped = int((usable & (r16 == 16 * R)).sum()) if R > 0 else 0
    sharp = int((usable & (r16 == 0)).sum())
    taps = report["front"] + report["behind_q"] + report["behind_p"]
    count = (int(usable.sum()), sharp, capped, taps, int(bad is not None))
    return SimpleNamespace(rgb=np.ascontiguousarray(out if hwc else out.transpose(2, 0, 1)), valid=usable.astype(np.uint8),
                           radius=np.where(usable, r16, UNUSABLE).astype(np.uint16), count=count, capped=capped, sharp=sharp,
                           unusable=int((~usable).sum()), bad=bad, peak_bits=int(max(int(C.max()), 1)).bit_length(), r16=r16, usable=usable,
                           **report)
