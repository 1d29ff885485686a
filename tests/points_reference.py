"""The numpy float64 restatement of depth to 3D (include/marigold_hip.h, "DEPTH TO 3D"; csrc/points.hip): usable, joined and kept
pixels, points, normals and the compacted records, vectorised, every product, sum and quotient a numpy operation of its own in the
order the header writes them - numpy rounds each one, as the kernels built with -ffp-contract=off do.  What the GPU tests are held
against; no part of the package."""
from types import SimpleNamespace

import numpy as np

EAST, WEST, SOUTH, NORTH = 0, 1, 2, 3
_STEP = ((0, 1), (0, -1), (1, 0), (-1, 0))   # (dy, dx) of the neighbour
NONE, CENTRAL, HIGH_ONLY, LOW_ONLY = 0, 1, 2, 3   # the form of a tangent: no neighbour, both, east / south only, west / north only


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], ``fill`` outside the map"""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    yt, xt = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    out[ys, xs] = a[yt, xt]
    return out


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def points_reference(d, K, *, colors=None, hwc=True, mask=None, coef=None, z_range=(0.0, np.inf), edge_rel=0.0, frame="camera", capacity=None):
    """``d`` fp32 [h, w], ``K`` = (fx, fy, cx, cy), ``colors`` uint8 [h, w, 3] (``hwc``) or [3, h, w], ``mask`` [h, w], ``coef`` (s, t) ->
    a namespace: ``usable``, ``kept`` bool [h, w]; ``dense`` fp32 [3, h, w] and ``valid`` uint8 [h, w] (mg_depth_normals); the records
    ``xyz`` fp32 [written, 3], ``nrm`` fp32 [written, 3], ``rgb`` uint8 [written, 3] | None, ``index`` int32 [written]; ``count`` =
    (kept, written); ``form_u``, ``form_v`` [h, w]: the form of either tangent at kept pixels (NONE elsewhere); ``removed``: how many
    pixels each rule removes - mask, nonfinite, range, edge."""
    d = np.asarray(d, np.float32)
    h, w = d.shape
    fx, fy, cx, cy = (np.float64(v) for v in K)
    z_min, z_max = (np.float64(v) for v in z_range)
    edge_rel = np.float64(edge_rel)
    with np.errstate(all="ignore"):
        z = d.astype(np.float64)
        if coef is not None:
            z = z * np.float64(coef[0]) + np.float64(coef[1])
        in_mask = np.ones((h, w), bool) if mask is None else np.asarray(mask).reshape(h, w) != 0
        finite = np.isfinite(d) & np.isfinite(z)
        in_range = (z > z_min) & (z <= z_max)
        usable = in_mask & finite & in_range
        joined, zq = [], []
        kept = usable.copy()
        for dy, dx in _STEP:
            q_usable, q = _shift(usable, dy, dx, False), _shift(z, dy, dx, np.nan)
            j = usable & q_usable & ((edge_rel == 0.0) | (np.abs(z - q) <= edge_rel * np.minimum(z, q)))
            kept &= ~q_usable | j
            joined.append(j)
            zq.append(q)
        joined = [j & kept for j in joined]
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")

        def point(x, y, zz):
            return np.stack([((x - cx) * zz) / fx, ((y - cy) * zz) / fy, zz])

        P = point(xs, ys, z)

        def tangent(hi, lo):
            (dy, dx) = _STEP[hi]
            A = np.where(joined[hi], point(xs + dx, ys + dy, zq[hi]), P)
            B = np.where(joined[lo], point(xs - dx, ys - dy, zq[lo]), P)
            form = np.where(joined[hi] & joined[lo], CENTRAL, np.where(joined[hi], HIGH_ONLY, np.where(joined[lo], LOW_ONLY, NONE)))
            return A - B, form

        Tu, form_u = tangent(EAST, WEST)
        Tv, form_v = tangent(SOUTH, NORTH)
        N = np.stack([Tv[1] * Tu[2] - Tv[2] * Tu[1], Tv[2] * Tu[0] - Tv[0] * Tu[2], Tv[0] * Tu[1] - Tv[1] * Tu[0]])
        N = np.where(_dot(N, P) > 0.0, -N, N)
        nn = _dot(N, N)
        has = kept & (form_u != NONE) & (form_v != NONE) & (nn > 0.0) & np.isfinite(nn)
        N = N / np.sqrt(nn)
        if frame == "marigold":
            N = np.stack([N[0], -N[1], -N[2]])
        elif frame != "camera":
            raise ValueError(frame)
        dense = np.where(has, N, 0.0).astype(np.float32)
        P32 = P.astype(np.float32)
    index = np.flatnonzero(kept).astype(np.int32)
    total = len(index)
    written = total if capacity is None else min(total, int(capacity))
    index = index[:written]
    rgb = None
    if colors is not None:
        colors = np.asarray(colors, np.uint8)
        flat = colors.reshape(h * w, 3) if hwc else colors.reshape(3, h * w).T
        rgb = np.ascontiguousarray(flat[index])
    removed = dict(mask=int((~in_mask).sum()), nonfinite=int((in_mask & ~finite).sum()), range=int((in_mask & finite & ~in_range).sum()),
                   edge=int((usable & ~kept).sum()))
    return SimpleNamespace(usable=usable, kept=kept, dense=dense, valid=has.astype(np.uint8), xyz=np.ascontiguousarray(P32.reshape(3, -1).T[index]),
                           nrm=np.ascontiguousarray(dense.reshape(3, -1).T[index]), rgb=rgb, index=index, count=(total, written),
                           form_u=np.where(kept, form_u, NONE), form_v=np.where(kept, form_v, NONE), removed=removed)
