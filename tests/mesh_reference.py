"""The numpy float64 restatement of depth to mesh (include/marigold_hip.h, "DEPTH TO MESH"; csrc/mesh.hip): usable pixels, cells, their
split or three-corner form, faces, vertices, the records and the four counts, vectorised, every product, sum and quotient a numpy
operation of its own in the order the header writes them.  It also reports what each cell did - its form, whether its split was a tie,
how many faces a four-corner cell kept - so that the tests can ask whether their scenes reach every branch.  What the GPU tests are
held against; no part of the package."""
from types import SimpleNamespace

import numpy as np

from tests.points_reference import _STEP, _dot, _shift, EAST, NORTH, SOUTH, WEST

# the form of a cell: no candidate, four corners split along A-D / along B-C, or three corners with D / A / B / C missing
NO_CELL, SPLIT_AD, SPLIT_BC, NO_D, NO_A, NO_B, NO_C = -1, 0, 1, 2, 3, 4, 5
A, B, C, D = 0, 1, 2, 3
_ACD, _ADB, _ACB, _BCD = (A, C, D), (A, D, B), (A, C, B), (B, C, D)
# the candidates of every form, T0 then T1 (a three-corner form has T0 alone; the second entry is never a face)
CANDIDATES = np.array([(_ACD, _ADB), (_ACB, _BCD), (_ACB, _ACB), (_BCD, _BCD), (_ACD, _ACD), (_ADB, _ADB)])


def mesh_reference(d, K, *, colors=None, hwc=True, mask=None, coef=None, z_range=(0.0, np.inf), edge_rel=0.0, frame="camera", capacity_v=None,
                   capacity_f=None):
    """``d`` fp32 [h, w], ``K`` = (fx, fy, cx, cy), ``colors`` uint8 [h, w, 3] (``hwc``) or [3, h, w], ``mask`` [h, w], ``coef`` (s, t) ->
    a namespace: ``usable``, ``vertex``, ``has_normal`` bool [h, w]; per cell [h - 1, w - 1]: ``form``, ``tie`` (four corners and equal
    diagonal differences), ``t0``, ``t1`` (which candidates are faces), ``kept4`` (faces kept by a four-corner cell, -1 elsewhere); the
    records ``xyz`` fp32 [V_written, 3], ``nrm`` fp32 [V_written, 3], ``rgb`` uint8 [V_written, 3] | None, ``index`` int32 [V_written],
    ``faces`` int32 [F_written, 3]; ``count`` = (V, V_written, F, F_written)."""
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
        usable = in_mask & np.isfinite(d) & np.isfinite(z) & (z > z_min) & (z <= z_max)

        def joined(zp, zq):
            return (edge_rel == 0.0) | (np.abs(zp - zq) <= edge_rel * np.minimum(zp, zq))

        # ---- cells ----
        corner = (np.s_[:-1, :-1], np.s_[:-1, 1:], np.s_[1:, :-1], np.s_[1:, 1:])
        u, zc = [usable[c] for c in corner], [z[c] for c in corner]
        n_usable = u[A].astype(int) + u[B] + u[C] + u[D]
        four, three = n_usable == 4, n_usable == 3
        dad, dbc = np.abs(zc[A] - zc[D]), np.abs(zc[B] - zc[C])
        form = np.full(four.shape, NO_CELL)
        form[four & (dad <= dbc)] = SPLIT_AD
        form[four & ~(dad <= dbc)] = SPLIT_BC
        for missing, name in ((D, NO_D), (A, NO_A), (B, NO_B), (C, NO_C)):
            form[three & ~u[missing]] = name
        tie = four & (dad == dbc)
        cand = CANDIDATES[np.maximum(form, 0)]                                  # [h - 1, w - 1, 2, 3]: corners
        zs = np.stack(zc, axis=-1)[:, :, None, :].repeat(2, axis=2)            # [h - 1, w - 1, 2, 4]
        z0, z1, z2 = (np.take_along_axis(zs, cand[..., k:k + 1], axis=-1)[..., 0] for k in range(3))
        is_face = joined(z0, z1) & joined(z1, z2) & joined(z2, z0) & (form >= 0)[..., None]
        is_face[..., 1] &= four
        t0, t1 = is_face[..., 0], is_face[..., 1]
        kept4 = np.where(four, t0.astype(int) + t1, -1)
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pixel = ys * w + xs
        pix = np.stack([pixel[c] for c in corner], axis=-1)[:, :, None, :].repeat(2, axis=2)
        face_pixels = np.take_along_axis(pix, cand, axis=-1)[is_face].reshape(-1, 3)   # row-major cells, T0 before T1

        # ---- vertices ----
        vertex = np.zeros(h * w, bool)
        vertex[face_pixels.reshape(-1)] = True
        rank = np.cumsum(vertex) - 1
        vertex = vertex.reshape(h, w)
        assert not (vertex & ~usable).any()

        # ---- points and normals: 6h's rule on "usable and joined to this pixel", without the demotion of a kept pixel ----
        ysf, xsf = ys.astype(np.float64), xs.astype(np.float64)

        def point(x, y, zz):
            return np.stack([((x - cx) * zz) / fx, ((y - cy) * zz) / fy, zz])

        P = point(xsf, ysf, z)
        j4, zq = [], []
        for dy, dx in _STEP:
            q = _shift(z, dy, dx, np.nan)
            j4.append(usable & _shift(usable, dy, dx, False) & joined(z, q))
            zq.append(q)

        def tangent(hi, lo):
            (dy, dx) = _STEP[hi]
            Ta = np.where(j4[hi], point(xsf + dx, ysf + dy, zq[hi]), P)
            Tb = np.where(j4[lo], point(xsf - dx, ysf - dy, zq[lo]), P)
            return Ta - Tb, j4[hi] | j4[lo]

        Tu, has_u = tangent(EAST, WEST)
        Tv, has_v = tangent(SOUTH, NORTH)
        N = np.stack([Tv[1] * Tu[2] - Tv[2] * Tu[1], Tv[2] * Tu[0] - Tv[0] * Tu[2], Tv[0] * Tu[1] - Tv[1] * Tu[0]])
        N = np.where(_dot(N, P) > 0.0, -N, N)
        nn = _dot(N, N)
        has_normal = vertex & has_u & has_v & (nn > 0.0) & np.isfinite(nn)
        N = N / np.sqrt(nn)
        if frame == "marigold":
            N = np.stack([N[0], -N[1], -N[2]])
        elif frame != "camera":
            raise ValueError(frame)
        dense = np.where(has_normal, N, 0.0).astype(np.float32)
        P32 = P.astype(np.float32)
    index = np.flatnonzero(vertex).astype(np.int32)
    V, F = len(index), len(face_pixels)
    Vw = V if capacity_v is None else min(V, int(capacity_v))
    Fw = (F if capacity_f is None else min(F, int(capacity_f))) if V == Vw else 0
    index = index[:Vw]
    rgb = None
    if colors is not None:
        colors = np.asarray(colors, np.uint8)
        flat = colors.reshape(h * w, 3) if hwc else colors.reshape(3, h * w).T
        rgb = np.ascontiguousarray(flat[index])
    return SimpleNamespace(usable=usable, vertex=vertex, has_normal=has_normal, form=form, tie=tie, t0=t0, t1=t1, kept4=kept4,
                           xyz=np.ascontiguousarray(P32.reshape(3, -1).T[index]), nrm=np.ascontiguousarray(dense.reshape(3, -1).T[index]), rgb=rgb,
                           index=index, faces=rank[face_pixels[:Fw]].astype(np.int32).reshape(-1, 3), count=(V, Vw, F, Fw))
