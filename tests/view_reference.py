"""The numpy restatement of depth to views (include/marigold_hip.h, "DEPTH TO VIEW"; csrc/view.hip), built on the restatement of the
meshes (tests/mesh_reference.py: which cells have which faces): the transform of every face's corners into the target camera, the four
reasons to drop a face, inclusive coverage in int64, the depth and the key of every offer, the winner of every pixel, its colour, the
row fill and the eight counts - float64 with every product, sum and quotient a numpy operation of its own in the order the header
writes them.  It also reports what happened on the way - why each face was dropped, which pixels saw a tie or a later face winning,
where each fill came from - so that the tests can ask whether their scenes reach every branch.  What the GPU tests are held against;
no part of the package."""
from types import SimpleNamespace

import numpy as np

from tests.mesh_reference import CANDIDATES, mesh_reference

MAX_SPAN, MAX_FILL = 64, 64
DRAWN, NEAR, OFF, BACK, SPAN = 0, 1, 2, 3, 4          # what became of a face
NO_FILL, LEFT_ONLY, RIGHT_ONLY, BOTH_LEFT, BOTH_RIGHT = 0, 1, 2, 3, 4   # where a filled pixel's value came from
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def _edge(ax, ay, bx, by, cx, cy):
    return (cx - ax) * (by - ay) - (bx - ax) * (cy - ay)


def view_reference(d, K, colors, *, hwc=True, mask=None, coef=None, z_range=(0.0, np.inf), edge_rel=0.0, pose=None, K_out=None, size=None,
                   z_near=1e-6, fill_radius=0):
    """``d`` fp32 [h, w], ``K`` = (fx, fy, cx, cy), ``colors`` uint8 [h, w, 3] (``hwc``) or [3, h, w], ``pose`` [3, 4] | None,
    ``K_out`` the target camera (default ``K``), ``size`` = (h2, w2) (default the map's) -> a namespace: ``rgb`` uint8 in the layout of
    ``colors``, ``depth`` fp32 [h2, w2], ``valid`` uint8, ``face`` int32, ``count`` (8 integers); per face, in face order: ``face_id``
    and ``fate`` (DRAWN, NEAR, OFF, BACK, SPAN); per target pixel: ``offers``, ``tie`` (the two smallest keys have the same depth),
    ``later_wins`` (the runner-up has another depth and a SMALLER face id than the winner), ``fill_kind``."""
    d = np.asarray(d, np.float32)
    h, w = d.shape
    h2, w2 = (h, w) if size is None else (int(size[0]), int(size[1]))
    fx, fy, cx, cy = (np.float64(v) for v in K)
    fx2, fy2, cx2, cy2 = (np.float64(v) for v in (K if K_out is None else K_out))
    Rt = IDENTITY if pose is None else np.asarray(pose, np.float64).reshape(3, 4)
    z_near = np.float64(z_near)
    colors = np.asarray(colors, np.uint8)
    flat = (colors.reshape(h * w, 3) if hwc else colors.reshape(3, h * w).T).astype(np.float64)
    m = mesh_reference(d, K, mask=mask, coef=coef, z_range=z_range, edge_rel=edge_rel)
    with np.errstate(all="ignore"):
        z = d.astype(np.float64)
        if coef is not None:
            z = z * np.float64(coef[0]) + np.float64(coef[1])
        # ---- the faces, row-major cells, T0 before T1 ----
        cy_, cx_, slot = np.nonzero(np.stack([m.t0, m.t1], axis=-1))
        corner = CANDIDATES[m.form[cy_, cx_], slot].reshape(-1, 3)                    # [F, 3]: A B C D as 0 1 2 3
        px, py = cx_[:, None] + (corner & 1), cy_[:, None] + (corner >> 1)
        face_id = 2 * (cy_.astype(np.int64) * w + cx_) + slot
        F = len(face_id)
        pixel = py * w + px                                                           # [F, 3]: the corners' source pixels
        Z = z[py, px]
        X, Y = ((px.astype(np.float64) - cx) * Z) / fx, ((py.astype(np.float64) - cy) * Z) / fy
        Xp, Yp, Zp = (((Rt[r, 0] * X + Rt[r, 1] * Y) + Rt[r, 2] * Z) + Rt[r, 3] for r in range(3))
        u, v, q = (fx2 * Xp) / Zp + cx2, (fy2 * Yp) / Zp + cy2, 1.0 / Zp
        # ---- dropped faces: the first reason that applies ----
        near = (~np.isfinite(Zp) | (Zp < z_near)).any(axis=1)
        off = ~near & (~(np.abs(u) <= 2.0 ** 20) | ~(np.abs(v) <= 2.0 ** 20)).any(axis=1)
        live = ~near & ~off
        xi, yi = np.zeros((F, 3), np.int64), np.zeros((F, 3), np.int64)
        xi[live], yi[live] = np.rint(256.0 * u[live]).astype(np.int64), np.rint(256.0 * v[live]).astype(np.int64)
        area = _edge(xi[:, 0], yi[:, 0], xi[:, 1], yi[:, 1], xi[:, 2], yi[:, 2])
        back = live & (area <= 0)
        live &= ~back
        x0, x1 = -((-xi.min(axis=1)) // 256), xi.max(axis=1) // 256
        y0, y1 = -((-yi.min(axis=1)) // 256), yi.max(axis=1) // 256
        span = live & ((x1 - x0 + 1 > MAX_SPAN) | (y1 - y0 + 1 > MAX_SPAN))
        live &= ~span
        fate = np.select([near, off, back, span], [NEAR, OFF, BACK, SPAN], DRAWN)
        # ---- every (face, pixel centre of its clamped box) pair ----
        x0, x1, y0, y1 = np.maximum(x0, 0), np.minimum(x1, w2 - 1), np.maximum(y0, 0), np.minimum(y1, h2 - 1)
        bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
        tests = np.where(live, bw * bh, 0)
        f = np.repeat(np.arange(F), tests)
        k = np.arange(len(f)) - np.repeat(np.cumsum(tests) - tests, tests)
        PX, PY = x0[f] + k % np.maximum(bw[f], 1), y0[f] + k // np.maximum(bw[f], 1)
        sx, sy = 256 * PX, 256 * PY
        e0 = _edge(sx, sy, xi[f, 1], yi[f, 1], xi[f, 2], yi[f, 2])
        e1 = _edge(xi[f, 0], yi[f, 0], sx, sy, xi[f, 2], yi[f, 2])
        e2 = _edge(xi[f, 0], yi[f, 0], xi[f, 1], yi[f, 1], sx, sy)
        assert np.array_equal(e0 + e1 + e2, area[f]) and (np.abs(np.stack([e0, e1, e2])) < 2 ** 30).all()
        w0, w1, w2_ = e0.astype(np.float64) * q[f, 0], e1.astype(np.float64) * q[f, 1], e2.astype(np.float64) * q[f, 2]
        s = (w0 + w1) + w2_
        zv = (area[f].astype(np.float64) / s).astype(np.float32)
        offer = (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & np.isfinite(zv) & (zv > 0)
        key = (zv.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face_id[f].astype(np.uint64)
        # ---- the smallest key of every pixel ----
        n2 = h2 * w2
        at, key_o = (PY * w2 + PX)[offer], key[offer]
        order = np.lexsort((key_o, at))
        at_s, key_s = at[order], key_o[order]
        first = np.ones(len(at_s), bool)
        first[1:] = at_s[1:] != at_s[:-1]
        win = order[first]                                                            # index into the offers: every pixel's winner
        pix = at_s[first]
        offers = np.bincount(at, minlength=n2)
        second = np.flatnonzero(first) + 1                                            # the runner-up, where the pixel has one
        has2 = offers[pix] >= 2
        tie, later_wins = np.zeros(n2, bool), np.zeros(n2, bool)
        a, b = key_s[np.flatnonzero(first)[has2]], key_s[second[has2]]
        tie[pix[has2]] = (a >> np.uint64(32)) == (b >> np.uint64(32))
        later_wins[pix[has2]] = ((a >> np.uint64(32)) != (b >> np.uint64(32))) & ((a & np.uint64(0xFFFFFFFF)) > (b & np.uint64(0xFFFFFFFF)))
        keys = np.full(n2, EMPTY)
        keys[pix] = key_o[win]
        # ---- the winner's colour ----
        g = np.flatnonzero(offer)[win]                                                # index into the pairs
        c = [flat[pixel[f[g], j]] for j in range(3)]                                  # [W, 3] each: the corners' bytes
        mix = ((w0[g, None] * c[0] + w1[g, None] * c[1]) + w2_[g, None] * c[2]) / s[g, None]
        rgb = np.zeros((n2, 3), np.uint8)
        rgb[pix] = np.minimum((mix + 0.5).astype(np.int64), 255).astype(np.uint8)
        depth = np.zeros(n2, np.float32)
        depth[pix] = zv[g]
        valid = np.zeros(n2, np.uint8)
        valid[pix] = 1
        face = np.full(n2, -1, np.int32)
        face[pix] = face_id[f[g]]
        # ---- the row fill: from pixels a face covers, never from a fill ----
        r = int(fill_radius)
        assert 0 <= r <= MAX_FILL
        covered = (valid == 1).reshape(h2, w2)
        xs = np.broadcast_to(np.arange(w2), (h2, w2))
        left, right = np.full((h2, w2), -1), np.full((h2, w2), -1)
        for k in range(1, min(r, w2 - 1) + 1):
            seen = np.zeros((h2, w2), bool)
            seen[:, k:] = covered[:, :-k]
            take = seen & (left < 0)
            left[take] = (xs - k)[take]
            seen = np.zeros((h2, w2), bool)
            seen[:, :-k] = covered[:, k:]
            take = seen & (right < 0)
            right[take] = (xs + k)[take]
        hole = ~covered
        rows = np.broadcast_to(np.arange(h2)[:, None], (h2, w2))
        depth2 = depth.reshape(h2, w2)
        dl, dr = depth2[rows, np.maximum(left, 0)], depth2[rows, np.maximum(right, 0)]
        has_l, has_r = hole & (left >= 0), hole & (right >= 0)
        use_r = has_r & (~has_l | (dr > dl))
        use_l = has_l & ~use_r
        fill_kind = np.select([use_l & ~has_r, use_r & ~has_l, use_l, use_r], [LEFT_ONLY, RIGHT_ONLY, BOTH_LEFT, BOTH_RIGHT], NO_FILL)
        src = np.where(use_r, right, left)
        filled = use_l | use_r
        take_from = (rows * w2 + src)[filled]
        to = np.flatnonzero(filled.reshape(-1))
        rgb[to], depth[to], valid[to] = rgb[take_from], depth[take_from], 2
    count = (F, int((fate == DRAWN).sum()), int(near.sum()), int(off.sum()), int(back.sum()), int(span.sum()), int((valid == 1).sum()),
             int((valid == 2).sum()))
    rgb = rgb.reshape(h2, w2, 3)
    return SimpleNamespace(rgb=rgb if hwc else np.ascontiguousarray(rgb.transpose(2, 0, 1)), depth=depth.reshape(h2, w2), valid=valid.reshape(h2, w2),
                           face=face.reshape(h2, w2), count=count, face_id=face_id, fate=fate, offers=offers.reshape(h2, w2), tie=tie.reshape(h2, w2),
                           later_wins=later_wins.reshape(h2, w2), fill_kind=fill_kind, mesh=m)
