"""The scenes of the view tests (tests/test_view_host.py asks the restatement whether they reach every branch; tests/test_gpu_view.py
runs them on the device): every source map of the ladder under every pose, the options rotating over the cases, each with the
restatement's result - computed once, on the CPU.  No part of the package."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from tests.test_gpu_mesh import _mask, _mesh_scene
from tests.test_gpu_points import _camera, COEF, Z_RANGE
from tests.view_reference import IDENTITY, view_reference

SHAPES = ((1, 1), (1, 7), (2, 2), (3, 5), (17, 33), (64, 67), (129, 257))
POSES = ("identity", "stereo_left", "stereo_right", "turn", "forward", "mirror", "zoom", "extreme")
TARGETS = ("equal", "smaller", "larger", "one", "wide")
MASKS = ("none", "half", "corner")
FILLS = (0, 3, 64)
OPTIONS = [(coef, edge, hwc) for coef in (None, COEF) for edge in (0.0, 0.05) for hwc in (True, False)]
Z_NEAR = 0.25
NO_SPAN = ("identity", "stereo_left", "stereo_right", "mirror")   # poses under which no face may reach the span cap on an equal target


def pose_of(name):
    """-> (the 3 x 4 pose or None, the factor on the target's focal lengths)"""
    m = IDENTITY.copy()
    if name == "identity":
        return None, 1.0
    if name in ("stereo_left", "stereo_right"):
        m[0, 3] = 0.12 if name == "stereo_left" else -0.12
    elif name == "turn":          # 0.3 rad about the vertical axis, with a shift
        c, s = math.cos(0.3), math.sin(0.3)
        m[:, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
        m[:, 3] = (-0.7, 0.05, 0.2)
    elif name == "forward":       # into the scene: what is nearer than 2.2 + Z_NEAR falls behind the near plane
        m[2, 3] = -2.2
    elif name == "mirror":
        m[0, 0] = -1.0
    elif name == "zoom":          # magnified 50 times after half a unit forward: near cells pass the span cap, far ones do not
        m[2, 3] = -0.5
        return m, 50.0
    elif name == "extreme":       # magnified a million times: corners leave the snapping range
        return None, 1.0e6
    else:
        raise ValueError(name)
    return m, 1.0


def target_of(kind, h, w, K, zoom):
    """-> ((h2, w2), the target camera): the source camera rescaled to the target's size under the pixel-centre rule, then zoomed"""
    h2, w2 = {"equal": (h, w), "smaller": (h // 2 + 1, (2 * w) // 3 + 1), "larger": (h + 5, 2 * w + 1), "one": (1, 1), "wide": (max(1, h // 3), w + 9)}[kind]
    fx, fy, cx, cy = K
    sx, sy = w2 / w, h2 / h
    return (h2, w2), (fx * sx * zoom, fy * sy * zoom, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5)


@functools.lru_cache(maxsize=None)
def cases():
    """[namespace: name, d, colors (in the option's layout), mask, K, opt = (coef, edge_rel, hwc), pose, K_out, size, fill, face (whether
    the face map is asked for), want (the restatement's result)]"""
    out, k = [], 0
    for h, w in SHAPES:
        for pose_name in POSES:
            coef, edge, hwc = opt = OPTIONS[(3 * k) % len(OPTIONS)]
            mask_kind, fill, face = MASKS[(k // 2) % len(MASKS)], FILLS[k % len(FILLS)], k % 4 != 3
            target = "equal" if pose_name == "identity" and k % 2 == 0 else TARGETS[k % len(TARGETS)]
            k += 1
            d, colors = _mesh_scene(h, w, coef)
            mask, K = _mask(mask_kind, h, w), _camera(h, w)
            pose, zoom = pose_of(pose_name)
            size, K_out = target_of(target, h, w, K, zoom)
            lay = colors if hwc else np.ascontiguousarray(colors.transpose(2, 0, 1))
            want = view_reference(d, K, lay, hwc=hwc, mask=mask, coef=coef, z_range=Z_RANGE, edge_rel=edge, pose=pose, K_out=K_out, size=size,
                                  z_near=Z_NEAR, fill_radius=fill)
            out.append(SimpleNamespace(name=f"{h}x{w}/{pose_name}/{target}/{mask_kind}/fill{fill}/{opt}", shape=(h, w), pose_name=pose_name, target=target,
                                       mask_kind=mask_kind, d=d, colors=lay, mask=mask, K=K, opt=opt, pose=pose, K_out=K_out, size=size, fill=fill,
                                       face=face, want=want))
    return out
