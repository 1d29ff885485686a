"""The scenes of the focus tests (tests/test_focus_host.py asks the restatement whether they reach every branch; tests/test_gpu_focus.py
runs them on the device), each with the restatement's result - computed once per session, on the CPU.  No part of the package.

Sizes: 1 x 1, 1 x 9 and 9 x 1; one less and one more than the gather tile's edges (8 rows of 32 targets) in each direction, and the tile
itself; 20 x 24, smaller than the halo in both directions at max_radius = 32; 70 x 90 at max_radius = 32 (several tiles, every one with
a clipped halo); 129 x 257 at max_radius 8 and less (17 x 9 tiles, interior ones with a whole halo).  The general scene is the points
tests': a smooth surface with a 30 % and a 20 % step, NaN and +-inf planted, values at and just beyond the range.  The step scenes are
two flat halves, the near one on the left, with the focus on either."""
import functools
from types import SimpleNamespace

import numpy as np

from tests.focus_reference import focus_reference, LENS, LINEAR
from tests.test_gpu_points import _mask, _scene, COEF, Z_RANGE

TILE = (8, 32)   # TILE_H, TILE_W of csrc/focus.hip
OPEN = (0.0, float("inf"))


def step_scene(h, w, seed=3):
    """two flat halves, z = 2 left of the middle column and z = 4 right of it, random colours -> (d, colours [h, w, 3])"""
    d = np.where(np.arange(w) < w // 2, 2.0, 4.0).astype(np.float32) * np.ones((h, 1), np.float32)
    return d, np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _spec():
    """(kind, h, w, max_radius, space, gain, focus: ("at", y, x) | ("z", value), mask kind, coef, z_range, hwc, radius given)"""
    T, S = True, False
    th, tw = TILE
    return [
        ("scene", 1, 1, 8, LENS, 60.0, ("at", 0, 0), "none", None, OPEN, T, T),
        ("scene", 1, 1, 0, LINEAR, 5.0, ("z", 2.0), "none", None, OPEN, S, S),
        ("scene", 1, 9, 8, LENS, 400.0, ("at", 0, 4), "none", None, OPEN, S, T),
        ("scene", 9, 1, 8, LINEAR, 40.0, ("z", 2.1), "none", COEF, OPEN, T, S),
        ("scene", 1, 9, 1, LINEAR, 40.0, ("z", 2.05), "second", None, OPEN, T, T),
        # around the tile's edges
        ("scene", th - 1, tw - 1, 8, LENS, 60.0, ("at", 3, 5), "none", None, Z_RANGE, T, T),
        ("scene", th + 1, tw + 1, 8, LENS, 60.0, ("z", 2.5), "half", COEF, Z_RANGE, S, S),
        ("scene", th - 1, tw + 1, 8, LINEAR, 8.0, ("z", 2.4), "none", COEF, Z_RANGE, T, S),
        ("scene", th + 1, tw - 1, 8, LINEAR, 8.0, ("at", 0, 30), "half", None, Z_RANGE, S, T),
        ("scene", th, tw, 8, LENS, 60.0, ("z", 2.2), "none", None, OPEN, S, T),
        ("scene", th + 1, tw + 1, 1, LENS, 12.0, ("z", 2.2), "none", None, Z_RANGE, T, T),
        ("scene", th - 1, tw - 1, 0, LENS, 60.0, ("at", 2, 2), "second", COEF, Z_RANGE, S, T),
        ("scene", th + 1, tw + 1, 32, LENS, 250.0, ("at", 4, 16), "none", COEF, Z_RANGE, T, S),
        ("scene", 2 * th + 1, 2 * tw + 1, 8, LINEAR, 8.0, ("at", 16, 64), "none", COEF, Z_RANGE, T, T),
        ("scene", 2 * th + 1, 2 * tw + 1, 1, LENS, 12.0, ("at", 1, 1), "none", None, OPEN, S, S),
        # smaller than the halo in both directions
        ("scene", 20, 24, 32, LENS, 250.0, ("at", 10, 3), "none", None, Z_RANGE, T, T),
        ("scene", 20, 24, 32, LINEAR, 30.0, ("z", 2.3), "half", COEF, Z_RANGE, S, T),
        ("scene", 20, 24, 32, LENS, 2000.0, ("z", 2.0), "none", None, OPEN, S, S),          # nearly everything capped
        # several tiles at the largest radius
        ("scene", 70, 90, 32, LENS, 250.0, ("at", 20, 20), "none", COEF, Z_RANGE, T, T),
        ("scene", 70, 90, 32, LINEAR, 30.0, ("at", 60, 80), "half", None, Z_RANGE, S, S),
        ("scene", 70, 90, 32, LENS, 40.0, ("z", 3.0), "none", None, OPEN, S, T),            # small radii under a large cap
        # many tiles, whole halos
        ("scene", 129, 257, 8, LENS, 60.0, ("at", 30, 40), "none", None, Z_RANGE, T, T),
        ("scene", 129, 257, 8, LINEAR, 8.0, ("z", 2.6), "half", COEF, Z_RANGE, S, S),
        ("scene", 129, 257, 1, LENS, 12.0, ("at", 100, 200), "none", COEF, OPEN, T, S),
        ("scene", 129, 257, 0, LINEAR, 8.0, ("at", 5, 5), "none", None, Z_RANGE, S, T),
        ("scene", 129, 257, 8, LENS, 0.0, ("at", 64, 128), "none", None, Z_RANGE, T, T),    # gain 0: everything in focus
        # a bad focus: the pixel is masked out, the pixel is out of range, the distance is not finite, is zero, is behind the camera
        ("scene", 33, 40, 8, LENS, 60.0, ("at", 0, 1), "second", None, OPEN, T, T),
        ("scene", 33, 40, 8, LINEAR, 8.0, ("at", 16, 20), "none", None, (2.9, 3.0), S, T),
        ("scene", 33, 40, 8, LENS, 60.0, ("z", float("nan")), "none", COEF, Z_RANGE, T, S),
        ("scene", 33, 40, 8, LINEAR, 8.0, ("z", float("inf")), "none", None, Z_RANGE, S, T),
        ("scene", 33, 40, 8, LENS, 60.0, ("z", 0.0), "half", None, Z_RANGE, T, T),
        ("scene", 33, 40, 8, LENS, 60.0, ("z", -2.0), "none", COEF, Z_RANGE, S, S),
        ("scene", 33, 40, 8, LINEAR, 3.0, ("z", -2.0), "none", None, Z_RANGE, T, T),        # legal in linear space: everything capped
        # the step edge, the focus on the near side and on the far side
        ("step", 24, 48, 8, LENS, 30.0, ("at", 12, 4), "none", None, OPEN, T, T),
        ("step", 24, 48, 8, LENS, 30.0, ("at", 12, 44), "none", None, OPEN, T, T),
        ("step", 24, 48, 8, LINEAR, 2.5, ("z", 2.0), "none", None, OPEN, S, S),
        ("step", 24, 48, 8, LINEAR, 2.5, ("z", 4.0), "none", None, OPEN, S, T),
        ("step", 40, 70, 32, LENS, 100.0, ("at", 0, 0), "none", None, OPEN, T, S),
        ("step", 40, 70, 32, LENS, 100.0, ("at", 39, 69), "none", None, OPEN, S, T),
        ("step", 24, 48, 8, LENS, 30.0, ("z", 3.0), "none", None, OPEN, T, T),              # the focus between the two: both blurred
    ]


@functools.lru_cache(maxsize=None)
def cases():
    """[namespace: name, kind, shape, d, colors (in the case's layout), mask, coef, z_range, space, gain, max_radius, focus_at | None,
    focus | None, hwc, radius (whether the map of radii is asked for), want (the restatement's result)]"""
    out = []
    for k, (kind, h, w, R, space, gain, focus, mask_kind, coef, z_range, hwc, radius) in enumerate(_spec()):
        d, colors = _scene(h, w, coef) if kind == "scene" else step_scene(h, w)
        mask = _mask(mask_kind, h, w)
        lay = colors if hwc else np.ascontiguousarray(colors.transpose(2, 0, 1))
        focus_at, value = ((focus[1], focus[2]), None) if focus[0] == "at" else (None, focus[1])
        want = focus_reference(d, lay, hwc=hwc, mask=mask, coef=coef, z_range=z_range, space=space, gain=gain, max_radius=R, focus_at=focus_at,
                               focus=value)
        out.append(SimpleNamespace(name=f"{k}:{kind}/{h}x{w}/R{R}/space{space}/gain{gain}/{focus}/{mask_kind}/{coef}/{'hwc' if hwc else 'chw'}",
                                   kind=kind, shape=(h, w), d=d, colors=lay, mask=mask, mask_kind=mask_kind, coef=coef, z_range=z_range, space=space,
                                   gain=gain, max_radius=R, focus_at=focus_at, focus=value, hwc=hwc, radius=radius, want=want))
    return out
