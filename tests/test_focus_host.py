"""Host checks of depth to focus, no GPU.  The numpy restatement the GPU tests are held against has the properties the
definitions promise - no blur returns the picture, a sharp foreground is not polluted by its blurred background, a blurred foreground
bleeds over the edge - and the scenes of tests/focus_scenes.py reach every branch of it; the two C entry points are declared, bound and
exported by both operand libraries without a new op kind, and refuse bad arguments before any GPU work (no GPU is here: a call that got
as far as a launch would fail differently, so the message proves where it stopped); the command line has its flags on the depth parser
alone, refuses what it must, and writes the refocused picture through a stand-in pipeline with the restatement in the kernel's place."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import focus as F
from marigold_amd import points as P
from tests import c_hosts
from tests.focus_reference import focus_reference, LENS, LINEAR, N, W
from tests.focus_scenes import cases, step_scene, TILE
from tests.test_points_host import _FakeCliPipe, INF, NAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------

def _room(h=24, w=40):
    """a slanted wall with a near box in front of it, random colours"""
    z = (3.0 + 0.02 * np.broadcast_to(np.arange(w), (h, w))).astype(np.float32)
    z[8:16, 12:24] = 1.5
    return z, np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_the_weights():
    assert (N[0], N[15], N[16], N[512]) == (1, 1, 5, 3209) and W[0] == 1 << 24 and W.min() == W[512] == 5228 and len(W) == 513
    assert (np.diff(N) >= 0).all() and 4225 * (1 << 24) * 255 < 1 << 45


def test_no_blur_returns_the_picture():
    z, colors = _room()
    for hwc in (True, False):
        lay = colors if hwc else np.ascontiguousarray(colors.transpose(2, 0, 1))
        for kw in (dict(gain=0.0, max_radius=8), dict(gain=50.0, max_radius=0)):
            for space in (LENS, LINEAR):
                r = focus_reference(z, lay, hwc=hwc, space=space, focus=2.0, **kw)
                assert np.array_equal(r.rgb, lay) and r.count == (z.size, z.size, 0, z.size, 0) and not r.radius.any()
    flat = np.full((9, 11), 2.5, np.float32)       # a constant depth, in focus: by pixel and by value
    for kw in (dict(focus_at=(4, 4)), dict(focus=2.5)):
        r = focus_reference(flat, colors[:9, :11], space=LENS, gain=500.0, max_radius=32, **kw)
        assert np.array_equal(r.rgb, colors[:9, :11]) and r.sharp == 99 and r.capped == 0
    r = focus_reference(flat, colors[:9, :11], space=LENS, gain=500.0, max_radius=32, focus=2.0)   # out of focus: it is blurred
    assert not np.array_equal(r.rgb, colors[:9, :11]) and r.capped == 99 and r.count[3] == 99 * 99 and r.peak_bits <= 45


def test_a_constant_colour_stays_constant():
    z, _ = _room()
    z[3, 3], z[4, 30] = np.nan, np.inf
    colors = np.empty(z.shape + (3,), np.uint8)
    colors[:] = (200, 3, 255)
    for space, gain, R in ((LENS, 40.0, 8), (LINEAR, 9.0, 32), (LENS, 1e6, 32), (LINEAR, 0.9, 1)):
        r = focus_reference(z, colors, space=space, gain=gain, max_radius=R, focus=2.0, z_range=(1.0, 3.5))
        assert np.array_equal(r.rgb, colors) and r.count[3] > r.count[0] and 0 < r.unusable == (r.valid == 0).sum()


def test_a_sharp_foreground_is_not_polluted_and_a_blurred_one_bleeds():
    d, colors = step_scene(24, 48)
    near, far = np.s_[:, :24], np.s_[:, 24:]
    other = colors.copy()
    other[far] = 255 - other[far]
    for kw in (dict(space=LENS, gain=30.0), dict(space=LINEAR, gain=3.0)):
        a = focus_reference(d, colors, max_radius=8, focus_at=(12, 4), **kw)       # the focus on the near side
        b = focus_reference(d, other, max_radius=8, focus_at=(12, 4), **kw)
        assert np.array_equal(a.rgb[near], colors[near]) and np.array_equal(b.rgb[near], colors[near])   # no near byte depends on the far colours
        assert not np.array_equal(a.rgb[far], colors[far]) and a.behind_q == a.behind_p == 0 and (a.r16[near] == 0).all() and (a.r16[far] > 16).all()
        a = focus_reference(d, colors, max_radius=8, focus_at=(12, 44), **kw)      # the focus on the far side
        b = focus_reference(d, other, max_radius=8, focus_at=(12, 44), **kw)
        assert (a.r16[far] == 0).all() and (a.r16[near] > 16).all()
        assert not np.array_equal(a.rgb[:, 24:28], colors[:, 24:28])                # the near side bleeds over the edge
        assert np.array_equal(a.rgb[:, 34:], colors[:, 34:])                        # and no farther than its radius
        lit = colors.copy()
        lit[near] = 255 - lit[near]
        assert not np.array_equal(focus_reference(d, lit, max_radius=8, focus_at=(12, 44), **kw).rgb[:, 24:28], a.rgb[:, 24:28])


def test_the_scenes_reach_every_branch():
    cs = cases()
    assert 35 <= len(cs) <= 45
    for bucket in ("front", "behind_q", "behind_p", "no_usable", "no_inside", "no_disc", "capped", "sharp", "unusable"):
        assert sum(getattr(c.want, bucket) for c in cs) > 0, bucket
    assert {c.want.bad for c in cs} == {None, "pixel", "nonfinite", "behind"}
    assert sum(c.want.bad == "pixel" for c in cs) >= 2                              # masked out, and cut out by the range
    assert {c.max_radius for c in cs} == {0, 1, 8, 32} and {c.space for c in cs} == {LENS, LINEAR} and {c.hwc for c in cs} == {True, False}
    assert {c.radius for c in cs} == {True, False} and {c.coef is None for c in cs} == {True, False} and {c.mask is None for c in cs} == {True, False}
    assert {c.focus_at is None for c in cs} == {True, False}
    th, tw = TILE
    shapes = {c.shape for c in cs}
    assert {(1, 1), (1, 9), (9, 1), (th - 1, tw - 1), (th + 1, tw + 1), (th - 1, tw + 1), (th + 1, tw - 1), (129, 257)} <= shapes
    assert any(c.max_radius == 32 and c.shape[0] < 32 and c.shape[1] < 32 for c in cs)
    assert all(c.shape[0] * c.shape[1] <= 70 * 90 for c in cs if c.max_radius == 32) and all(c.max_radius <= 8 for c in cs if c.shape == (129, 257))
    src = open(os.path.join(ROOT, "marigold_amd", "csrc", "focus.hip")).read()
    assert re.search(r"TILE_W = %d, TILE_H = %d;" % (tw, th), src)                  # the sizes straddle the kernel's tile
    assert any(np.isnan(c.d).any() and np.isinf(c.d).any() for c in cs) and any(c.z_range[0] > 0 and c.want.unusable > 0 for c in cs)
    steps = [c for c in cs if c.kind == "step" and c.want.bad is None]
    assert any((c.want.r16[:, 0] == 0).all() for c in steps) and any((c.want.r16[:, -1] == 0).all() for c in steps)
    for c in cs:
        w = c.want
        assert w.count[0] == w.valid.sum() and w.count[3] == w.front + w.behind_q + w.behind_p >= w.count[0] and w.peak_bits <= 45, c.name
        assert ((w.radius == 0xFFFF) == (w.valid == 0)).all() and w.count[1] == (w.radius == 0).sum(), c.name
        lay = c.colors if c.hwc else c.colors.transpose(1, 2, 0)
        got = w.rgb if c.hwc else w.rgb.transpose(1, 2, 0)
        assert np.array_equal(got[w.valid == 0], lay[w.valid == 0]), c.name          # a pixel that is not usable keeps its bytes
        if w.bad is not None or c.max_radius == 0 or c.gain == 0.0:
            assert np.array_equal(w.rgb, c.colors) and w.count[1] == w.count[0] == w.count[3] and w.count[2] == 0, c.name
        assert w.count[4] == (w.bad is not None), c.name


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "long long mg_depth_focus_workspace_bytes(long long n);" in flat
    assert ("int mg_depth_focus(const float* d, const unsigned char* colors, int hwc, const unsigned char* mask_or_null, "
            "const double* coef_or_null, int h, int w, double z_min, double z_max, int space, double gain, int max_radius, int focus_x, "
            "int focus_y, double z_focus, unsigned char* rgb, unsigned char* valid, unsigned short* radius_or_null, long long* count, "
            "void* ws, long long ws_bytes, void* stream);") in flat
    assert "DEPTH TO FOCUS" in hdr and "b = gain * fabs(1.0 / z - 1.0 / zf)" in flat and "256 * (dx * dx + dy * dy) <= e * e" in flat
    assert re.search(r"#define MG_FOCUS_MAX_RADIUS 32\b", hdr) and L.FOCUS_MAX_RADIUS == 32 and L.FOCUS_SPACE == {"lens": 0, "linear": 1}
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfocus\.hip\b", makefile, re.M)
    assert re.search(r"^FLAGS_focus\s*:=\s*-ffp-contract=off\s*$", makefile, re.M)
    assert re.search(r"^.*\$\(BUILD\)/focus\.o.*: depth3d\.h$", makefile, re.M)
    src = open(os.path.join(ROOT, "marigold_amd", "csrc", "focus.hip")).read()
    assert '#include "depth3d.h"' in src                                            # one copy of the usable rule
    assert not re.search(r"\b(depth_at|load_coef|check_common)\([^;{]*\)\s*\{", src)
    assert "asm" not in src and "atomicCAS" not in src and "cooperative" not in src and not re.search(r"atomicAdd\(\s*\(?\s*(float|double)", src)
    assert "hipMemcpy" not in src                                                   # the weights are not uploaded
    vp, i, ll, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_depth_focus_workspace_bytes", "mg_depth_focus"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_depth_focus_workspace_bytes.argtypes == [ll] and lib.mg_depth_focus_workspace_bytes.restype is ll
        assert lib.mg_depth_focus.argtypes == [vp, vp, i, vp, vp, i, i, dbl, dbl, i, dbl, i, i, i, dbl] + [vp] * 5 + [ll, vp]
    assert len(L.OP_NAMES) == 35 and ctypes.sizeof(L.MgOp) == 360   # a plain C call, no op kind
    assert not any("focus" in name for name in L.OP_NAMES.values())
    import marigold_amd
    for name in ("HostRefocus", "Refocus", "refocus"):
        assert getattr(marigold_amd, name) is getattr(F, name)
    from marigold_amd import view as V
    assert F.write_ppm is V.write_ppm


@LIBS
def test_workspace_bytes(f16):
    lib = L.load(f16)
    for n in (0, -1, -(1 << 40), (1 << 30) + 1):
        assert lib.mg_depth_focus_workspace_bytes(n) == -1
        assert lib.mg_last_error().decode().startswith("mg_depth_focus_workspace_bytes:")
    sizes = [1, 2, 3, 7, 8, 9, 63, 64, 65, 2049, 12319, 768 * 768, 3000 * 4000, 1 << 30]
    # (float)z and r16 per pixel, each array rounded up to 16 bytes
    assert [lib.mg_depth_focus_workspace_bytes(n) for n in sizes] == [(4 * n + 15) // 16 * 16 + (2 * n + 15) // 16 * 16 for n in sizes]


_FOCUS = ("d", "colors", "hwc", "mask", "coef", "h", "w", "z_min", "z_max", "space", "gain", "max_radius", "focus_x", "focus_y", "z_focus", "rgb",
          "valid", "radius", "count", "ws", "ws_bytes")


@LIBS
def test_the_focus_call_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()                      # stands for every device buffer: no call gets as far as reading it
    p = (ctypes.addressof(mem) + 15) // 16 * 16
    need = lib.mg_depth_focus_workspace_bytes(100)

    def call(**kw):
        a = dict(d=p, colors=p, hwc=1, mask=None, coef=None, h=10, w=10, z_min=0.0, z_max=INF, space=0, gain=10.0, max_radius=8, focus_x=3, focus_y=9,
                 z_focus=0.0, rgb=p, valid=p, radius=p, count=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.mg_depth_focus(*(a[k] for k in _FOCUS), None), lib.mg_last_error().decode()

    def refused(*words, **kw):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("mg_depth_focus:") and all(w in msg for w in words), (kw, rc, msg)

    for name in ("d", "colors", "rgb", "valid", "count", "ws"):
        refused("null pointer", **{name: None})
    for kw in (dict(h=0), dict(w=-3), dict(h=32769, w=32769)):
        refused("1 to 2^30 pixels", **kw)
    for kw in (dict(z_min=-0.5), dict(z_min=NAN), dict(z_min=INF)):     # (lens space or not: a usable z is > 0)
        refused("z_min", **kw)
        refused("z_min", space=1, **kw)
    for kw in (dict(z_max=NAN), dict(z_min=1.0, z_max=1.0), dict(z_min=2.0, z_max=1.0)):
        refused("z_max", **kw)
    for bad in (-1, 2, 7):
        refused("unknown space", space=bad)
    for bad in (-1.0, NAN, INF, -INF):
        refused("gain", gain=bad)
    for bad in (-1, 33, 1 << 20):
        refused("max_radius", max_radius=bad)
    for kw in (dict(focus_x=-1), dict(focus_y=-1), dict(focus_x=-2, focus_y=-2), dict(focus_x=-1, focus_y=-2), dict(focus_x=-7, focus_y=3)):
        refused("neither a pixel nor (-1, -1)", **kw)
    for kw in (dict(focus_x=10), dict(focus_y=10), dict(focus_x=1 << 20, focus_y=1 << 20)):
        refused("outside the picture", **kw)
    for kw in (dict(d=p + 2), dict(radius=p + 1), dict(count=p + 4), dict(coef=p + 4)):
        refused("aligned to their elements", **kw)
    refused("16-byte aligned", ws=p + 8)
    refused("workspace holds", ws_bytes=need - 1)
    refused("workspace holds", ws_bytes=0)
    refused("workspace holds", ws_bytes=lib.mg_depth_focus_workspace_bytes(96))
    assert list(mem) == [0.0] * 64


# ---- marigold_amd.focus on the host ------------------------------------------------------------------------------------------------

def test_the_python_call_refuses_what_is_not_a_device_map(tmp_path):
    d = torch.zeros(4, 5)
    colors = torch.zeros(4, 5, 3, dtype=torch.uint8)
    for bad in (d, d.numpy(), None):
        with pytest.raises(ValueError, match="refocus: depth"):
            F.refocus(bad, colors, focus=2.0, gain=1.0)
    # each bad argument has its own refusal, which does not wait for a device
    for word, bad in (("exactly one of focus and focus_at", dict(focus=2.0, focus_at=(1, 1), gain=1.0)), ("exactly one of focus and focus_at", dict(gain=1.0)),
                      ("either gain, or K with aperture", dict(focus=2.0)), ("gain must be finite", dict(focus=2.0, gain=-1.0)),
                      ("gain must be finite", dict(focus=2.0, gain=float("inf"))), ("gain must be finite", dict(focus=2.0, gain=NAN)),
                      ("gain must be a number", dict(focus=2.0, gain="1")), ("max_radius", dict(focus=2.0, gain=1.0, max_radius=33)),
                      ("max_radius", dict(focus=2.0, gain=1.0, max_radius=-1)), ("max_radius", dict(focus=2.0, gain=1.0, max_radius=2.0)),
                      ("max_radius", dict(focus=2.0, gain=1.0, max_radius=True)), ("space must be", dict(focus=2.0, gain=1.0, space="log")),
                      ("focus_at must be", dict(focus_at=(0, -1), gain=1.0)), ("focus_at must be", dict(focus_at=(0.5, 1), gain=1.0)),
                      ("focus_at must be", dict(focus_at=3, gain=1.0)), ("focus_at must be", dict(focus_at=(1, 2, 3), gain=1.0)),
                      ("focus must be a number", dict(focus="near", gain=1.0)),
                      ("either gain, or K with aperture", dict(focus=2.0, gain=1.0, K=(1.0, 1.0, 0.0, 0.0), aperture=1.0)),
                      ("either gain, or K with aperture", dict(focus=2.0, K=(1.0, 1.0, 0.0, 0.0))), ("either gain, or K with aperture", dict(focus=2.0, aperture=1.0)),
                      ("K must be Intrinsics", dict(focus=2.0, K=(1.0, 1.0), aperture=1.0)), ("aperture must be a number", dict(focus=2.0, K=(1.0, 1.0, 0.0, 0.0), aperture="wide")),
                      ("thin lens", dict(focus=2.0, K=(1.0, 1.0, 0.0, 0.0), aperture=1.0, space="linear"))):
        with pytest.raises(ValueError, match="refocus: .*" + re.escape(word)):
            F.refocus(d, colors, **bad)
    with pytest.raises(ValueError, match="refocus: depth"):      # and a good set of them gets as far as the map
        F.refocus(d, colors, focus_at=(1, 1), K=P.Intrinsics(1.0, 1.0, 0.0, 0.0), aperture=1.0, max_radius=32)
    assert F.COUNT_NAMES == ("usable", "sharp", "capped", "contributions", "bad_focus") and F.SPACES == ("lens", "linear")
    rgb = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    F.HostRefocus(rgb, None, None, {}).write_ppm(tmp_path / "a.ppm")
    assert open(tmp_path / "a.ppm", "rb").read() == b"P6\n4 2\n255\n" + rgb.tobytes()


# ---- the command line --------------------------------------------------------------------------------------------------------------

def test_the_parser_flags():
    from marigold_amd import cli
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    a = cli.build_parser("depth").parse_args(io)
    assert (a.save_refocus, a.refocus_at, a.refocus_distance, a.refocus_aperture, a.refocus_max_radius) == (False, "0.5,0.5", None, 0.1, 16)
    a = cli.build_parser("depth").parse_args(io + ["--save_refocus", "--fov_deg", "60", "--refocus_at", "0.25,0.75", "--refocus_distance", "3",
                                                   "--refocus_aperture", "0.3", "--refocus_max_radius", "32"])
    assert (a.save_refocus, a.refocus_at, a.refocus_distance, a.refocus_aperture, a.refocus_max_radius, a.save_stereo) == \
        (True, "0.25,0.75", 3.0, 0.3, 32, False)
    text = re.sub(r"\s+", " ", cli.build_parser("depth").format_help())
    assert text.count("No measurement stands behind the default") == 2              # both defaults say so
    for kind in ("normals", "iid"):
        for flag in (["--save_refocus"], ["--refocus_at", "0,0"], ["--refocus_distance", "1"], ["--refocus_aperture", "1"],
                     ["--refocus_max_radius", "1"]):
            with pytest.raises(SystemExit):
                cli.build_parser(kind).parse_args(io + flag)
        assert "refocus" not in cli.build_parser(kind).format_help()
    for kind in ("depth", "normals", "iid"):   # the launchers reach the flags through cli.main and do not name them
        src = open(os.path.join(ROOT, "script", kind, "run.py")).read()
        assert "refocus" not in src and "cli" in src


class _Host(F.HostRefocus):
    __slots__ = ()

    def to_host(self):
        return self


def _restated_refocus(calls):
    """``refocus`` with the restatement in the kernel's place: host tensors in, a host picture out"""
    def fake(depth, colors, *, focus=None, focus_at=None, K=None, aperture=None, max_radius=16, coef=None):
        calls.append(dict(K=K, coef=coef, focus=focus, focus_at=focus_at, aperture=aperture, max_radius=max_radius, colors=tuple(colors.shape)))
        r = focus_reference(depth.numpy(), colors.numpy(), hwc=False, coef=coef, space=LENS, gain=0.5 * K.fx * aperture, max_radius=max_radius,
                            focus=focus, focus_at=focus_at)
        return _Host(r.rgb.transpose(1, 2, 0), r.valid, None, dict(zip(F.COUNT_NAMES, r.count)))
    return fake


def test_cli_main_writes_the_refocused_picture(tmp_path, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    g = np.random.default_rng(1)
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(g.integers(0, 256, (6, 8, 3), dtype=np.uint8)).save(inp / "b.png")      # the map's size
    Image.fromarray(g.integers(0, 256, (12, 16, 3), dtype=np.uint8)).save(inp / "a.png")    # twice the map's size
    out = tmp_path / "out"
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(out)]
    calls = []
    monkeypatch.setattr(F, "refocus", _restated_refocus(calls))
    pipe = _FakeCliPipe()
    assert cli.main("depth", base, pipeline=pipe) == 0                                      # without the flag: no folder, no call
    assert calls == [] and sorted(os.listdir(out)) == ["depth_bw", "depth_colored", "depth_npy"]
    depth = pipe._out().depth_np
    small = P.intrinsics_from_fov(6, 8, 60.0)
    for extra, video in ((["--maps_in_flight", "2"], False), (["--sequence"], True)):
        del calls[:]
        pipe = _FakeCliPipe()
        argv = base + extra + ["--save_refocus", "--fov_deg", "60", "--points_near", "2", "--points_far", "6", "--refocus_at", "0.5,0.99",
                               "--refocus_aperture", "4", "--refocus_max_radius", "3"]
        assert cli.main("depth", argv, pipeline=pipe) == 0
        assert pipe.calls[0][0] == ("map_video" if video else "map_images") and "refocus" not in " ".join(pipe.calls[0][2])
        assert sorted(os.listdir(out / "depth_refocus")) == ["a_refocus.png", "b_refocus.png"]
        assert len(calls) == 2 and all(c["colors"] == (3, 6, 8) and c["coef"] == (4.0, 2.0) and c["aperture"] == 4.0 and c["max_radius"] == 3
                                       and c["focus"] is None and c["focus_at"] == (3, 7) for c in calls)
        big = P.intrinsics_from_fov(12, 16, 60.0)
        assert calls[0]["K"] == P.scale_intrinsics(big, (12, 16), (6, 8)) and calls[1]["K"] == small   # (sorted: a.png first)
    b = np.array(Image.open(inp / "b.png"))
    got = np.array(Image.open(out / "depth_refocus" / "b_refocus.png"))
    want = focus_reference(depth, b, coef=(4.0, 2.0), space=LENS, gain=0.5 * small.fx * 4.0, max_radius=3, focus_at=(3, 7))
    assert got.shape == (6, 8, 3) and np.array_equal(got, want.rgb) and want.bad is None    # at the map's size
    assert not np.array_equal(got, b) and want.count[3] > want.count[0] == 48
    del calls[:]
    assert cli.main("depth", base + ["--save_refocus", "--focal_px", "9", "--refocus_distance", "2.5", "--refocus_at", "0,0"], pipeline=pipe) == 0
    assert calls[1] == dict(K=P.Intrinsics(9.0, 9.0, 3.5, 2.5), coef=(9.0, 1.0), focus=2.5, focus_at=None, aperture=0.1, max_radius=16, colors=(3, 6, 8))


def test_cli_refusals(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / "a.png")
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    calls = []
    monkeypatch.setattr(F, "refocus", _restated_refocus(calls))
    pipe = _FakeCliPipe()
    with pytest.raises(ValueError, match="--save_refocus cannot be combined with --tile_size"):
        cli.main("depth", base + ["--save_refocus", "--fov_deg", "60", "--tile_size", "64"], pipeline=pipe)
    ok = ["--save_refocus", "--fov_deg", "60"]
    for extra, word in ((["--save_refocus"], "exactly one of"), (ok + ["--focal_px", "100"], "exactly one of"),
                        (["--save_refocus", "--fov_deg", "180"], "--fov_deg"), (ok + ["--points_near", "3", "--points_far", "2"], "near < far"),
                        (ok + ["--refocus_at", "0.5"], "--refocus_at"), (ok + ["--refocus_at", "0.5,1.5"], "--refocus_at"),
                        (ok + ["--refocus_at", "a,b"], "--refocus_at"), (ok + ["--refocus_at", "nan,0"], "--refocus_at"),
                        (ok + ["--refocus_distance", "0"], "--refocus_distance"), (ok + ["--refocus_distance", "inf"], "--refocus_distance"),
                        (ok + ["--refocus_aperture", "-1"], "--refocus_aperture"), (ok + ["--refocus_aperture", "nan"], "--refocus_aperture"),
                        (ok + ["--refocus_max_radius", "33"], "--refocus_max_radius"), (ok + ["--refocus_max_radius", "-1"], "--refocus_max_radius")):
        with pytest.raises(SystemExit) as e:
            cli.main("depth", base + extra, pipeline=pipe)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert pipe.calls == [] and calls == []
    # without --save_refocus its flags pass unseen
    assert cli.main("depth", base + ["--refocus_max_radius", "99", "--tile_size", "64"], pipeline=pipe) == 0 and calls == []
    assert cli.main("depth", base + ok + ["--refocus_at", "1,1"], pipeline=pipe) == 0 and calls[0]["focus_at"] == (5, 7)


# ---- the C host example ------------------------------------------------------------------------------------------------------------

def test_the_c_host_example_compiles(tmp_path):
    c_hosts.compile_only(os.path.join(ROOT, "examples", "host_focus.cpp"), tmp_path / "host_focus.o")
    assert os.path.getsize(tmp_path / "host_focus.o") > 0
    assert "host_focus" in open(os.path.join(ROOT, "README.md")).read()
