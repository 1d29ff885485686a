"""Host checks of depth to views, no GPU.  The numpy restatement the GPU tests are held against has the properties the
definitions promise - an identity view is the picture and the map - and the scenes of tests/view_scenes.py reach every branch of it;
the two C entry points are declared, bound and exported by both operand libraries without a new op kind, and refuse bad arguments
before any GPU work (no GPU is here: a call that got as far as a launch would fail differently, so the message proves where it
stopped); the cell rules have one copy; the command line has its flags on the depth parser alone, refuses what it must, and writes the
stereo picture through a stand-in pipeline with the restatement in the kernel's place."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import points as P
from marigold_amd import view as V
from tests import c_hosts
from tests.test_points_host import _FakeCliPipe, _SHARED, INF, NAN
from tests.view_reference import (BACK, BOTH_LEFT, BOTH_RIGHT, DRAWN, IDENTITY, LEFT_ONLY, NEAR, NO_FILL, OFF, RIGHT_ONLY, SPAN,
                                  view_reference)
from tests.view_scenes import cases, NO_SPAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------

def _wall():
    """a slanted wall of 24 x 40 with a near box in front of it, random colours"""
    h, w = 24, 40
    xs = np.broadcast_to(np.arange(w), (h, w))
    z = (3.0 + 0.02 * xs).astype(np.float32)
    z[8:16, 12:24] = 1.5
    return z, (40.0, 40.0, 19.5, 11.5), np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ulps(a, b):
    a, b = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(a - b)


def test_an_identity_view_is_the_picture_and_the_map():
    z, K, colors = _wall()
    for edge in (0.0, 0.05):
        for hwc in (True, False):
            lay = colors if hwc else np.ascontiguousarray(colors.transpose(2, 0, 1))
            r = view_reference(z, K, lay, hwc=hwc, edge_rel=edge)
            assert (r.valid == 1).all() and np.array_equal(r.rgb, lay)             # every pixel covered, the last row and column too
            assert _ulps(r.depth, z).max() <= 1
            assert r.count[0] == r.count[1] == len(r.fate) and r.count[2:6] == (0, 0, 0, 0) and r.count[6:] == (z.size, 0)
            assert r.tie.sum() > z.size // 2 and (r.offers >= 1).all()              # equal-depth offers at the vertices, decided by the id
            # the lowest face id of those that touch the pixel
            assert r.face[0, 0] == 0 and (r.face >= 0).all()
    assert view_reference(z, K, colors, edge_rel=0.05).count[0] == 1718             # the box's rim has no faces
    assert view_reference(z, K, colors, edge_rel=0.0).count[0] == 2 * 23 * 39


def test_the_stereo_shift_the_mirror_and_the_zoom_of_the_wall():
    z, K, colors = _wall()
    left = IDENTITY.copy()
    left[0, 3] = 0.1
    r = view_reference(z, K, colors, edge_rel=0.05, pose=left)
    assert r.count[5] == 0 and r.count[1] == r.count[0] and 800 < r.count[6] < 960 and r.count[7] == 0
    holes = r.valid == 0
    assert holes.any() and (r.depth[holes] == 0).all() and (r.rgb[holes] == 0).all() and (r.face[holes] == -1).all()
    f = view_reference(z, K, colors, edge_rel=0.05, pose=left, fill_radius=3)
    assert np.array_equal(f.valid == 1, r.valid == 1) and np.array_equal(f.face, r.face)        # a fill covers nothing
    assert f.count[7] == (f.valid == 2).sum() > 0 and np.array_equal(f.depth[f.valid == 1], r.depth[r.valid == 1])
    mirror = IDENTITY.copy()
    mirror[0, 0] = -1.0
    m = view_reference(z, K, colors, edge_rel=0.05, pose=mirror)
    assert m.count == (1718, 0, 0, 0, 1718, 0, 0, 0) and (m.fate == BACK).all() and not m.valid.any()
    zoom = view_reference(z, K, colors, edge_rel=0.05, K_out=(70 * 40.0, 70 * 40.0, 19.5, 11.5))
    assert zoom.count[5] == zoom.count[0] and zoom.count[1] == 0                                # every cell is 70 pixels wide
    assert view_reference(z[:1], K, colors[:1]).count == (0,) * 8                               # h == 1: no cells
    assert not view_reference(z[:1], K, colors[:1], fill_radius=64).valid.any()


def test_a_fill_takes_the_farther_side_and_leaves_wide_holes_open():
    """two strips of wall with a gap of masked columns between them: the gap has no faces; its pixels are filled from the left strip,
    from the right strip, or from the farther of the two, and where the gap is wider than 2 r its middle stays open"""
    h, w = 4, 30
    z = np.full((h, w), 2.0, np.float32)
    z[:, 18:] = 3.0                       # the right strip is the background
    mask = np.ones((h, w), np.uint8)
    mask[:, 10:18] = 0                    # columns 10 .. 17: no faces touch 10 .. 17, and the cells 9 and 17 go with them
    K = (30.0, 30.0, 14.5, 1.5)
    colors = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    bare = view_reference(z, K, colors, mask=mask)
    assert not bare.valid[:, 10:18].any() and bare.valid[:, :10].all() and bare.valid[:, 18:].all()
    r = view_reference(z, K, colors, mask=mask, fill_radius=3)
    assert r.valid[0].tolist() == [1] * 10 + [2] * 3 + [0] * 2 + [2] * 3 + [1] * 12      # 8 wide > 2 r = 6: the middle stays open
    assert (r.fill_kind[:, 10:13] == LEFT_ONLY).all() and (r.fill_kind[:, 15:18] == RIGHT_ONLY).all() and (r.fill_kind[:, 13:15] == NO_FILL).all()
    assert (r.depth[:, 10:13] == r.depth[:, 9:10]).all() and (r.rgb[:, 15:18] == r.rgb[:, 18:19]).all()
    r = view_reference(z, K, colors, mask=mask, fill_radius=8)
    assert (r.valid[:, 10:18] == 2).all() and (r.fill_kind[:, 10:18] == BOTH_RIGHT).all() and (r.depth[:, 10:18] == 3.0).all()
    assert (r.rgb[:, 10:18] == r.rgb[:, 18:19]).all() and (r.face[:, 10:18] == -1).all() and r.count[7] == 8 * h
    flat = view_reference(np.full((h, w), 2.0, np.float32), K, colors, mask=mask, fill_radius=8)
    assert (flat.fill_kind[:, 10:18] == BOTH_LEFT).all() and (flat.rgb[:, 10:18] == flat.rgb[:, 9:10]).all()   # equal depth: the left
    near_right = view_reference(np.where(np.arange(w) >= 18, 1.5, 2.0).astype(np.float32) * np.ones((h, 1), np.float32), K, colors, mask=mask,
                                fill_radius=8)
    assert (near_right.fill_kind[:, 10:18] == BOTH_LEFT).all() and (near_right.depth[:, 10:18] == 2.0).all()


def test_the_scenes_reach_every_branch():
    cs = cases()
    assert {c.opt for c in cs} == {(coef, edge, hwc) for coef in (None, (1.25, -0.5)) for edge in (0.0, 0.05) for hwc in (True, False)}
    for fate in (DRAWN, NEAR, OFF, BACK, SPAN):
        assert sum(int((c.want.fate == fate).sum()) for c in cs) > 100, fate
    assert any(c.want.later_wins.any() for c in cs)                     # two depths, and the later face is the nearer one
    assert sum(int(c.want.tie.sum()) for c in cs) > 1000               # equal fp32 depth: the face id decides
    assert any((c.want.offers >= 2).any() and not c.want.tie.all() for c in cs)
    for kind in (LEFT_ONLY, RIGHT_ONLY, BOTH_LEFT, BOTH_RIGHT):
        assert sum(int((c.want.fill_kind == kind).sum()) for c in cs) > 10, kind
    assert any(c.fill > 0 and c.want.count[6] > 0 and (c.want.valid == 0).any() for c in cs)      # a hole wider than the fill stays open
    assert any(c.fill == 0 and c.want.count[6] > 0 and (c.want.valid == 0).any() for c in cs)     # a hole, unfilled
    assert all(c.want.count == (0,) * 8 and not c.want.valid.any() for c in cs if c.shape[0] == 1)   # no cells
    assert {c.target for c in cs} == {"equal", "smaller", "larger", "one", "wide"} and {c.fill for c in cs} == {0, 3, 64}
    assert {c.face for c in cs} == {True, False} and {c.mask_kind for c in cs} == {"none", "half", "corner"}
    for c in cs:
        w = c.want
        assert w.count[0] == sum(w.count[1:6]) == len(w.fate) == w.mesh.count[2], c.name
        assert w.count[6] == (w.valid == 1).sum() and w.count[7] == (w.valid == 2).sum(), c.name
        assert ((w.face >= 0) == (w.valid == 1)).all() and (w.depth[w.valid == 0] == 0).all() and (w.depth[w.valid != 0] > 0).all(), c.name
        if c.pose_name in NO_SPAN:
            assert w.count[5] == 0, c.name
        if c.fill == 0:
            assert w.count[7] == 0, c.name
        if c.pose_name == "mirror":
            assert w.count[4] == w.count[0], c.name
        if c.pose_name == "identity" and c.target == "equal" and c.mask is None and c.fill == 0:
            seen = w.valid == 1
            lay = c.colors if c.opt[2] else c.colors.transpose(1, 2, 0)
            got = w.rgb if c.opt[2] else w.rgb.transpose(1, 2, 0)
            assert np.array_equal(got[seen], lay[seen]) and w.count[6] == w.mesh.count[0], c.name   # every vertex is seen, as its own byte


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "long long mg_depth_view_workspace_bytes(long long n2);" in flat
    assert ("int mg_depth_view(const float* d, const unsigned char* colors, int hwc, const unsigned char* mask_or_null, "
            "const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy, double z_min, double z_max, "
            "double edge_rel, const double* pose_or_null, double fx2, double fy2, double cx2, double cy2, int h2, int w2, double z_near, "
            "int fill_radius, unsigned char* rgb, float* depth, unsigned char* valid, int* face_or_null, long long* count, void* ws, "
            "long long ws_bytes, void* stream);") in flat
    assert "DEPTH TO VIEW" in hdr and "s = (e0 q0 + e1 q1) + e2 q2" in flat            # the header states the rules
    assert re.search(r"#define MG_VIEW_MAX_SPAN 64\b", hdr) and re.search(r"#define MG_VIEW_MAX_FILL 64\b", hdr)
    assert (L.VIEW_MAX_SPAN, L.VIEW_MAX_FILL) == (64, 64)
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bview\.hip\b", makefile, re.M)
    assert re.search(r"^FLAGS_view\s*:=\s*-ffp-contract=off\s*$", makefile, re.M)
    # one copy of each rule: the cell rules are the shared header's, and no kernel file defines them again
    csrc = os.path.join(ROOT, "marigold_amd", "csrc")
    rules = open(os.path.join(csrc, "depth3d.h")).read()
    for name in ("triangle_of", "cell_code"):
        assert len(re.findall(r"\b%s\([^;{]*\)\s*\{" % name, rules)) == 1, name
    assert "FORM_SPLIT_AD" in rules and "TRI_ACD" in rules and "CORNER_A" in rules
    for name in ("points.hip", "mesh.hip", "view.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "depth3d.h"' in src
        assert not re.search(r"\b(depth_at|joined_to|point_of|load_coef|check_common|triangle_of|cell_code)\([^;{]*\)\s*\{", src), name
        assert not re.search(r"\b(FORM_SPLIT_AD|TRI_ACD|CORNER_A)\s*=", src), name
    src = open(os.path.join(csrc, "view.hip")).read()
    assert "atomicMin(" in src and "asm" not in src and "atomicCAS" not in src and not re.search(r"atomicAdd\(\s*\(?\s*(float|double)", src)
    vp, i, ll, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_depth_view_workspace_bytes", "mg_depth_view"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_depth_view_workspace_bytes.argtypes == [ll] and lib.mg_depth_view_workspace_bytes.restype is ll
        assert lib.mg_depth_view.argtypes == [vp, vp, i, vp, vp, i, i] + [dbl] * 7 + [vp] + [dbl] * 4 + [i, i, dbl, i] + [vp] * 6 + [ll, vp]
    assert len(L.OP_NAMES) == 35 and ctypes.sizeof(L.MgOp) == 360   # a plain C call, no op kind
    assert not any("view" in name for name in L.OP_NAMES.values())
    import marigold_amd
    for name in ("HostView", "View", "render_view", "stereo_pair"):
        assert getattr(marigold_amd, name) is getattr(V, name)


@LIBS
def test_workspace_bytes(f16):
    lib = L.load(f16)
    for n in (0, -1, -(1 << 40), (1 << 30) + 1):
        assert lib.mg_depth_view_workspace_bytes(n) == -1
        assert lib.mg_last_error().decode().startswith("mg_depth_view_workspace_bytes:")
    sizes = [1, 2, 3, 63, 64, 65, 2049, 12319, 768 * 768, 3000 * 4000, 1 << 30]
    # a 64-bit key per target pixel, rounded up to 16 bytes; the counts are summed in `count` itself
    assert [lib.mg_depth_view_workspace_bytes(n) for n in sizes] == [(8 * n + 15) // 16 * 16 for n in sizes]


_VIEW = ("d", "colors", "hwc", "mask", "coef", "h", "w", "fx", "fy", "cx", "cy", "z_min", "z_max", "edge_rel", "pose", "fx2", "fy2", "cx2", "cy2",
         "h2", "w2", "z_near", "fill", "rgb", "depth", "valid", "face", "count", "ws", "ws_bytes")


@LIBS
def test_the_view_call_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()                      # stands for every device buffer: no call gets as far as reading it
    p = (ctypes.addressof(mem) + 15) // 16 * 16
    need = lib.mg_depth_view_workspace_bytes(12 * 9)
    pose = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)

    def call(**kw):
        a = dict(d=p, colors=p, hwc=1, mask=None, coef=None, h=10, w=10, fx=50.0, fy=50.0, cx=4.5, cy=4.5, z_min=0.0, z_max=INF, edge_rel=0.05,
                 pose=ctypes.addressof(pose), fx2=50.0, fy2=50.0, cx2=4.0, cy2=5.5, h2=12, w2=9, z_near=1e-6, fill=3, rgb=p, depth=p, valid=p, face=p,
                 count=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.mg_depth_view(*(a[k] for k in _VIEW), None), lib.mg_last_error().decode()

    def refused(*words, **kw):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("mg_depth_view:") and all(w in msg for w in words), (kw, rc, msg)

    for name in ("d", "colors", "rgb", "depth", "valid", "count", "ws"):
        refused("null pointer", **{name: None})
    for words, kw in _SHARED:          # what mg_depth_points refuses about the map, the camera and the rules
        if "frame" not in kw:          # (a view has no normals frame)
            refused(words, **kw)
    for kw in (dict(h2=0), dict(w2=-1), dict(h2=32769, w2=32769)):
        refused("target", "1 to 2^30 pixels", **kw)
    for kw in (dict(fx2=0.0), dict(fy2=-1.0), dict(fx2=NAN), dict(fy2=INF)):
        refused("target's focal lengths", **kw)
    for kw in (dict(cx2=NAN), dict(cy2=-INF)):
        refused("target's principal point", **kw)
    for k, bad in ((0, NAN), (3, INF), (11, -INF)):
        spoiled = (ctypes.c_double * 12)(*pose)
        spoiled[k] = bad
        refused("pose entry %d" % k, pose=ctypes.addressof(spoiled))
    for bad in (0.0, -1.0, NAN, INF):
        refused("z_near", z_near=bad)
    for bad in (-1, 65, 1 << 20):
        refused("fill_radius", fill=bad)
    for kw in (dict(d=p + 2), dict(depth=p + 2), dict(depth=p + 1), dict(face=p + 2), dict(count=p + 4), dict(coef=p + 4)):
        refused("aligned to their elements", **kw)
    refused("16-byte aligned", ws=p + 8)
    refused("workspace holds", ws_bytes=need - 1)
    refused("workspace holds", ws_bytes=0)
    refused("workspace holds", ws_bytes=lib.mg_depth_view_workspace_bytes(12 * 9 - 2))
    assert list(mem) == [0.0] * 64


# ---- marigold_amd.view on the host -------------------------------------------------------------------------------------------------

def test_the_python_calls_refuse_what_is_not_a_device_map(tmp_path):
    d = torch.zeros(4, 5)
    colors = torch.zeros(4, 5, 3, dtype=torch.uint8)
    K = P.Intrinsics(5.0, 5.0, 2.0, 1.5)
    for bad in (d, d.numpy(), None):
        with pytest.raises(ValueError, match="render_view"):
            V.render_view(bad, K, colors)
        with pytest.raises(ValueError, match="render_view"):
            V.stereo_pair(bad, K, colors, 0.1)
    with pytest.raises(ValueError, match="stereo_pair"):
        V.stereo_pair(d, K, colors, float("nan"))
    with pytest.raises(ValueError, match="stereo_pair"):
        V.stereo_pair(d, K, colors, 0.1, pose=None)
    assert V._pose("x", None) is None
    both = V._pose("x", (np.eye(3), (1.0, 2.0, 3.0)))
    assert both.tolist() == [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]] and np.array_equal(V._pose("x", both), both) and both.flags.c_contiguous
    assert np.array_equal(V._pose("x", torch.from_numpy(both)), both)
    for bad in ((np.eye(3),), np.eye(4), "pose", (np.eye(3), (1.0, NAN, 0.0))):
        with pytest.raises(ValueError, match="x: pose"):
            V._pose("x", bad)
    rgb = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    V.HostView(rgb, None, None, None, {}).write_ppm(tmp_path / "a.ppm")
    assert open(tmp_path / "a.ppm", "rb").read() == b"P6\n4 2\n255\n" + rgb.tobytes()
    with pytest.raises(ValueError, match="write_ppm"):
        V.write_ppm(tmp_path / "b.ppm", rgb[0])


# ---- the command line --------------------------------------------------------------------------------------------------------------

def test_the_parser_flags():
    from marigold_amd import cli
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    a = cli.build_parser("depth").parse_args(io)
    assert (a.save_stereo, a.stereo_baseline, a.stereo_fill) == (False, 0.065, 8)
    a = cli.build_parser("depth").parse_args(io + ["--save_stereo", "--fov_deg", "60", "--stereo_baseline", "0.3", "--stereo_fill", "0"])
    assert (a.save_stereo, a.stereo_baseline, a.stereo_fill, a.save_mesh, a.save_points) == (True, 0.3, 0, False, False)
    text = re.sub(r"\s+", " ", cli.build_parser("depth").format_help())
    assert text.count("rests on nothing measured") == 2                # both defaults say so
    for kind in ("normals", "iid"):
        for flag in (["--save_stereo"], ["--stereo_baseline", "1"], ["--stereo_fill", "1"]):
            with pytest.raises(SystemExit):
                cli.build_parser(kind).parse_args(io + flag)
        text = cli.build_parser(kind).format_help()
        assert "stereo" not in text and "points" not in text
    for kind in ("depth", "normals", "iid"):   # the launchers reach the flags through cli.main and do not name them
        src = open(os.path.join(ROOT, "script", kind, "run.py")).read()
        assert "stereo" not in src and "cli" in src


class _Host(V.HostView):
    __slots__ = ()

    def to_host(self):
        return self


def _restated_view(calls):
    """``render_view`` with the restatement in the kernel's place: host tensors in, a host view out"""
    def fake(depth, K, colors, *, pose=None, coef=None, edge_rel=0.05, fill_radius=0, **kw):
        calls.append(dict(K=K, coef=coef, edge_rel=edge_rel, fill=fill_radius, pose=V._pose("fake", pose), colors=tuple(colors.shape), **kw))
        r = view_reference(depth.numpy(), tuple(K), colors.numpy(), hwc=False, coef=coef, edge_rel=edge_rel, pose=V._pose("fake", pose),
                           fill_radius=fill_radius)
        return _Host(r.rgb.transpose(1, 2, 0), r.depth, r.valid, None, dict(zip(V.COUNT_NAMES, r.count)))
    return fake


def test_cli_main_writes_the_stereo_picture(tmp_path, monkeypatch):
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
    monkeypatch.setattr(V, "render_view", _restated_view(calls))
    pipe = _FakeCliPipe()
    assert cli.main("depth", base, pipeline=pipe) == 0                                      # without the flag: no folder, no call
    assert calls == [] and sorted(os.listdir(out)) == ["depth_bw", "depth_colored", "depth_npy"]
    depth = pipe._out().depth_np
    for extra, video in ((["--maps_in_flight", "2"], False), (["--sequence"], True)):
        del calls[:]
        pipe = _FakeCliPipe()
        argv = base + extra + ["--save_stereo", "--fov_deg", "60", "--points_near", "2", "--points_far", "6", "--stereo_baseline", "0.5",
                               "--stereo_fill", "2"]
        assert cli.main("depth", argv, pipeline=pipe) == 0
        assert pipe.calls[0][0] == ("map_video" if video else "map_images") and "stereo" not in " ".join(pipe.calls[0][2])
        assert sorted(os.listdir(out / "depth_stereo")) == ["a_stereo.png", "b_stereo.png"]
        assert len(calls) == 4 and all(c["colors"] == (3, 6, 8) and c["coef"] == (4.0, 2.0) and c["edge_rel"] == 0.05 and c["fill"] == 2 for c in calls)
        assert [c["pose"][0, 3] for c in calls] == [0.25, -0.25, 0.25, -0.25]               # the left eye, then the right
        assert all(np.array_equal(c["pose"][:, :3], np.eye(3)) and not c["pose"][1:, 3].any() for c in calls)
        big, small = P.intrinsics_from_fov(12, 16, 60.0), P.intrinsics_from_fov(6, 8, 60.0)
        assert calls[0]["K"] == P.scale_intrinsics(big, (12, 16), (6, 8)) and calls[2]["K"] == small   # (sorted: a.png first)
    b = np.array(Image.open(inp / "b.png"))
    got = np.array(Image.open(out / "depth_stereo" / "b_stereo.png"))
    assert got.shape == (6, 16, 3)                                                          # left beside right, at the map's size
    for half, tx in ((got[:, :8], 0.25), (got[:, 8:], -0.25)):
        pose = IDENTITY.copy()
        pose[0, 3] = tx
        want = view_reference(depth, tuple(small), b, coef=(4.0, 2.0), edge_rel=0.05, pose=pose, fill_radius=2)
        assert np.array_equal(half, want.rgb) and want.count[6] > 24
    assert not np.array_equal(got[:, :8], got[:, 8:])


def test_cli_refusals(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / "a.png")
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    calls = []
    monkeypatch.setattr(V, "render_view", _restated_view(calls))
    pipe = _FakeCliPipe()
    with pytest.raises(ValueError, match="--save_stereo cannot be combined with --tile_size"):
        cli.main("depth", base + ["--save_stereo", "--fov_deg", "60", "--tile_size", "64"], pipeline=pipe)
    for extra, word in ((["--save_stereo"], "exactly one of"), (["--save_stereo", "--fov_deg", "60", "--focal_px", "100"], "exactly one of"),
                        (["--save_stereo", "--fov_deg", "180"], "--fov_deg"),
                        (["--save_stereo", "--fov_deg", "60", "--points_near", "3", "--points_far", "2"], "near < far"),
                        (["--save_stereo", "--fov_deg", "60", "--stereo_baseline", "nan"], "--stereo_baseline"),
                        (["--save_stereo", "--fov_deg", "60", "--stereo_fill", "65"], "--stereo_fill"),
                        (["--save_stereo", "--fov_deg", "60", "--stereo_fill", "-1"], "--stereo_fill")):
        with pytest.raises(SystemExit) as e:
            cli.main("depth", base + extra, pipeline=pipe)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert pipe.calls == [] and calls == []
    # without --save_stereo its flags pass unseen
    assert cli.main("depth", base + ["--stereo_fill", "99", "--tile_size", "64"], pipeline=pipe) == 0 and calls == []
    assert cli.main("depth", base + ["--save_stereo", "--focal_px", "9"], pipeline=pipe) == 0
    assert calls[0]["K"] == P.Intrinsics(9.0, 9.0, 3.5, 2.5) and calls[0]["fill"] == 8 and calls[0]["pose"][0, 3] == 0.0325


# ---- the C host example ------------------------------------------------------------------------------------------------------------

def test_the_c_host_example_compiles(tmp_path):
    c_hosts.compile_only(os.path.join(ROOT, "examples", "host_view.cpp"), tmp_path / "host_view.o")
    assert os.path.getsize(tmp_path / "host_view.o") > 0
    assert "host_view" in open(os.path.join(ROOT, "README.md")).read()
