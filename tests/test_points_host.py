"""Host checks of depth to 3D, no GPU.  The numpy restatement the GPU tests are held against gives what geometry says
on scenes with a closed form; the three C entry points are declared, bound and exported by both operand libraries without a new op
kind, and refuse bad arguments before any GPU work (no GPU is here: a call that got as far as a launch would fail differently, so the
message proves where it stopped); the camera helpers and the PLY writer and reader round-trip; the command line has its flags on the
depth parser alone, refuses what it must, and writes the file through a stand-in pipeline with the restatement in the kernel's place."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import points as P
from marigold_amd.pipeline import MarigoldDepthOutput
from tests import c_hosts
from tests.points_reference import CENTRAL, HIGH_ONLY, LOW_ONLY, NONE, points_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


# ---- the restatement on scenes with a closed form ----------------------------------------------------------------------------------

def test_a_plane_facing_the_camera_has_the_normal_0_0_1():
    d = np.full((9, 13), 2.5, np.float32)
    for K in ((11.0, 12.5, 6.3, 3.9), (700.0, 700.0, 6.0, 4.0)):
        r = points_reference(d, K, frame="marigold")
        assert r.kept.all() and r.valid.all() and r.count == (117, 117)
        assert (r.dense[0] == 0).all() and (r.dense[1] == 0).all() and (r.dense[2] == 1).all()
        assert (r.form_u[:, 1:-1] == CENTRAL).all() and (r.form_u[:, 0] == HIGH_ONLY).all() and (r.form_u[:, -1] == LOW_ONLY).all()
        assert (r.form_v[1:-1] == CENTRAL).all() and (r.form_v[0] == HIGH_ONLY).all() and (r.form_v[-1] == LOW_ONLY).all()
        cam = points_reference(d, K, frame="camera")
        assert (cam.dense[2] == -1).all() and (cam.dense[:2] == 0).all()
        assert np.array_equal(r.index, np.arange(117)) and (r.xyz[:, 2] == 2.5).all()
        assert r.xyz[0, 0] == np.float32(((0 - K[2]) * 2.5) / K[0]) and r.xyz[-1, 1] == np.float32(((8 - K[3]) * 2.5) / K[1])


def test_a_tilted_plane_has_its_analytic_normal():
    """The plane Z = a X + b Y + c in the camera's coordinates, seen by a pinhole: along the ray of pixel (x, y) the depth is
    c / (1 - a rx - b ry).  Neighbouring points all lie in the plane, so every tangent does and the cross product is the plane's
    normal, (a, b, -1) normalised, at every pixel - central or one-sided.  The restatement computes in fp64 and rounds unit vectors to
    fp32, whose resolution is 6e-8; the depths themselves are fp32, which at this wide angle (f = 4 pixels) costs a few 1e-7 more.
    The bound is 1e-6 per component."""
    a, b, c = 0.3, -0.2, 3.0
    K = (4.0, 5.0, 5.2, 3.9)
    ys, xs = np.meshgrid(np.arange(9, dtype=np.float64), np.arange(11, dtype=np.float64), indexing="ij")
    d = (c / (1.0 - a * (xs - K[2]) / K[0] - b * (ys - K[3]) / K[1])).astype(np.float32)
    assert (d > 0).all()
    n = np.array([a, b, -1.0]) / math.sqrt(a * a + b * b + 1.0)
    for frame, want in (("camera", n), ("marigold", n * (1, -1, -1))):
        r = points_reference(d, K, frame=frame)
        assert r.valid.all()
        err = np.abs(r.dense.astype(np.float64) - want[:, None, None]).max()
        assert err <= 1e-6, err
    # the same map as 0.5 * d' + 1 with d' = 2 (d - 1): coef carries the affine step
    r2 = points_reference(((d.astype(np.float64) - 1.0) * 2.0).astype(np.float32), K, coef=(0.5, 1.0), frame="camera")
    assert np.abs(r2.dense.astype(np.float64) - n[:, None, None]).max() <= 1e-6


def test_a_depth_step_drops_the_two_columns_at_the_step():
    """A 20 % step with edge_rel = 0.05: the columns either side of it are not joined to each other, so exactly those two are dropped.
    The columns beside them keep central tangents - their neighbour in a dropped column is usable and joined to them, which is all the
    definition of a tangent asks - and still look at the camera.  One-sided tangents appear where the neighbour is not usable: with the
    two columns masked out as well, the columns beside them difference to one side only, and the normal is unchanged."""
    d = np.full((5, 12), 2.0, np.float32)
    d[:, 6:] = 2.4
    K = (20.0, 20.0, 5.5, 2.0)
    r = points_reference(d, K, edge_rel=0.05, frame="marigold")
    assert r.usable.all() and not r.kept[:, 5:7].any() and r.kept[:, :5].all() and r.kept[:, 7:].all()
    assert r.removed == dict(mask=0, nonfinite=0, range=0, edge=10) and r.count == (50, 50)
    assert (r.form_u[:, 4] == CENTRAL).all() and (r.form_u[:, 7] == CENTRAL).all() and (r.form_u[:, 5:7] == NONE).all()
    assert (r.valid[:, 5:7] == 0).all() and (r.dense[:, :, 5:7] == 0).all()
    keep = np.r_[0:5, 7:12]
    assert (r.dense[2][:, keep] == 1).all() and (r.dense[:2][:, :, keep] == 0).all()
    assert not points_reference(d, K, edge_rel=0.0).removed["edge"] and not points_reference(d, K, edge_rel=0.25).removed["edge"]
    mask = np.ones((5, 12), np.uint8)
    mask[:, 5:7] = 0
    m = points_reference(d, K, mask=mask, edge_rel=0.05, frame="marigold")
    assert np.array_equal(m.kept, r.kept) and m.removed == dict(mask=10, nonfinite=0, range=0, edge=0)
    assert (m.form_u[:, 4] == LOW_ONLY).all() and (m.form_u[:, 7] == HIGH_ONLY).all()
    assert (m.dense[2][:, keep] == 1).all() and (m.dense[:2][:, :, keep] == 0).all()


def test_the_restatement_s_rules():
    d = np.array([[2.0, np.nan, 2.0, np.inf, 2.0, 1.0, 3.0, 2.0]], np.float32)
    r = points_reference(d, (5.0, 5.0, 3.5, 0.0), z_range=(1.0, 3.0))
    assert r.usable.tolist() == [[True, False, True, False, True, False, True, True]]   # z_min < z <= z_max
    assert r.removed == dict(mask=0, nonfinite=2, range=1, edge=0)
    assert (r.form_u[0, [0, 2, 4]] == NONE).all() and r.kept[0, [0, 2, 4]].all() and not r.valid.any()   # kept, yet no normal
    assert (r.nrm == 0).all() and len(r.nrm) == r.count[0] == 5
    cut = points_reference(d, (5.0, 5.0, 3.5, 0.0), z_range=(1.0, 3.0), capacity=2, colors=np.arange(24, dtype=np.uint8).reshape(1, 8, 3))
    assert cut.count == (5, 2) and cut.index.tolist() == [0, 2] and cut.rgb.tolist() == [[0, 1, 2], [6, 7, 8]]
    planes = points_reference(d, (5.0, 5.0, 3.5, 0.0), z_range=(1.0, 3.0), colors=np.arange(24, dtype=np.uint8).reshape(3, 1, 8), hwc=False)
    assert planes.rgb[:2].tolist() == [[0, 8, 16], [2, 10, 18]]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "enum { MG_NORMALS_FRAME_CAMERA = 0, MG_NORMALS_FRAME_MARIGOLD = 1 };" in flat
    assert ("int mg_depth_normals(const float* d, const unsigned char* mask_or_null, const double* coef_or_null, int h, int w, double fx, "
            "double fy, double cx, double cy, double z_min, double z_max, double edge_rel, int normals_frame, float* out, "
            "unsigned char* valid, void* stream);") in flat
    assert "long long mg_depth_points_workspace_bytes(long long n);" in flat
    assert ("int mg_depth_points(const float* d, const unsigned char* colors_or_null, int hwc, const unsigned char* mask_or_null, "
            "const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy, double z_min, double z_max, "
            "double edge_rel, int normals_frame, long long capacity, float* xyz, unsigned char* rgb_or_null, float* nrm_or_null, "
            "int* index_or_null, long long* count, void* ws, long long ws_bytes, void* stream);") in flat
    assert "x right, y up, z toward the viewer" in flat   # the header states the published convention
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bpoints\.hip\b", makefile, re.M)
    assert re.search(r"^FLAGS_points\s*:=\s*-ffp-contract=off\s*$", makefile, re.M)
    vp, i, ll, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_depth_normals", "mg_depth_points_workspace_bytes", "mg_depth_points"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_depth_normals.argtypes == [vp, vp, vp, i, i] + [dbl] * 7 + [i, vp, vp, vp]
        assert lib.mg_depth_points_workspace_bytes.argtypes == [ll] and lib.mg_depth_points_workspace_bytes.restype is ll
        assert lib.mg_depth_points.argtypes == [vp, vp, i, vp, vp, i, i] + [dbl] * 7 + [i, ll] + [vp] * 6 + [ll, vp]
    assert L.NORMALS_FRAME == {"camera": 0, "marigold": 1}
    assert len(L.OP_NAMES) == 35 and ctypes.sizeof(L.MgOp) == 360   # plain C calls, no op kind
    assert not any("point" in name for name in L.OP_NAMES.values())
    import marigold_amd
    for name in ("Intrinsics", "PointCloud", "depth_to_normals", "depth_to_points", "intrinsics_from_fov", "read_ply", "scale_intrinsics",
                 "write_ply"):
        assert getattr(marigold_amd, name) is getattr(P, name)


@LIBS
def test_workspace_bytes(f16):
    lib = L.load(f16)
    for n in (0, -1, -(1 << 40), (1 << 30) + 1):
        assert lib.mg_depth_points_workspace_bytes(n) == -1
        assert lib.mg_last_error().decode().startswith("mg_depth_points_workspace_bytes:")
    sizes = [1, 2, 63, 64, 65, 2047, 2048, 2049, 12319, 768 * 768, 3000 * 4000, 1 << 30]
    got = [lib.mg_depth_points_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 16 == 0 for b in got) and got == sorted(got)
    assert got[6] < got[7] and got[0] == got[6]                   # one chunk of 2048 pixels, then two
    assert got[-1] == (1 << 30) // 2048 * 16                      # the counts and the offsets of the chunks, nothing else


_POINTS = ("d", "colors", "hwc", "mask", "coef", "h", "w", "fx", "fy", "cx", "cy", "z_min", "z_max", "edge_rel", "frame", "capacity", "xyz", "rgb",
           "nrm", "index", "count", "ws", "ws_bytes")
_NORMALS = ("d", "mask", "coef", "h", "w", "fx", "fy", "cx", "cy", "z_min", "z_max", "edge_rel", "frame", "out", "valid")
INF, NAN = float("inf"), float("nan")
_SHARED = [("1 to 2^30 pixels", dict(h=0)), ("1 to 2^30 pixels", dict(w=-3)), ("1 to 2^30 pixels", dict(h=32769, w=32769)),
           ("focal lengths", dict(fx=0.0)), ("focal lengths", dict(fy=-1.0)), ("focal lengths", dict(fx=NAN)), ("focal lengths", dict(fy=INF)),
           ("principal point", dict(cx=NAN)), ("principal point", dict(cy=-INF)),
           ("z_min", dict(z_min=-0.5)), ("z_min", dict(z_min=NAN)), ("z_min", dict(z_min=INF)),
           ("z_max", dict(z_max=NAN)), ("z_max", dict(z_min=1.0, z_max=1.0)), ("z_max", dict(z_min=2.0, z_max=1.0)),
           ("edge_rel", dict(edge_rel=-0.1)), ("edge_rel", dict(edge_rel=NAN)), ("edge_rel", dict(edge_rel=INF)),
           ("normals frame", dict(frame=-1)), ("normals frame", dict(frame=2))]


@LIBS
def test_the_points_call_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()                      # stands for every device buffer: no call gets as far as reading it
    p = (ctypes.addressof(mem) + 15) // 16 * 16
    need = lib.mg_depth_points_workspace_bytes(100)

    def call(**kw):
        a = dict(d=p, colors=p, hwc=1, mask=None, coef=None, h=10, w=10, fx=50.0, fy=50.0, cx=4.5, cy=4.5, z_min=0.0, z_max=INF, edge_rel=0.05, frame=0,
                 capacity=100, xyz=p, rgb=p, nrm=p, index=p, count=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.mg_depth_points(*(a[k] for k in _POINTS), None), lib.mg_last_error().decode()

    def refused(*words, **kw):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("mg_depth_points:") and all(w in msg for w in words), (kw, rc, msg)

    for name in ("d", "xyz", "count", "ws"):
        refused("null pointer", **{name: None})
    refused("go together", colors=None)
    refused("go together", rgb=None)
    for words, kw in _SHARED:
        refused(words, **kw)
    for capacity in (0, -1):
        refused("capacity", capacity=capacity)
    for kw in (dict(d=p + 2), dict(xyz=p + 2), dict(nrm=p + 1), dict(index=p + 2), dict(count=p + 4), dict(coef=p + 4)):
        refused("aligned to their elements", **kw)
    refused("16-byte aligned", ws=p + 8)
    refused("workspace holds", ws_bytes=need - 1)
    refused("workspace holds", ws_bytes=0)
    assert list(mem) == [0.0] * 64


@LIBS
def test_the_normals_call_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()
    p = (ctypes.addressof(mem) + 15) // 16 * 16

    def refused(*words, **kw):
        a = dict(d=p, mask=None, coef=None, h=10, w=10, fx=50.0, fy=50.0, cx=4.5, cy=4.5, z_min=0.0, z_max=INF, edge_rel=0.0, frame=1, out=p, valid=p)
        a.update(kw)
        rc = lib.mg_depth_normals(*(a[k] for k in _NORMALS), None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_depth_normals:") and all(w in msg for w in words), (kw, rc, msg)

    for name in ("d", "out", "valid"):
        refused("null pointer", **{name: None})
    for words, kw in _SHARED:
        refused(words, **kw)
    for kw in (dict(d=p + 2), dict(out=p + 1), dict(coef=p + 4)):
        refused("aligned to their elements", **kw)
    assert list(mem) == [0.0] * 64


# ---- marigold_amd.points on the host -----------------------------------------------------------------------------------------------

def test_the_camera_helpers():
    K = P.intrinsics_from_fov(480, 640, 90.0)
    assert K.cx == 319.5 and K.cy == 239.5 and K.fx == K.fy and abs(K.fx - 320.0) < 1e-9
    assert abs(P.intrinsics_from_fov(10, 20, 60.0).fx - 10.0 / math.tan(math.radians(30.0))) < 1e-12
    # the pixel-centre rule: the picture's corner (-0.5, -0.5) stays the corner, the centre stays the centre
    half = P.scale_intrinsics(K, (480, 640), (240, 320))
    assert half == P.Intrinsics(K.fx / 2, K.fy / 2, 159.5, 119.5)
    assert P.scale_intrinsics(P.Intrinsics(100.0, 100.0, -0.5, -0.5), (30, 40), (77, 13))[2:] == (-0.5, -0.5)
    for K0 in (K, P.Intrinsics(511.3, 498.7, 300.25, 251.5)):
        for to in ((96, 128), (77, 1013), (1, 1), (2161, 3)):
            back = P.scale_intrinsics(P.scale_intrinsics(K0, (480, 640), to), to, (480, 640))
            assert max(abs(u - v) for u, v in zip(back, K0)) <= 1e-12 * max(1.0, max(abs(v) for v in K0)), (K0, to, back)
    for bad in ((0, 10, 60.0), (10, 10, 0.0), (10, 10, 180.0)):
        with pytest.raises(ValueError, match="intrinsics_from_fov"):
            P.intrinsics_from_fov(*bad)
    with pytest.raises(ValueError, match="scale_intrinsics"):
        P.scale_intrinsics(K, (480, 640), (0, 5))


@pytest.mark.parametrize("normals", [False, True], ids=["bare", "normals"])
@pytest.mark.parametrize("colours", [False, True], ids=["plain", "colours"])
def test_a_ply_round_trip_byte_for_byte(tmp_path, normals, colours):
    g = np.random.default_rng(3)
    xyz = g.standard_normal((37, 3)).astype(np.float32)
    xyz[0] = (np.inf, -0.0, 1e-42)
    nrm = g.standard_normal((37, 3)).astype(np.float32) if normals else None
    rgb = g.integers(0, 256, (37, 3), dtype=np.uint8) if colours else None
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    P.write_ply(a, xyz, nrm, rgb)
    raw = open(a, "rb").read()
    names = ["x", "y", "z"] + ["nx", "ny", "nz"] * normals + ["red", "green", "blue"] * colours
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 37\n" + \
        "".join(f"property {'uchar' if n in ('red', 'green', 'blue') else 'float'} {n}\n" for n in names) + "end_header\n"
    assert raw.startswith(head.encode()) and len(raw) == len(head) + 37 * (12 + 12 * normals + 3 * colours)
    assert raw[len(head):len(head) + 12] == xyz[0].tobytes()
    cloud = P.read_ply(a)
    assert (cloud.kept, cloud.written, cloud.index) == (37, 37, None)
    assert cloud.xyz.tobytes() == xyz.tobytes() and (cloud.normals is None) == (not normals) and (cloud.rgb is None) == (not colours)
    assert (not normals or cloud.normals.tobytes() == nrm.tobytes()) and (not colours or np.array_equal(cloud.rgb, rgb))
    cloud.write_ply(b)
    assert open(b, "rb").read() == raw
    P.write_ply(b, xyz[:0], None if nrm is None else nrm[:0], None if rgb is None else rgb[:0])   # an empty cloud is a file too
    assert P.read_ply(b).written == 0
    with pytest.raises(ValueError, match="read_ply"):
        open(b, "wb").write(raw[:-1])
        P.read_ply(b)


def test_the_python_calls_refuse_what_is_not_a_device_map():
    d = torch.zeros(4, 5)
    for fn in (P.depth_to_points, P.depth_to_normals):
        for bad in (d, d.numpy(), None):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(bad, P.Intrinsics(5.0, 5.0, 2.0, 1.5))


# ---- the command line --------------------------------------------------------------------------------------------------------------

class _FakeCliPipe:
    """a depth pipeline as the command line sees one: maps of 6 x 8 whatever the picture's size"""
    scale_invariant = shift_invariant = True
    default_denoising_steps, default_processing_resolution = 4, 768

    def __init__(self):
        self.calls = []

    def _out(self):
        from PIL import Image
        ys, xs = np.meshgrid(np.arange(6), np.arange(8), indexing="ij")
        depth = (0.2 + 0.01 * xs + 0.02 * ys + 0.4 * (xs >= 5)).astype(np.float32)   # a gentle slope and one step
        return MarigoldDepthOutput(depth, Image.fromarray(np.zeros((6, 8, 3), np.uint8)), None)

    def map_images(self, images, in_flight=None, generators=None, **kw):
        images = list(images)
        self.calls.append(("map_images", len(images), kw))
        return [self._out() for _ in images]

    def map_video(self, frames, strength=0.1, in_flight=None, generators=None, **kw):
        frames = list(frames)
        self.calls.append(("map_video", len(frames), kw))
        return [self._out() for _ in frames]

    def predict_tiled(self, image, **kw):
        self.calls.append(("predict_tiled", 1, kw))
        return self._out()


def test_the_parser_flags():
    from marigold_amd import cli
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    a = cli.build_parser("depth").parse_args(io)
    assert (a.save_points, a.fov_deg, a.focal_px, a.points_near, a.points_far, a.points_edge_rel, a.points_normals) == \
        (False, None, None, 1.0, 10.0, 0.05, False)
    a = cli.build_parser("depth").parse_args(io + ["--save_points", "--focal_px", "500", "--points_near", "0.5", "--points_far", "4",
                                                   "--points_edge_rel", "0", "--points_normals"])
    assert (a.save_points, a.fov_deg, a.focal_px, a.points_near, a.points_far, a.points_edge_rel, a.points_normals) == \
        (True, None, 500.0, 0.5, 4.0, 0.0, True)
    assert "arbitrary" in re.sub(r"\s+", " ", cli.build_parser("depth").format_help())
    for kind in ("normals", "iid"):
        for flag in (["--save_points"], ["--fov_deg", "60"], ["--focal_px", "500"], ["--points_near", "1"], ["--points_far", "2"],
                     ["--points_edge_rel", "0"], ["--points_normals"]):
            with pytest.raises(SystemExit):
                cli.build_parser(kind).parse_args(io + flag)
        assert "points" not in cli.build_parser(kind).format_help()
    for kind in ("depth", "normals", "iid"):   # the launchers reach the flags through cli.main and name none of them
        src = open(os.path.join(ROOT, "script", kind, "run.py")).read()
        assert "points" not in src and "cli" in src


def _restated(calls):
    """``depth_to_points`` with the restatement in the kernel's place: host tensors in, a host cloud out"""
    def fake(depth, K, *, colors=None, coef=None, edge_rel=0.0, normals=False, frame="camera", **kw):
        calls.append(dict(K=K, coef=coef, edge_rel=edge_rel, normals=normals, frame=frame, colors=tuple(colors.shape), **kw))
        r = points_reference(depth.numpy(), tuple(K), colors=colors.numpy(), hwc=False, coef=coef, edge_rel=edge_rel, frame=frame)
        return P.HostPointCloud(r.xyz, r.rgb, r.nrm if normals else None, None, *r.count)
    return fake


def test_cli_main_writes_the_cloud(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    g = np.random.default_rng(1)
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(g.integers(0, 256, (6, 8, 3), dtype=np.uint8)).save(inp / "b.png")      # the map's size
    Image.fromarray(g.integers(0, 256, (12, 16, 3), dtype=np.uint8)).save(inp / "a.png")    # twice the map's size
    out = tmp_path / "out"
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(out)]
    # without the flag nothing changes: no folder, no call
    calls = []
    monkeypatch.setattr(P, "depth_to_points", _restated(calls))
    pipe = _FakeCliPipe()
    assert cli.main("depth", base, pipeline=pipe) == 0
    assert calls == [] and not (out / "depth_points").exists() and sorted(os.listdir(out)) == ["depth_bw", "depth_colored", "depth_npy"]
    depth = pipe._out().depth_np
    for extra, video in ((["--maps_in_flight", "2"], False), (["--sequence"], True)):
        for normals in (False, True):
            del calls[:]
            pipe = _FakeCliPipe()
            argv = base + extra + ["--save_points", "--fov_deg", "60", "--points_near", "2", "--points_far", "6"] + ["--points_normals"] * normals
            assert cli.main("depth", argv, pipeline=pipe) == 0
            assert pipe.calls[0][0] == ("map_video" if video else "map_images") and "points" not in " ".join(pipe.calls[0][2])
            assert sorted(os.listdir(out / "depth_points")) == ["a_points.ply", "b_points.ply"]
            assert [c["colors"] for c in calls] == [(3, 6, 8)] * 2 and all(c["coef"] == (4.0, 2.0) and c["edge_rel"] == 0.05 for c in calls)
            big, small = P.intrinsics_from_fov(12, 16, 60.0), P.intrinsics_from_fov(6, 8, 60.0)
            assert calls[0]["K"] == P.scale_intrinsics(big, (12, 16), (6, 8)) and calls[1]["K"] == small   # (sorted: a.png first)
            assert abs(calls[0]["K"].fx - small.fx) < 1e-12 and calls[0]["K"].cx == 3.5
            for name, c in zip(("a", "b"), calls):
                raw = open(out / "depth_points" / f"{name}_points.ply", "rb").read()
                want = points_reference(depth, tuple(c["K"]), coef=(4.0, 2.0), edge_rel=0.05)
                assert 0 < want.count[1] < 48
                head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {want.count[1]}\nproperty float x\nproperty float y\nproperty float z\n"
                        + "property float nx\nproperty float ny\nproperty float nz\n" * normals
                        + "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
                assert raw.startswith(head.encode()) and len(raw) == len(head) + want.count[1] * (27 if normals else 15)
                cloud = P.read_ply(out / "depth_points" / f"{name}_points.ply")
                assert cloud.xyz.tobytes() == want.xyz.tobytes() and (cloud.normals is not None) == normals
    b = np.array(Image.open(inp / "b.png"))
    assert np.array_equal(P.read_ply(out / "depth_points" / "b_points.ply").rgb, b.reshape(-1, 3)[want.index])


def test_cli_refusals(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / "a.png")
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    calls = []
    monkeypatch.setattr(P, "depth_to_points", _restated(calls))
    pipe = _FakeCliPipe()
    with pytest.raises(ValueError, match="--save_points cannot be combined with --tile_size"):
        cli.main("depth", base + ["--save_points", "--fov_deg", "60", "--tile_size", "64"], pipeline=pipe)
    for extra, word in ((["--save_points"], "exactly one of"), (["--save_points", "--fov_deg", "60", "--focal_px", "100"], "exactly one of"),
                        (["--save_points", "--fov_deg", "180"], "--fov_deg"), (["--save_points", "--focal_px", "0"], "--focal_px"),
                        (["--save_points", "--fov_deg", "60", "--points_near", "3", "--points_far", "2"], "near < far"),
                        (["--save_points", "--fov_deg", "60", "--points_edge_rel", "-1"], "--points_edge_rel")):
        with pytest.raises(SystemExit) as e:
            cli.main("depth", base + extra, pipeline=pipe)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert pipe.calls == [] and calls == []
    # without --save_points the other flags pass unseen, and --tile_size runs as before
    assert cli.main("depth", base + ["--fov_deg", "60", "--tile_size", "64"], pipeline=pipe) == 0
    assert pipe.calls[0][0] == "predict_tiled" and calls == []
    # --focal_px: the principal point at the picture's centre
    assert cli.main("depth", base + ["--save_points", "--focal_px", "9"], pipeline=pipe) == 0
    assert calls[0]["K"] == P.Intrinsics(9.0, 9.0, 3.5, 2.5)


# ---- the C host example ------------------------------------------------------------------------------------------------------------

def test_the_c_host_example_compiles(tmp_path):
    c_hosts.compile_only(os.path.join(ROOT, "examples", "host_points.cpp"), tmp_path / "host_points.o")
    assert os.path.getsize(tmp_path / "host_points.o") > 0
    assert "host_points" in open(os.path.join(ROOT, "README.md")).read()
