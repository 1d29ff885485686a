"""Host checks of depth to mesh, no GPU.  The numpy restatement the GPU tests are held against gives what geometry says
on scenes with a closed form; the two C entry points are declared, bound and exported by both operand libraries without a new op kind,
and refuse bad arguments before any GPU work (no GPU is here: a call that got as far as a launch would fail differently, so the message
proves where it stopped); the PLY writer and reader round-trip; the command line has its flag on the depth parser alone, refuses what
it must, and writes the file through a stand-in pipeline with the restatement in the kernel's place."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import mesh as M
from marigold_amd import points as P
from tests import c_hosts
from tests.mesh_reference import NO_A, NO_B, NO_C, NO_CELL, NO_D, SPLIT_AD, SPLIT_BC, mesh_reference
from tests.points_reference import points_reference
from tests.test_points_host import _FakeCliPipe, _SHARED, INF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


# ---- the restatement on scenes with a closed form ----------------------------------------------------------------------------------

def _dets(r):
    """det[P0, P1, P2] of every face, fp64 from the fp32 records: negative when (P1 - P0) x (P2 - P0) points toward the camera"""
    p = r.xyz.astype(np.float64)[r.faces]
    return np.einsum("ni,ni->n", p[:, 0], np.cross(p[:, 1], p[:, 2]))


def test_a_constant_plane_is_two_triangles_per_cell():
    for h, w in ((2, 2), (5, 9), (9, 4)):
        d = np.full((h, w), 2.5, np.float32)
        for K in ((11.0, 12.5, 3.3, 1.9), (700.0, 700.0, 4.0, 2.0)):
            r = mesh_reference(d, K, edge_rel=0.05)
            V, F = h * w, 2 * (h - 1) * (w - 1)
            assert r.count == (V, V, F, F) and r.vertex.all() and r.has_normal.all()
            assert (r.form == SPLIT_AD).all() and r.tie.all() and (r.kept4 == 2).all()      # the tie goes to A-D
            assert (_dets(r) < 0).all()                                                      # every face looks at the camera
            assert np.array_equal(np.unique(r.faces), np.arange(V))                          # every vertex is referenced
            assert np.array_equal(r.index, np.arange(V))
            # the first cell: T0 = (A, C, D), T1 = (A, D, B); the last face ends in the last cell's B
            assert r.faces[0].tolist() == [0, w, w + 1] and r.faces[1].tolist() == [0, w + 1, 1]
            assert r.faces[-1].tolist() == [V - w - 2, V - 1, V - w - 1]
            assert (r.nrm[:, 2] == -1).all() and (r.nrm[:, :2] == 0).all()
            assert (mesh_reference(d, K, frame="marigold").nrm[:, 2] == 1).all()


def test_a_depth_step_removes_the_faces_of_the_column_that_straddles_it():
    """A 20 % step with edge_rel = 0.05: the cells whose corners sit either side of it lose both triangles, whichever way they are
    split - each triangle has an edge across the step.  Every pixel still belongs to a face of the cells beside them: no vertex goes.
    With the two columns at the step masked out, the cells that touch them have two usable corners at the most, and the vertices go."""
    h, w = 5, 12
    d = np.full((h, w), 2.0, np.float32)
    d[:, 6:] = 2.4
    K = (20.0, 20.0, 5.5, 2.0)
    r = mesh_reference(d, K, edge_rel=0.05)
    assert r.usable.all() and r.count == (h * w, h * w, 2 * (h - 1) * (w - 2), 2 * (h - 1) * (w - 2))
    assert (r.kept4[:, 5] == 0).all() and (np.delete(r.kept4, 5, axis=1) == 2).all()
    assert r.vertex.all() and (_dets(r) < 0).all()
    # the vertices at the step have one-sided horizontal tangents: their normals still look at the camera
    assert r.has_normal.all() and (r.nrm[:, 2] == -1).all()
    # a cloud of the same map drops those two columns (6h's demotion); the mesh keeps them
    assert not points_reference(d, K, edge_rel=0.05).kept[:, 5:7].any()
    for edge in (0.0, 0.25):
        assert mesh_reference(d, K, edge_rel=edge).count[2] == 2 * (h - 1) * (w - 1)
    mask = np.ones((h, w), np.uint8)
    mask[:, 5:7] = 0
    m = mesh_reference(d, K, mask=mask, edge_rel=0.05)
    assert m.count == (h * (w - 2), h * (w - 2), 2 * (h - 1) * (w - 4), 2 * (h - 1) * (w - 4))
    assert not m.vertex[:, 5:7].any() and m.vertex[:, :5].all() and m.vertex[:, 7:].all()
    assert (m.form[:, 4:7] == NO_CELL).all() and (_dets(m) < 0).all()
    assert np.array_equal(m.index, np.flatnonzero(mask.reshape(-1)))


def test_each_three_corner_form_of_a_2_x_2_map():
    K = (3.0, 3.0, 0.5, 0.5)
    # (the corner removed, the form, the candidate as pixels of the full map A = 0, B = 1, C = 2, D = 3)
    for gone, form, pixels in ((3, NO_D, (0, 2, 1)), (0, NO_A, (1, 2, 3)), (1, NO_B, (0, 2, 3)), (2, NO_C, (0, 3, 1))):
        d = np.array([[2.0, 2.1], [2.2, 2.3]], np.float32)
        d.reshape(-1)[gone] = np.nan
        r = mesh_reference(d, K)
        assert r.form.tolist() == [[form]] and r.count == (3, 3, 1, 1) and r.t0.all() and not r.t1.any() and (r.kept4 == -1).all()
        assert r.index.tolist() == [i for i in range(4) if i != gone]
        assert r.index[r.faces[0]].tolist() == list(pixels)
        assert (_dets(r) < 0).all()
    # the split follows the smaller diagonal difference; either way both triangles look at the camera
    ad = mesh_reference(np.array([[2.0, 2.5], [3.0, 2.125]], np.float32), K)
    bc = mesh_reference(np.array([[2.0, 2.5], [2.625, 3.0]], np.float32), K)
    assert ad.form.tolist() == [[SPLIT_AD]] and ad.faces.tolist() == [[0, 2, 3], [0, 3, 1]] and not ad.tie.any()
    assert bc.form.tolist() == [[SPLIT_BC]] and bc.faces.tolist() == [[0, 2, 1], [1, 2, 3]]
    assert (_dets(ad) < 0).all() and (_dets(bc) < 0).all()
    # the split is chosen first; then each triangle stands or falls on its own: D far away leaves (A, C, B) of the B-C split
    one = mesh_reference(np.array([[2.0, 2.01], [2.02, 3.0]], np.float32), K, edge_rel=0.05)
    assert one.form.tolist() == [[SPLIT_BC]] and one.kept4.tolist() == [[1]] and one.count == (3, 3, 1, 1) and one.usable.all()
    assert one.index.tolist() == [0, 1, 2] and one.faces.tolist() == [[0, 2, 1]]
    # two usable corners: nothing; one row or one column: no cells
    assert mesh_reference(np.array([[2.0, np.nan], [np.inf, 2.0]], np.float32), K).count == (0, 0, 0, 0)
    assert mesh_reference(np.full((1, 7), 2.0, np.float32), K).count == (0, 0, 0, 0)
    assert mesh_reference(np.full((7, 1), 2.0, np.float32), K).count == (0, 0, 0, 0)


def test_the_restatement_s_capacities_and_colours():
    d = np.full((3, 4), 2.0, np.float32)
    K = (5.0, 5.0, 1.5, 1.0)
    colors = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    r = mesh_reference(d, K, colors=colors, capacity_f=5)
    assert r.count == (12, 12, 12, 5) and len(r.faces) == 5 and r.rgb.tolist() == colors.reshape(12, 3).tolist()
    cut = mesh_reference(d, K, colors=colors.transpose(2, 0, 1), hwc=False, capacity_v=11)
    assert cut.count == (12, 11, 12, 0) and len(cut.faces) == 0 and len(cut.xyz) == 11 and cut.rgb.tolist() == colors.reshape(12, 3)[:11].tolist()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "long long mg_depth_mesh_workspace_bytes(long long n);" in flat
    assert ("int mg_depth_mesh(const float* d, const unsigned char* colors_or_null, int hwc, const unsigned char* mask_or_null, "
            "const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy, double z_min, double z_max, "
            "double edge_rel, int normals_frame, long long capacity_v, long long capacity_f, float* xyz, unsigned char* rgb_or_null, "
            "float* nrm_or_null, int* index_or_null, int* faces, long long* count, void* ws, long long ws_bytes, void* stream);") in flat
    assert "split along A-D when |z_A - z_D| <= |z_B - z_C|" in flat   # the header states the rules
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh\.hip\b", makefile, re.M) and re.search(r"^SRCS\s*:=.*\bpoints\.hip\b", makefile, re.M)
    assert re.search(r"^FLAGS_mesh\s*:=\s*-ffp-contract=off\s*$", makefile, re.M)
    # one copy of each rule: the two kernel files take them from the header they share
    csrc = os.path.join(ROOT, "marigold_amd", "csrc")
    for name in ("points.hip", "mesh.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "depth3d.h"' in src
        assert not re.search(r"\b(depth_at|joined_to|point_of|normal_of|load_coef|check_common)\([^;{]*\)\s*\{", src), name
    vp, i, ll, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_depth_mesh_workspace_bytes", "mg_depth_mesh"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_depth_mesh_workspace_bytes.argtypes == [ll] and lib.mg_depth_mesh_workspace_bytes.restype is ll
        assert lib.mg_depth_mesh.argtypes == [vp, vp, i, vp, vp, i, i] + [dbl] * 7 + [i, ll, ll] + [vp] * 7 + [ll, vp]
    assert len(L.OP_NAMES) == 35 and ctypes.sizeof(L.MgOp) == 360   # a plain C call, no op kind
    assert not any("mesh" in name for name in L.OP_NAMES.values())
    import marigold_amd
    for name in ("HostMesh", "Mesh", "depth_to_mesh", "read_mesh_ply", "write_mesh_ply"):
        assert getattr(marigold_amd, name) is getattr(M, name)


@LIBS
def test_workspace_bytes(f16):
    lib = L.load(f16)
    for n in (0, -1, -(1 << 40), (1 << 30) + 1):
        assert lib.mg_depth_mesh_workspace_bytes(n) == -1
        assert lib.mg_last_error().decode().startswith("mg_depth_mesh_workspace_bytes:")
    sizes = [1, 2, 63, 64, 65, 2047, 2048, 2049, 12319, 768 * 768, 3000 * 4000, 1 << 30]
    got = [lib.mg_depth_mesh_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 16 == 0 for b in got) and got == sorted(got) and got[0] < got[2] < got[6] < got[7] < got[-1]
    # four tables of the chunks of 2048 pixels, a rank per pixel and a byte per cell, rounded up to 16 bytes
    assert got == [(-(-n // 2048) * 32 + 5 * n + 15) // 16 * 16 for n in sizes]


_MESH = ("d", "colors", "hwc", "mask", "coef", "h", "w", "fx", "fy", "cx", "cy", "z_min", "z_max", "edge_rel", "frame", "capacity_v", "capacity_f",
         "xyz", "rgb", "nrm", "index", "faces", "count", "ws", "ws_bytes")


@LIBS
def test_the_mesh_call_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()                      # stands for every device buffer: no call gets as far as reading it
    p = (ctypes.addressof(mem) + 15) // 16 * 16
    need = lib.mg_depth_mesh_workspace_bytes(100)

    def call(**kw):
        a = dict(d=p, colors=p, hwc=1, mask=None, coef=None, h=10, w=10, fx=50.0, fy=50.0, cx=4.5, cy=4.5, z_min=0.0, z_max=INF, edge_rel=0.05, frame=0,
                 capacity_v=100, capacity_f=162, xyz=p, rgb=p, nrm=p, index=p, faces=p, count=p, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.mg_depth_mesh(*(a[k] for k in _MESH), None), lib.mg_last_error().decode()

    def refused(*words, **kw):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("mg_depth_mesh:") and all(w in msg for w in words), (kw, rc, msg)

    for name in ("d", "xyz", "faces", "count", "ws"):
        refused("null pointer", **{name: None})
    refused("go together", colors=None)
    refused("go together", rgb=None)
    for words, kw in _SHARED:          # what mg_depth_points refuses about the map, the camera and the rules
        refused(words, **kw)
    for kw in (dict(capacity_v=0), dict(capacity_v=-1), dict(capacity_f=0), dict(capacity_f=-5)):
        refused("capacities", **kw)
    for kw in (dict(d=p + 2), dict(xyz=p + 2), dict(nrm=p + 1), dict(index=p + 2), dict(faces=p + 2), dict(faces=p + 1), dict(count=p + 4),
               dict(coef=p + 4)):
        refused("aligned to their elements", **kw)
    refused("16-byte aligned", ws=p + 8)
    refused("workspace holds", ws_bytes=need - 1)
    refused("workspace holds", ws_bytes=0)
    refused("workspace holds", ws_bytes=lib.mg_depth_points_workspace_bytes(100))   # a cloud's workspace is too short
    assert list(mem) == [0.0] * 64


# ---- marigold_amd.mesh on the host -------------------------------------------------------------------------------------------------

def _header(vertices, faces, normals, colours):
    names = ["x", "y", "z"] + ["nx", "ny", "nz"] * normals + ["red", "green", "blue"] * colours
    return (f"ply\nformat binary_little_endian 1.0\nelement vertex {vertices}\n"
            + "".join(f"property {'uchar' if n in ('red', 'green', 'blue') else 'float'} {n}\n" for n in names)
            + f"element face {faces}\nproperty list uchar int vertex_indices\nend_header\n")


@pytest.mark.parametrize("normals", [False, True], ids=["bare", "normals"])
@pytest.mark.parametrize("colours", [False, True], ids=["plain", "colours"])
def test_a_mesh_ply_round_trip_byte_for_byte(tmp_path, normals, colours):
    g = np.random.default_rng(3)
    xyz = g.standard_normal((37, 3)).astype(np.float32)
    xyz[0] = (np.inf, -0.0, 1e-42)
    nrm = g.standard_normal((37, 3)).astype(np.float32) if normals else None
    rgb = g.integers(0, 256, (37, 3), dtype=np.uint8) if colours else None
    faces = g.integers(0, 37, (50, 3)).astype(np.int32)
    a, b, c = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "c.ply"
    M.write_mesh_ply(a, xyz, faces, nrm, rgb)
    raw = open(a, "rb").read()
    head = _header(37, 50, normals, colours)
    stride = 12 + 12 * normals + 3 * colours
    assert raw.startswith(head.encode()) and len(raw) == len(head) + 37 * stride + 50 * 13
    assert raw[len(head):len(head) + 12] == xyz[0].tobytes()
    first = raw[len(head) + 37 * stride:][:13]
    assert first[0] == 3 and first[1:] == faces[0].astype("<i4").tobytes()
    # the vertex element is write_ply's, byte for byte
    P.write_ply(c, xyz, nrm, rgb)
    cloud = open(c, "rb").read()
    cut = len(cloud) - 37 * stride
    assert cloud[cut:] == raw[len(head):len(head) + 37 * stride] and cloud[:cut - len("end_header\n")] == raw[:cut - len("end_header\n")]
    mesh = M.read_mesh_ply(a)
    assert (mesh.vertices, mesh.vertices_written, mesh.faces_total, mesh.faces_written, mesh.index) == (37, 37, 50, 50, None)
    assert mesh.xyz.tobytes() == xyz.tobytes() and np.array_equal(mesh.faces, faces) and mesh.faces.dtype == np.int32
    assert (mesh.normals is None) == (not normals) and (mesh.rgb is None) == (not colours)
    assert (not normals or mesh.normals.tobytes() == nrm.tobytes()) and (not colours or np.array_equal(mesh.rgb, rgb))
    mesh.write_ply(b)
    assert open(b, "rb").read() == raw
    M.write_mesh_ply(b, xyz[:0], faces[:0], None if nrm is None else nrm[:0], None if rgb is None else rgb[:0])   # an empty mesh is a file too
    assert open(b, "rb").read() == _header(0, 0, normals, colours).encode()
    empty = M.read_mesh_ply(b)
    assert empty.vertices_written == 0 and empty.faces_written == 0 and empty.faces.shape == (0, 3) and empty.xyz.shape == (0, 3)
    with pytest.raises(ValueError, match="read_mesh_ply"):
        open(b, "wb").write(raw[:-1])
        M.read_mesh_ply(b)
    with pytest.raises(ValueError, match="read_mesh_ply"):
        M.read_mesh_ply(c)                       # a cloud is no mesh
    with pytest.raises(ValueError, match="read_ply"):
        P.read_ply(a)                            # and a mesh no cloud: read_ply keeps its refusals


def test_the_python_call_refuses_what_is_not_a_device_map():
    d = torch.zeros(4, 5)
    for bad in (d, d.numpy(), None):
        with pytest.raises(ValueError, match="depth_to_mesh"):
            M.depth_to_mesh(bad, P.Intrinsics(5.0, 5.0, 2.0, 1.5))


# ---- the command line --------------------------------------------------------------------------------------------------------------

def test_the_parser_flag():
    from marigold_amd import cli
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    assert cli.build_parser("depth").parse_args(io).save_mesh is False
    a = cli.build_parser("depth").parse_args(io + ["--save_mesh", "--fov_deg", "60"])
    assert a.save_mesh is True and a.save_points is False
    for kind in ("normals", "iid"):
        with pytest.raises(SystemExit):
            cli.build_parser(kind).parse_args(io + ["--save_mesh"])
        text = cli.build_parser(kind).format_help()
        assert "mesh" not in text and "points" not in text
    for kind in ("depth", "normals", "iid"):   # the launchers reach the flag through cli.main and do not name it
        src = open(os.path.join(ROOT, "script", kind, "run.py")).read()
        assert "mesh" not in src and "cli" in src


def _restated_mesh(calls):
    """``depth_to_mesh`` with the restatement in the kernel's place: host tensors in, a host mesh out"""
    def fake(depth, K, *, colors=None, coef=None, edge_rel=0.0, normals=False, frame="camera", **kw):
        calls.append(dict(K=K, coef=coef, edge_rel=edge_rel, normals=normals, frame=frame, colors=tuple(colors.shape), **kw))
        r = mesh_reference(depth.numpy(), tuple(K), colors=colors.numpy(), hwc=False, coef=coef, edge_rel=edge_rel, frame=frame)
        return M.HostMesh(r.xyz, r.rgb, r.nrm if normals else None, None, r.faces, *r.count)
    return fake


def _restated_points(calls):
    def fake(depth, K, *, colors=None, coef=None, edge_rel=0.0, normals=False, frame="camera", **kw):
        calls.append(tuple(K))
        r = points_reference(depth.numpy(), tuple(K), colors=colors.numpy(), hwc=False, coef=coef, edge_rel=edge_rel, frame=frame)
        return P.HostPointCloud(r.xyz, r.rgb, r.nrm if normals else None, None, *r.count)
    return fake


def test_cli_main_writes_the_mesh(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    g = np.random.default_rng(1)
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(g.integers(0, 256, (6, 8, 3), dtype=np.uint8)).save(inp / "b.png")      # the map's size
    Image.fromarray(g.integers(0, 256, (12, 16, 3), dtype=np.uint8)).save(inp / "a.png")    # twice the map's size
    out = tmp_path / "out"
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(out)]
    calls, cloud_calls = [], []
    monkeypatch.setattr(M, "depth_to_mesh", _restated_mesh(calls))
    monkeypatch.setattr(P, "depth_to_points", _restated_points(cloud_calls))
    # without the flag nothing changes: no folder, no call - with --save_points alone too
    pipe = _FakeCliPipe()
    assert cli.main("depth", base, pipeline=pipe) == 0
    assert calls == [] and sorted(os.listdir(out)) == ["depth_bw", "depth_colored", "depth_npy"]
    assert cli.main("depth", base + ["--save_points", "--fov_deg", "60"], pipeline=_FakeCliPipe()) == 0
    assert calls == [] and len(cloud_calls) == 2 and not (out / "depth_mesh").exists()
    depth = pipe._out().depth_np
    for extra, video in ((["--maps_in_flight", "2"], False), (["--sequence"], True)):
        for normals, with_points in ((False, False), (True, True)):
            del calls[:], cloud_calls[:]
            pipe = _FakeCliPipe()
            argv = base + extra + ["--save_mesh", "--fov_deg", "60", "--points_near", "2", "--points_far", "6"] + ["--points_normals"] * normals \
                + ["--save_points"] * with_points
            assert cli.main("depth", argv, pipeline=pipe) == 0
            assert pipe.calls[0][0] == ("map_video" if video else "map_images") and "mesh" not in " ".join(pipe.calls[0][2])
            assert sorted(os.listdir(out / "depth_mesh")) == ["a_mesh.ply", "b_mesh.ply"]
            assert len(cloud_calls) == 2 * with_points
            assert [c["colors"] for c in calls] == [(3, 6, 8)] * 2 and all(c["coef"] == (4.0, 2.0) and c["edge_rel"] == 0.05 for c in calls)
            big, small = P.intrinsics_from_fov(12, 16, 60.0), P.intrinsics_from_fov(6, 8, 60.0)
            assert calls[0]["K"] == P.scale_intrinsics(big, (12, 16), (6, 8)) and calls[1]["K"] == small   # (sorted: a.png first)
            for name, c in zip(("a", "b"), calls):
                raw = open(out / "depth_mesh" / f"{name}_mesh.ply", "rb").read()
                want = mesh_reference(depth, tuple(c["K"]), coef=(4.0, 2.0), edge_rel=0.05)
                V, _, F, _ = want.count
                assert V == 48 and F == 2 * 5 * 6                 # the step of the stand-in map costs a column of cells and no vertex
                head = _header(V, F, normals, True)
                assert raw.startswith(head.encode()) and len(raw) == len(head) + V * (27 if normals else 15) + F * 13
                mesh = M.read_mesh_ply(out / "depth_mesh" / f"{name}_mesh.ply")
                assert mesh.xyz.tobytes() == want.xyz.tobytes() and np.array_equal(mesh.faces, want.faces) and (mesh.normals is not None) == normals
    b = np.array(Image.open(inp / "b.png"))
    assert np.array_equal(M.read_mesh_ply(out / "depth_mesh" / "b_mesh.ply").rgb, b.reshape(-1, 3)[want.index])


def test_cli_refusals(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from marigold_amd import cli
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / "a.png")
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    calls = []
    monkeypatch.setattr(M, "depth_to_mesh", _restated_mesh(calls))
    pipe = _FakeCliPipe()
    with pytest.raises(ValueError, match="--save_mesh cannot be combined with --tile_size"):
        cli.main("depth", base + ["--save_mesh", "--fov_deg", "60", "--tile_size", "64"], pipeline=pipe)
    for extra, word in ((["--save_mesh"], "exactly one of"), (["--save_mesh", "--fov_deg", "60", "--focal_px", "100"], "exactly one of"),
                        (["--save_mesh", "--fov_deg", "180"], "--fov_deg"), (["--save_mesh", "--focal_px", "0"], "--focal_px"),
                        (["--save_mesh", "--fov_deg", "60", "--points_near", "3", "--points_far", "2"], "near < far"),
                        (["--save_mesh", "--fov_deg", "60", "--points_edge_rel", "-1"], "--points_edge_rel")):
        with pytest.raises(SystemExit) as e:
            cli.main("depth", base + extra, pipeline=pipe)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert pipe.calls == [] and calls == []
    assert cli.main("depth", base + ["--save_mesh", "--focal_px", "9"], pipeline=pipe) == 0
    assert calls[0]["K"] == P.Intrinsics(9.0, 9.0, 3.5, 2.5)


# ---- the C host example ------------------------------------------------------------------------------------------------------------

def test_the_c_host_example_compiles(tmp_path):
    c_hosts.compile_only(os.path.join(ROOT, "examples", "host_mesh.cpp"), tmp_path / "host_mesh.o")
    assert os.path.getsize(tmp_path / "host_mesh.o") > 0
    assert "host_mesh" in open(os.path.join(ROOT, "README.md")).read()
