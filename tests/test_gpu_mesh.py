"""``mg_depth_mesh`` (csrc/mesh.hip) on a real MI355X, both operand libraries, against the numpy float64 restatement of
tests/mesh_reference.py.

The ladder: maps of 1x1, 1x5, 5x1 (no cells); 2x2, 2x3, 3x3; 2x63, 2x64, 2x65, 7x65 (cells whose corners sit in different waves);
2 x (C/2 - 1), 2 x C/2, 2 x (C/2 + 1) and 3 x C (C = 2048, the chunk of the counts and the scatters: cells whose lower corners lie in
the next chunk); 97x127; and 513x1025 (257 chunks: more than the S = 256 lanes of the scan launch).  The scenes are those of
tests/test_gpu_points.py - a smooth surface with a 30 % and a 20 % step, NaN and +-inf planted, values at and just beyond both ends of
the range - with a flat patch planted for the tie of the split rule.  Each small shape meets six masks - none, all zero, every second
pixel (no cell reaches three usable corners), a random half, one pixel per chunk, one corner of every second cell - and the options
rotate over the cases so that every combination of coef / no coef, edge_rel 0 / 0.05, both frames and both colour layouts occurs.
Before anything runs on the device the restatement is asked, on the CPU, whether the scenes do their job.

Equality everywhere but the normals: count, faces, index, rgb and the fp32 bits of xyz.  The normals get 1 fp32 ulp, 6h's bound for
6h's reason: the one operation not known to be correctly rounded on both sides is the fp64 square root, and a last-place fp64
difference of the quotient moves the fp32 rounding by one step at the most.  The test prints how many components differ at all."""
import functools
import math

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests.mesh_reference import NO_A, NO_B, NO_C, NO_D, SPLIT_AD, SPLIT_BC, mesh_reference
from tests.test_gpu_points import CANARY, COEF, OPTIONS, Z_RANGE, _camera, _dev, _Padded, _ptr, _same_bits, _scene, _ulps

gpu = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
CHUNK, SCAN_LANES = 2048, 256   # MESH_CHUNK, MESH_SCAN_LANES of csrc/mesh.hip
SMALL = ((1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (3, 3), (2, 63), (2, 64), (2, 65), (7, 65), (2, CHUNK // 2 - 1), (2, CHUNK // 2),
         (2, CHUNK // 2 + 1), (3, CHUNK), (97, 127))
BIG = (513, 1025)
assert math.ceil(BIG[0] * BIG[1] / CHUNK) > SCAN_LANES
MASKS = ("none", "zero", "second", "half", "per_chunk", "corner")
CUT_SHAPES = ((7, 65), (2, CHUNK // 2 + 1), (97, 127))


def _mesh_scene(h, w, coef):
    """the points' scene with a flat patch of 3 x 3 pixels (2 x 2 where the map is smaller) in its upper left quarter: cells whose two
    diagonal differences are equal"""
    d, colors = _scene(h, w, coef)
    if h >= 2 and w >= 2:
        y, x = (h // 2 - 3) // 2 if h >= 8 else 0, (w // 2 - 3) // 2 if w >= 8 else 0
        d[y:y + 3, x:x + 3] = np.float32(2.0 if coef is None else (2.0 - coef[1]) / coef[0])
    return d, colors


def _mask(kind, h, w):
    n = h * w
    g = np.random.default_rng(900 + n)
    if kind == "none":
        return None
    if kind == "corner":   # odd rows, every fourth column: half of the cells lose one corner, each of the four in turn
        m = np.ones((h, w), np.uint8)
        m[1::2, 3::4] = 0
        return m
    m = np.zeros(n, np.uint8)
    if kind == "second":
        m[::2] = 1          # (a checkerboard for an odd width, stripes for an even one: two corners of every cell either way)
    elif kind == "half":
        pick = g.random(n) < 0.5
        m[pick] = g.integers(1, 256, int(pick.sum()), dtype=np.uint8)   # any non-zero byte counts
    elif kind == "per_chunk":
        for c in range(0, n, CHUNK):
            m[c + int(g.integers(0, min(CHUNK, n - c)))] = 255
    return m.reshape(h, w)


@functools.lru_cache(maxsize=None)
def _cases():
    """[(name, d, colors in the option's layout, mask, K, options, the restatement's result)] - computed once, on the CPU"""
    cases, k = [], 0
    for (h, w), masks in [(s, MASKS) for s in SMALL] + [(BIG, ("none", "half"))]:
        for kind in masks:
            coef, edge, frame, hwc = opt = OPTIONS[k % len(OPTIONS)]
            k += 5   # (5 and 16 are coprime: the rotation visits every combination)
            d, colors = _mesh_scene(h, w, coef)
            mask, K = _mask(kind, h, w), _camera(h, w)
            want = mesh_reference(d, K, colors=colors, hwc=True, mask=mask, coef=coef, z_range=Z_RANGE, edge_rel=edge, frame=frame)
            lay = colors if hwc else np.ascontiguousarray(colors.transpose(2, 0, 1))
            cases.append((f"{h}x{w}/{kind}/{opt}", d, lay, mask, K, opt, want))
    return cases


def test_the_scenes_do_their_job():
    """asked of the restatement alone, on the CPU, before the device is trusted with anything"""
    cases = _cases()
    assert {c[5] for c in cases} == set(OPTIONS)
    for form in (SPLIT_AD, SPLIT_BC):       # both splits produce faces, and some split is a tie
        assert any(((c[6].form == form) & c[6].t0).any() and ((c[6].form == form) & c[6].t1).any() for c in cases), form
    assert any((c[6].tie & c[6].t0 & c[6].t1).any() for c in cases)
    assert not any((c[6].tie & (c[6].form != SPLIT_AD)).any() for c in cases)           # the tie goes to A-D
    for form in (NO_D, NO_A, NO_B, NO_C):   # every three-corner form gives a face somewhere, in slot T0 alone
        assert any(((c[6].form == form) & c[6].t0).any() for c in cases), form
        assert not any(((c[6].form == form) & c[6].t1).any() for c in cases), form
    for kept in (0, 1, 2):
        assert any((c[6].kept4 == kept).any() for c in cases), kept
    assert any((c[6].usable & ~c[6].vertex).any() for c in cases)                       # a usable pixel that is no vertex
    assert any((c[6].vertex & ~c[6].has_normal).any() for c in cases)                   # a vertex without a normal
    assert any(c[6].count[0] == 0 and c[6].usable.any() for c in cases) and any(c[6].count[0] == c[1].size and c[1].size > 1 for c in cases)
    for c in cases:
        h, w = c[1].shape
        if min(h, w) == 1 or "/second/" in c[0] or "/zero/" in c[0] or "/per_chunk/" in c[0]:
            assert c[6].count == (0, 0, 0, 0), c[0]
        assert c[6].count[1] == c[6].count[0] and c[6].count[3] == c[6].count[2], c[0]
    big = [c for c in cases if c[1].shape == BIG]
    assert big and all(c[6].count[0] > SCAN_LANES and c[6].count[2] > SCAN_LANES for c in big)   # both tables exceed the scan's lanes
    for shape in CUT_SHAPES:
        assert sum(c[1].shape == shape and c[6].count[0] >= 3 and c[6].count[2] >= 3 for c in cases) >= 2, shape


def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


def _mesh(lib, d, colors, mask, K, opt, cap_v, cap_f, off=0, coef_dev=None, stream=None):
    """one raw mg_depth_mesh -> dict of the outputs as numpy (whole buffers of the capacities, canaries past what was written)"""
    coef, edge, frame, hwc = opt
    h, w = d.shape
    n = h * w
    dd = _Padded(np.float32, n, off, d)
    cc, mm = _dev(colors), _dev(mask)
    if coef_dev is None and coef is not None:
        coef_buf = _Padded(np.float64, 2, off, coef)
        coef_dev = coef_buf.view
    need = lib.mg_depth_mesh_workspace_bytes(n)
    assert need > 0
    ws = _Padded(np.uint8, need)
    xyz, rgb, nrm = _Padded(np.float32, 3 * cap_v, off), _Padded(np.uint8, 3 * cap_v, off), _Padded(np.float32, 3 * cap_v, off)
    index, faces, count = _Padded(np.int32, cap_v, off), _Padded(np.int32, 3 * cap_f, off), _Padded(np.int64, 4, off)
    rc = lib.mg_depth_mesh(dd.ptr(), _ptr(cc), int(hwc), _ptr(mm), _ptr(coef_dev), h, w, *K, Z_RANGE[0], Z_RANGE[1], edge, L.NORMALS_FRAME[frame],
                           cap_v, cap_f, xyz.ptr(), rgb.ptr(), nrm.ptr(), index.ptr(), faces.ptr(), count.ptr(), ws.ptr(), need, stream)
    assert rc == 0, lib.mg_last_error().decode()
    torch.cuda.synchronize()
    ws.read()
    assert np.array_equal(dd.read().view(np.uint32), d.reshape(-1).view(np.uint32))   # the inputs are left alone
    assert cc is None or np.array_equal(cc.cpu().numpy(), colors)
    assert mm is None or np.array_equal(mm.cpu().numpy(), mask)
    return dict(xyz=xyz.read().reshape(cap_v, 3), rgb=rgb.read().reshape(cap_v, 3), nrm=nrm.read().reshape(cap_v, 3), index=index.read(),
                faces=faces.read().reshape(cap_f, 3), count=count.read())


@functools.lru_cache(maxsize=None)
def _ladder(f16):
    """every case on the device; the capacities leave three records past what a map can hold"""
    lib = _lib(f16)
    return [_mesh(lib, d, colors, mask, K, opt, d.size + 3, 2 * (d.shape[0] - 1) * (d.shape[1] - 1) + 3) for _, d, colors, mask, K, opt, _ in _cases()]


def _canaries_past(got, vertices, faces):
    return all((got[k][vertices if k != "faces" else faces:] == np.asarray(CANARY[got[k].dtype], got[k].dtype)).all()
               for k in ("xyz", "rgb", "nrm", "index", "faces"))


@gpu
@LIBS
def test_the_ladder_against_the_restatement(f16):
    cases, runs = _cases(), _ladder(f16)
    differing = components = vertices = faces = 0
    for (name, d, _, _, _, _, want), got in zip(cases, runs):
        V, Vw, F, Fw = want.count
        assert got["count"].tolist() == [V, Vw, F, Fw], name
        assert np.array_equal(got["faces"][:Fw], want.faces), name
        assert np.array_equal(got["index"][:Vw], want.index), name
        assert np.array_equal(got["rgb"][:Vw], want.rgb), name
        assert _same_bits(got["xyz"][:Vw], want.xyz), name
        assert _canaries_past(got, Vw, Fw), name
        u = _ulps(got["nrm"][:Vw], want.nrm)
        assert np.isfinite(got["nrm"][:Vw]).all() and u.max(initial=0) <= 1, (name, int(u.max(initial=0)))
        differing += int((u != 0).sum())
        components += u.size
        vertices += Vw
        faces += Fw
    print(f"[mesh] {len(cases)} cases, {vertices} vertices, {faces} faces, {components} normal components compared, {differing} differ from "
          f"the restatement (by one fp32 step)")


@gpu
def test_two_runs_and_the_two_libraries_give_the_same_bytes():
    def raw(runs):
        return [np.ascontiguousarray(got[k]).tobytes() for got in runs for k in sorted(got)]
    a = raw(_ladder(False))
    _ladder.cache_clear()
    assert raw(_ladder(False)) == a and raw(_ladder(True)) == a


@gpu
@LIBS
def test_a_face_capacity_below_the_faces_cuts_the_faces_and_not_the_counts(f16):
    lib = _lib(f16)
    tried = 0
    for name, d, colors, mask, K, opt, want in _cases():
        V, _, F, _ = want.count
        if d.shape not in CUT_SHAPES or V < 3 or F < 3:
            continue
        for cap_f in (F - 1, 1):
            got = _mesh(lib, d, colors, mask, K, opt, V, cap_f)   # (the pads behind the last record stand for "past the capacity")
            assert got["count"].tolist() == [V, V, F, cap_f], (name, cap_f)
            assert np.array_equal(got["faces"], want.faces[:cap_f]), (name, cap_f)
            assert np.array_equal(got["index"], want.index) and _same_bits(got["xyz"], want.xyz) and np.array_equal(got["rgb"], want.rgb), (name, cap_f)
            tried += 1
    assert tried >= 12


@gpu
@LIBS
def test_a_vertex_capacity_below_the_vertices_leaves_no_face(f16):
    lib = _lib(f16)
    tried = 0
    for name, d, colors, mask, K, opt, want in _cases():
        V, _, F, _ = want.count
        if d.shape not in CUT_SHAPES or V < 3 or F < 3:
            continue
        for cap_v in (V - 1, 1):
            got = _mesh(lib, d, colors, mask, K, opt, cap_v, F + 3)
            assert got["count"].tolist() == [V, cap_v, F, 0], (name, cap_v)
            assert (got["faces"] == CANARY[np.dtype(np.int32)]).all(), (name, cap_v)          # no face written
            assert np.array_equal(got["index"], want.index[:cap_v]) and _same_bits(got["xyz"], want.xyz[:cap_v]), (name, cap_v)
            assert np.array_equal(got["rgb"], want.rgb[:cap_v]) and _ulps(got["nrm"], want.nrm[:cap_v]).max() <= 1, (name, cap_v)
            tried += 1
    assert tried >= 12


@gpu
@LIBS
def test_pointers_one_element_off_a_16_byte_boundary(f16):
    lib = _lib(f16)
    picked = [i for i, c in enumerate(_cases()) if c[1].shape in ((7, 65), (97, 127)) and c[6].count[0] > 0]
    assert len(picked) >= 6
    for i in picked:
        name, d, colors, mask, K, opt, _ = _cases()[i]
        got = _ladder(f16)[i]
        off = _mesh(lib, d, colors, mask, K, opt, d.size + 3, 2 * (d.shape[0] - 1) * (d.shape[1] - 1) + 3, off=1)
        assert all(np.array_equal(off[k].view(np.uint8), got[k].view(np.uint8)) for k in got), name


@gpu
@LIBS
def test_coef_straight_from_the_alignment_fit(f16):
    """the device coefficients mg_depth_align_fit leaves feed the mesh; the same two numbers uploaded give the same bytes"""
    lib = _lib(f16)
    h, w = 97, 127
    d, colors = _mesh_scene(h, w, COEF)
    g = np.random.default_rng(5)
    ref = (d.astype(np.float64) * 1.3 - 0.45 + 0.01 * g.standard_normal((h, w))).astype(np.float32)
    ref[~np.isfinite(ref)] = 2.0
    coef = torch.empty(2, dtype=torch.float64, device="cuda")
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    need = lib.mg_depth_align_workspace_bytes(h * w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dd, rr = _dev(d), _dev(ref)
    rc = lib.mg_depth_align_fit(dd.data_ptr(), rr.data_ptr(), None, h * w, 1, 4, L.ALIGN_START_LS, 1.0, 0.0, 0.05, coef.data_ptr(),
                                flag.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, lib.mg_last_error().decode()
    opt, K = (COEF, 0.05, "marigold", True), _camera(h, w)
    cap_f = 2 * (h - 1) * (w - 1)
    straight = _mesh(lib, d, colors, None, K, opt, h * w, cap_f, coef_dev=coef)
    s, t = coef.cpu().tolist()
    assert flag.item() == 0 and abs(s - 1.3) < 0.05 and abs(t + 0.45) < 0.05
    uploaded = _mesh(lib, d, colors, None, K, ((s, t),) + opt[1:], h * w, cap_f)
    assert all(np.array_equal(straight[k].view(np.uint8), uploaded[k].view(np.uint8)) for k in straight)
    want = mesh_reference(d, K, colors=colors, coef=(s, t), z_range=Z_RANGE, edge_rel=0.05, frame="marigold")
    V, _, F, _ = want.count
    assert straight["count"].tolist() == list(want.count) and V > h * w // 2 and F > h * w // 2
    assert _same_bits(straight["xyz"][:V], want.xyz) and np.array_equal(straight["index"][:V], want.index)
    assert np.array_equal(straight["faces"][:F], want.faces)


@gpu
@LIBS
def test_the_python_layer_returns_what_the_raw_call_writes(f16):
    from marigold_amd import Intrinsics, Mesh, depth_to_mesh
    lib = _lib(f16)
    picked = [i for i, c in enumerate(_cases()) if c[1].shape in ((1, 5), (3, 3), (7, 65), (97, 127))]
    for i in picked:
        name, d, colors, mask, K, (coef, edge, frame, hwc), want = _cases()[i]
        got = _ladder(f16)[i]
        V, _, F, _ = want.count
        coef_arg = coef if i % 2 else (None if coef is None else torch.tensor(coef, dtype=torch.float64, device="cuda"))
        mask_arg = None if mask is None else (_dev(mask) if i % 2 else _dev(mask) != 0)
        if d.shape == (3, 3) and not hwc:
            colors = colors.transpose(1, 2, 0)   # ([3, 3, 3] is read as [h, w, 3])
        mesh = depth_to_mesh(_dev(d), Intrinsics(*K), colors=_dev(colors), mask=mask_arg, coef=coef_arg, z_range=Z_RANGE, edge_rel=edge,
                             normals=True, frame=frame, index=True, lib=lib)
        assert isinstance(mesh, Mesh) and mesh.xyz.shape == (d.size, 3) and mesh.faces.shape == (max(1, 2 * (d.shape[0] - 1) * (d.shape[1] - 1)), 3)
        assert mesh.count.dtype == torch.int64 and mesh.count.is_cuda and mesh.count.shape == (4,) and mesh.faces.dtype == torch.int32
        host = mesh.to_host()
        assert (host.vertices, host.vertices_written, host.faces_total, host.faces_written) == want.count, name
        assert _same_bits(host.xyz, got["xyz"][:V]) and _same_bits(host.normals, got["nrm"][:V]), name
        assert np.array_equal(host.rgb, got["rgb"][:V]) and np.array_equal(host.index, got["index"][:V]), name
        assert np.array_equal(host.faces, got["faces"][:F]) and host.faces.shape == (F, 3), name
        bare = depth_to_mesh(_dev(d), K, mask=mask_arg, coef=coef_arg, z_range=Z_RANGE, edge_rel=edge, face_capacity=max(1, F // 2), lib=lib)
        assert bare.rgb is None and bare.normals is None and bare.index is None
        half = bare.to_host()
        assert (half.vertices, half.vertices_written, half.faces_total, half.faces_written) == (V, V, F, min(F, max(1, F // 2))), name
        assert _same_bits(half.xyz, got["xyz"][:V]) and np.array_equal(half.faces, got["faces"][:half.faces_written]), name
        if V > 1:
            cut = depth_to_mesh(_dev(d), K, mask=mask_arg, coef=coef_arg, z_range=Z_RANGE, edge_rel=edge, capacity=V - 1, lib=lib).to_host()
            assert (cut.vertices, cut.vertices_written, cut.faces_total, cut.faces_written) == (V, V - 1, F, 0) and cut.faces.shape == (0, 3), name
    d = _dev(_cases()[picked[-1]][1])
    K = _cases()[picked[-1]][4]
    for bad in (dict(z_range=(2.0, 1.0)), dict(z_range=(-1.0, 2.0)), dict(edge_rel=-0.1), dict(frame="world"), dict(capacity=0),
                dict(face_capacity=0), dict(face_capacity=2.5), dict(coef=(1.0,)), dict(mask=torch.ones(3, 3, device="cuda")),
                dict(colors=torch.zeros(3, 3, 3, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError, match="depth_to_mesh"):
            depth_to_mesh(d, K, lib=lib, **bad)
    with pytest.raises(ValueError, match="depth_to_mesh"):
        depth_to_mesh(d, (0.0, 1.0, 0.0, 0.0), lib=lib)
    with pytest.raises(ValueError, match="depth_to_mesh"):
        depth_to_mesh(d.cpu(), K, lib=lib)
