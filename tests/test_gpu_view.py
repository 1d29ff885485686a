"""``mg_depth_view`` (csrc/view.hip) on a real MI355X, both operand libraries, against the numpy restatement of tests/view_reference.py.

The scenes are those of tests/view_scenes.py, of which tests/test_view_host.py asks, on the CPU, whether they reach every branch:
source maps of 1x1, 1x7 (no cells), 2x2, 3x5, 17x33, 64x67 and 129x257 (more than one workgroup of the splat and of the resolve, rows
that straddle workgroups) - the meshes' scene, a smooth surface with a 30 % and a 20 % step, NaN and +-inf planted - under eight poses:
the identity, the two eyes of a stereo pair, a 0.3 rad turn with a shift, a forward move that puts part of the scene behind z_near, a
mirror (every face back), a 50-fold zoom after a forward move (near cells pass the span cap, far ones do not) and a million-fold zoom
(corners leave the snapping range).  Targets equal to the map, smaller, larger, 1 x 1 and wide; masks none, a random half and one
corner of every second cell; ``coef`` or none, ``edge_rel`` 0 and 0.05, both colour layouts, ``fill_radius`` 0, 3 and 64, ``face``
given and NULL rotate over the cases.

Equality everywhere: ``rgb``, the bits of ``depth``, ``valid``, ``face`` and all eight counts.  Every operation of the definitions is
an fp64 product, sum or quotient, an exact conversion, a rounding to fp32 or integer arithmetic - correctly rounded on both sides - so
there is no tolerance to choose.  The pads around every output and the workspace keep their canaries, the inputs are untouched, a
workspace pre-filled with other garbage gives the same bytes, so do two runs and the two libraries, and pointers one element off a
16-byte boundary change nothing."""
import functools

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests.test_gpu_points import _dev, _Padded, _ptr, Z_RANGE
from tests.view_scenes import cases, NO_SPAN, Z_NEAR

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
KEYS = ("rgb", "depth", "valid", "face", "count")


def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


def _view(lib, c, off=0, garbage=None, coef_dev=None, face=None, stream=None):
    """one raw mg_depth_view of case ``c`` -> dict of the outputs as numpy (``face`` None where it was not asked for)"""
    coef, edge, hwc = c.opt
    (h, w), (h2, w2) = c.shape, c.size
    n, n2 = h * w, h2 * w2
    dd = _Padded(np.float32, n, off, c.d)
    cc, mm = _Padded(np.uint8, 3 * n, off, c.colors), _dev(c.mask)
    if coef_dev is None and coef is not None:
        coef_buf = _Padded(np.float64, 2, off, coef)
        coef_dev = coef_buf.view
    need = lib.mg_depth_view_workspace_bytes(n2)
    assert need == (8 * n2 + 15) // 16 * 16
    ws = _Padded(np.uint8, need, 0, garbage)
    rgb, depth, valid = _Padded(np.uint8, 3 * n2, off), _Padded(np.float32, n2, off), _Padded(np.uint8, n2, off)
    want_face = c.face if face is None else face
    fmap, count = _Padded(np.int32, n2, off), _Padded(np.int64, 8, off)
    pose = None if c.pose is None else np.ascontiguousarray(c.pose, np.float64)
    rc = lib.mg_depth_view(dd.ptr(), cc.ptr(), int(hwc), _ptr(mm), _ptr(coef_dev), h, w, *c.K, Z_RANGE[0], Z_RANGE[1], edge,
                           None if pose is None else pose.ctypes.data, *c.K_out, h2, w2, Z_NEAR, c.fill, rgb.ptr(), depth.ptr(), valid.ptr(),
                           fmap.ptr() if want_face else None, count.ptr(), ws.ptr(), need, stream)
    assert rc == 0, lib.mg_last_error().decode()
    torch.cuda.synchronize()
    ws.read()
    assert np.array_equal(dd.read().view(np.uint32), c.d.reshape(-1).view(np.uint32))   # the inputs are left alone
    assert np.array_equal(cc.read(), c.colors.reshape(-1))
    assert mm is None or np.array_equal(mm.cpu().numpy(), c.mask)
    got_face = fmap.read()
    if not want_face:
        assert (got_face == got_face[0]).all() and got_face[0] == -77777                # untouched
    return dict(rgb=rgb.read().reshape((h2, w2, 3) if hwc else (3, h2, w2)), depth=depth.read().reshape(h2, w2), valid=valid.read().reshape(h2, w2),
                face=got_face.reshape(h2, w2) if want_face else None, count=count.read())


@functools.lru_cache(maxsize=None)
def _ladder(f16):
    lib = _lib(f16)
    return [_view(lib, c) for c in cases()]


def _raw(got):
    return [b"" if got[k] is None else np.ascontiguousarray(got[k]).tobytes() for k in KEYS]


@LIBS
def test_the_ladder_against_the_restatement(f16):
    cs = cases()
    for c in cs:   # the cap cannot hide a failure: where no face may reach it, the restatement's count is zero
        if c.pose_name in NO_SPAN:
            assert c.want.count[5] == 0, c.name
    faces = drawn = covered = filled = 0
    for c, got in zip(cs, _ladder(f16)):
        want = c.want
        assert got["count"].tolist() == list(want.count), c.name
        assert np.array_equal(got["valid"], want.valid), c.name
        assert got["face"] is None or np.array_equal(got["face"], want.face), c.name
        assert np.array_equal(got["depth"].view(np.uint32), want.depth.view(np.uint32)), c.name
        assert np.array_equal(got["rgb"], want.rgb), c.name
        faces, drawn, covered, filled = faces + want.count[0], drawn + want.count[1], covered + want.count[6], filled + want.count[7]
    print(f"[view] {len(cs)} cases, {faces} faces, {drawn} drawn, {covered} pixels covered, {filled} filled: every byte equals the restatement")


def test_two_runs_and_the_two_libraries_give_the_same_bytes():
    a = [_raw(got) for got in _ladder(False)]
    _ladder.cache_clear()
    assert [_raw(got) for got in _ladder(False)] == a and [_raw(got) for got in _ladder(True)] == a


@LIBS
def test_a_workspace_full_of_garbage_and_pointers_off_a_16_byte_boundary(f16):
    lib = _lib(f16)
    picked = [i for i, c in enumerate(cases()) if c.shape in ((17, 33), (64, 67)) and c.want.count[0] > 0]
    assert len(picked) >= 12
    g = np.random.default_rng(11)
    for i in picked:
        c, got = cases()[i], _ladder(f16)[i]
        need = lib.mg_depth_view_workspace_bytes(c.size[0] * c.size[1])
        for other in (_view(lib, c, garbage=g.integers(0, 256, need, dtype=np.uint8)), _view(lib, c, garbage=np.zeros(need, np.uint8)),
                      _view(lib, c, off=1)):
            assert _raw(other) == _raw(got), c.name
        if c.face:   # the face map is an extra: without it the other outputs are the same
            bare = _view(lib, c, face=False)
            assert bare["face"] is None and _raw(dict(bare, face=got["face"])) == _raw(got), c.name


@LIBS
def test_coef_straight_from_the_alignment_fit(f16):
    """the device coefficients mg_depth_align_fit leaves feed the view; the same two numbers uploaded give the same bytes, and the
    restatement's"""
    from tests.view_reference import view_reference
    lib = _lib(f16)
    c = next(c for c in cases() if c.shape == (64, 67) and c.pose_name == "stereo_left")
    h, w = c.shape
    g = np.random.default_rng(5)
    ref = (c.d.astype(np.float64) * 1.3 - 0.45 + 0.01 * g.standard_normal((h, w))).astype(np.float32)
    ref[~np.isfinite(ref)] = 2.0
    coef = torch.empty(2, dtype=torch.float64, device="cuda")
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    need = lib.mg_depth_align_workspace_bytes(h * w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dd, rr = _dev(c.d), _dev(ref)
    rc = lib.mg_depth_align_fit(dd.data_ptr(), rr.data_ptr(), None, h * w, 1, 4, L.ALIGN_START_LS, 1.0, 0.0, 0.05, coef.data_ptr(),
                                flag.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, lib.mg_last_error().decode()
    straight = _view(lib, c, coef_dev=coef)
    s, t = coef.cpu().tolist()
    assert flag.item() == 0 and abs(s - 1.3) < 0.05 and abs(t + 0.45) < 0.05
    from types import SimpleNamespace
    uploaded = _view(lib, SimpleNamespace(**dict(vars(c), opt=((s, t),) + c.opt[1:])))
    assert _raw(straight) == _raw(uploaded)
    want = view_reference(c.d, c.K, c.colors, hwc=c.opt[2], mask=c.mask, coef=(s, t), z_range=Z_RANGE, edge_rel=c.opt[1], pose=c.pose, K_out=c.K_out,
                          size=c.size, z_near=Z_NEAR, fill_radius=c.fill)
    assert straight["count"].tolist() == list(want.count) and want.count[6] > 100
    assert np.array_equal(straight["rgb"], want.rgb) and np.array_equal(straight["depth"].view(np.uint32), want.depth.view(np.uint32))
    assert np.array_equal(straight["valid"], want.valid)


@LIBS
def test_the_python_layer_returns_what_the_raw_call_writes(f16):
    from marigold_amd import Intrinsics, View, render_view, stereo_pair
    lib = _lib(f16)
    picked = [i for i, c in enumerate(cases()) if c.shape in ((1, 7), (3, 5), (17, 33), (64, 67))]
    for i in picked:
        c, got = cases()[i], _ladder(f16)[i]
        coef, edge, hwc = c.opt
        coef_arg = coef if i % 2 else (None if coef is None else torch.tensor(coef, dtype=torch.float64, device="cuda"))
        mask_arg = None if c.mask is None else (_dev(c.mask) if i % 2 else _dev(c.mask) != 0)
        pose = c.pose if i % 2 or c.pose is None else (c.pose[:, :3], c.pose[:, 3])
        view = render_view(_dev(c.d), Intrinsics(*c.K), _dev(c.colors), pose=pose, K_out=c.K_out, size=c.size, coef=coef_arg, mask=mask_arg,
                           z_range=Z_RANGE, edge_rel=edge, z_near=Z_NEAR, fill_radius=c.fill, faces=c.face, lib=lib)
        assert isinstance(view, View) and view.count.dtype == torch.int64 and view.count.is_cuda and view.count.shape == (8,)
        assert tuple(view.depth.shape) == c.size and view.valid.dtype == torch.uint8 and (view.face is None) == (not c.face)
        assert _raw(dict(rgb=view.rgb.cpu().numpy(), depth=view.depth.cpu().numpy(), valid=view.valid.cpu().numpy(),
                         face=None if view.face is None else view.face.cpu().numpy(), count=view.count.cpu().numpy())) == _raw(got), c.name
        host = view.to_host()
        assert np.array_equal(host.rgb, got["rgb"] if hwc else got["rgb"].transpose(1, 2, 0)) and host.rgb.shape == c.size + (3,), c.name
        assert list(host.count.values()) == got["count"].tolist() and list(host.count) == ["faces", "drawn", "near", "off", "back", "span", "covered", "filled"]
    c = next(c for c in cases() if c.shape == (17, 33) and c.pose_name == "identity")
    d, colors, K = _dev(c.d), _dev(c.colors), c.K
    left, right = stereo_pair(d, K, colors, 0.24, z_range=Z_RANGE, edge_rel=0.0, fill_radius=3, lib=lib)
    for eye, tx in ((left, 0.12), (right, -0.12)):
        same = render_view(d, K, colors, pose=(np.eye(3), (tx, 0.0, 0.0)), z_range=Z_RANGE, edge_rel=0.0, fill_radius=3, lib=lib)
        assert all(torch.equal(a, b) for a, b in zip(eye[:3] + eye[4:], same[:3] + same[4:])) and eye.face is None
    assert not torch.equal(left.rgb, right.rgb)
    for bad in (dict(z_range=(2.0, 1.0)), dict(edge_rel=-0.1), dict(z_near=0.0), dict(z_near=float("nan")), dict(fill_radius=65), dict(fill_radius=-1),
                dict(fill_radius=2.0), dict(size=(0, 4)), dict(size=(3, 2.5)), dict(K_out=(0.0, 1.0, 0.0, 0.0)), dict(K_out=(1.0, 1.0)),
                dict(pose=np.eye(4)), dict(pose=(np.eye(3), (0.0, float("inf"), 0.0))), dict(coef=(1.0,)), dict(mask=torch.ones(3, 3, device="cuda"))):
        with pytest.raises(ValueError, match="render_view"):
            render_view(d, K, colors, lib=lib, **bad)
    for bad in (colors.cpu(), colors[:-1], colors.float(), None):
        with pytest.raises(ValueError, match="render_view"):
            render_view(d, K, bad, lib=lib)
