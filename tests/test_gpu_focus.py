"""``mg_depth_focus`` (csrc/focus.hip) on a real MI355X, both operand libraries, against the numpy restatement of tests/focus_reference.py.

The scenes are those of tests/focus_scenes.py, of which tests/test_focus_host.py asks, on the CPU, whether they reach every branch:
pictures of 1 x 1, 1 x 9, 9 x 1, one less and one more than the gather tile's 8 rows and 32 columns in each direction, 20 x 24 (smaller
than the halo at max_radius = 32), 70 x 90 at max_radius = 32 and 129 x 257 (17 x 9 tiles) at 8 and less; max_radius 0, 1, 8 and 32;
both spaces, both colour layouts, masks, ``coef``, a range that cuts pixels out, NaN and infinite depths, the focus by pixel and by value,
every cause of a bad focus, a step edge focused on either side, ``radius`` given and NULL.

Equality everywhere: ``rgb``, ``valid``, ``radius`` and all five counts.  The blur radius is fp64 products, differences and quotients,
correctly rounded on both sides, and one rounding to an integer; everything after it is integer arithmetic - there is no tolerance to
choose.  The pads around every output and the workspace keep their canaries, the inputs are untouched, a workspace pre-filled with
other garbage gives the same bytes, so do two runs and the two libraries, and pointers one element off a 16-byte boundary change
nothing."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests.focus_reference import focus_reference
from tests.focus_scenes import cases
from tests.test_gpu_points import _dev, _Padded, _ptr

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
KEYS = ("rgb", "valid", "radius", "count")


def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


def _focus(lib, c, off=0, garbage=None, coef_dev=None, radius=None, stream=None):
    """one raw mg_depth_focus of case ``c`` -> dict of the outputs as numpy (``radius`` None where it was not asked for)"""
    h, w = c.shape
    n = h * w
    dd = _Padded(np.float32, n, off, c.d)
    cc, mm = _Padded(np.uint8, 3 * n, off, c.colors), _dev(c.mask)
    if coef_dev is None and c.coef is not None:
        coef_buf = _Padded(np.float64, 2, off, c.coef)
        coef_dev = coef_buf.view
    need = lib.mg_depth_focus_workspace_bytes(n)
    assert need == (4 * n + 15) // 16 * 16 + (2 * n + 15) // 16 * 16
    ws = _Padded(np.uint8, need, 0, garbage)
    rgb, valid, count = _Padded(np.uint8, 3 * n, off), _Padded(np.uint8, n, off), _Padded(np.int64, 5, off)
    rad = _Padded(np.uint8, 2 * n, 2 * off)    # uint16 [n], one element off the boundary with ``off``
    want_radius = c.radius if radius is None else radius
    fy, fx = c.focus_at if c.focus_at is not None else (-1, -1)
    rc = lib.mg_depth_focus(dd.ptr(), cc.ptr(), int(c.hwc), _ptr(mm), _ptr(coef_dev), h, w, c.z_range[0], c.z_range[1], c.space, c.gain, c.max_radius,
                            fx, fy, 0.0 if c.focus is None else c.focus, rgb.ptr(), valid.ptr(), rad.ptr() if want_radius else None, count.ptr(),
                            ws.ptr(), need, stream)
    assert rc == 0, lib.mg_last_error().decode()
    torch.cuda.synchronize()
    ws.read()
    assert np.array_equal(dd.read().view(np.uint32), c.d.reshape(-1).view(np.uint32))   # the inputs are left alone
    assert np.array_equal(cc.read(), c.colors.reshape(-1))
    assert mm is None or np.array_equal(mm.cpu().numpy(), c.mask)
    got_radius = rad.read().view(np.uint16)
    if not want_radius:
        assert (got_radius == 0xA5A5).all()                                             # untouched
    return dict(rgb=rgb.read().reshape((h, w, 3) if c.hwc else (3, h, w)), valid=valid.read().reshape(h, w),
                radius=got_radius.reshape(h, w) if want_radius else None, count=count.read())


@functools.lru_cache(maxsize=None)
def _ladder(f16):
    lib = _lib(f16)
    return [_focus(lib, c) for c in cases()]


def _raw(got):
    return [b"" if got[k] is None else np.ascontiguousarray(got[k]).tobytes() for k in KEYS]


def _equal(got, want, name):
    assert got["count"].tolist() == list(want.count), name
    assert np.array_equal(got["valid"], want.valid), name
    assert got["radius"] is None or np.array_equal(got["radius"], want.radius), name
    assert np.array_equal(got["rgb"], want.rgb), name


@LIBS
def test_the_scenes_against_the_restatement(f16):
    cs = cases()
    usable = taps = changed = 0
    for c, got in zip(cs, _ladder(f16)):
        _equal(got, c.want, c.name)
        usable, taps, changed = usable + c.want.count[0], taps + c.want.count[3], changed + int((got["rgb"] != c.colors).sum())
    assert changed > 100000   # the pictures were blurred, not copied
    print(f"[focus] {len(cs)} scenes, {usable} usable pixels, {taps} contributions, {changed} bytes changed: every byte equals the restatement")


def test_two_runs_and_the_two_libraries_give_the_same_bytes():
    a = [_raw(got) for got in _ladder(False)]
    _ladder.cache_clear()
    assert [_raw(got) for got in _ladder(False)] == a and [_raw(got) for got in _ladder(True)] == a


@LIBS
def test_a_workspace_full_of_garbage_and_pointers_off_a_16_byte_boundary(f16):
    lib = _lib(f16)
    picked = [i for i, c in enumerate(cases()) if c.shape in ((9, 33), (17, 65), (20, 24), (33, 40), (24, 48))]
    assert len(picked) >= 12
    g = np.random.default_rng(11)
    for i in picked:
        c, got = cases()[i], _ladder(f16)[i]
        need = lib.mg_depth_focus_workspace_bytes(c.shape[0] * c.shape[1])
        for other in (_focus(lib, c, garbage=g.integers(0, 256, need, dtype=np.uint8)), _focus(lib, c, garbage=np.zeros(need, np.uint8)),
                      _focus(lib, c, off=1)):
            assert _raw(other) == _raw(got), c.name
        # the map of radii is an extra: without it, and with it, the other outputs are the same
        flipped = _focus(lib, c, radius=not c.radius)
        assert _raw(dict(flipped, radius=got["radius"])) == _raw(got), c.name
        assert flipped["radius"] is None or np.array_equal(flipped["radius"], c.want.radius), c.name


@LIBS
def test_coef_straight_from_the_alignment_fit(f16):
    """the device coefficients mg_depth_align_fit leaves feed the call; the same two numbers uploaded give the same bytes, and the
    restatement's"""
    lib = _lib(f16)
    c = next(c for c in cases() if c.shape == (129, 257) and c.coef is None and c.focus_at is not None and c.max_radius == 8 and c.gain > 0)
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
    straight = _focus(lib, c, coef_dev=coef)
    s, t = coef.cpu().tolist()
    assert flag.item() == 0 and abs(s - 1.3) < 0.05 and abs(t + 0.45) < 0.05
    uploaded = _focus(lib, SimpleNamespace(**dict(vars(c), coef=(s, t))))
    assert _raw(straight) == _raw(uploaded)
    want = focus_reference(c.d, c.colors, hwc=c.hwc, mask=c.mask, coef=(s, t), z_range=c.z_range, space=c.space, gain=c.gain, max_radius=c.max_radius,
                           focus_at=c.focus_at)
    assert want.bad is None and want.count[3] > 10 * want.count[0] > 1000
    _equal(straight, want, c.name)


@LIBS
def test_the_python_layer_returns_what_the_raw_call_writes(f16):
    from marigold_amd import Intrinsics, Refocus, refocus
    lib = _lib(f16)
    picked = [i for i, c in enumerate(cases()) if c.shape in ((1, 1), (1, 9), (9, 33), (17, 65), (33, 40), (24, 48))]
    names = {0: "lens", 1: "linear"}
    for i in picked:
        c, got = cases()[i], _ladder(f16)[i]
        coef_arg = c.coef if i % 2 else (None if c.coef is None else torch.tensor(c.coef, dtype=torch.float64, device="cuda"))
        mask_arg = None if c.mask is None else (_dev(c.mask) if i % 2 else _dev(c.mask) != 0)
        r = refocus(_dev(c.d), _dev(c.colors), focus=c.focus, focus_at=c.focus_at, gain=c.gain, space=names[c.space], max_radius=c.max_radius,
                    coef=coef_arg, mask=mask_arg, z_range=c.z_range, radius=c.radius, lib=lib)
        assert isinstance(r, Refocus) and r.count.dtype == torch.int64 and r.count.is_cuda and r.count.shape == (5,)
        assert tuple(r.valid.shape) == c.shape and r.valid.dtype == torch.uint8 and (r.radius is None) == (not c.radius)
        assert r.radius is None or (r.radius.dtype == torch.uint16 and r.radius.is_cuda)
        assert _raw(dict(rgb=r.rgb.cpu().numpy(), valid=r.valid.cpu().numpy(), radius=None if r.radius is None else r.radius.cpu().numpy(),
                         count=r.count.cpu().numpy())) == _raw(got), c.name
        host = r.to_host()
        assert np.array_equal(host.rgb, got["rgb"] if c.hwc else got["rgb"].transpose(1, 2, 0)) and host.rgb.shape == c.shape + (3,), c.name
        assert list(host.count.values()) == got["count"].tolist() and list(host.count) == ["usable", "sharp", "capped", "contributions", "bad_focus"]
    # K with an aperture is the thin lens' gain
    c = next(c for c in cases() if c.kind == "step" and c.space == 0 and c.focus_at is not None)
    d, colors = _dev(c.d), _dev(c.colors)
    a = refocus(d, colors, focus_at=c.focus_at, K=Intrinsics(120.0, 110.0, 3.0, 4.0), aperture=0.5, max_radius=8, lib=lib)
    b = refocus(d, colors, focus_at=c.focus_at, gain=30.0, max_radius=8, lib=lib)
    assert all(torch.equal(x, y) for x, y in zip(a[:2] + a[3:], b[:2] + b[3:])) and a.radius is None
    assert np.array_equal(a.rgb.cpu().numpy(), _ladder(f16)[cases().index(c)]["rgb"])
    for bad in (dict(focus=2.0, focus_at=(1, 1), gain=1.0), dict(gain=1.0), dict(focus=2.0), dict(focus=2.0, gain=-1.0),
                dict(focus=2.0, gain=float("inf")), dict(focus=2.0, gain=1.0, max_radius=33), dict(focus=2.0, gain=1.0, max_radius=-1),
                dict(focus=2.0, gain=1.0, max_radius=2.0), dict(focus=2.0, gain=1.0, space="log"), dict(focus_at=(24, 0), gain=1.0),
                dict(focus_at=(0, -1), gain=1.0), dict(focus_at=(0.5, 1), gain=1.0), dict(focus_at=3, gain=1.0), dict(focus="near", gain=1.0),
                dict(focus=2.0, gain=1.0, K=(1.0, 1.0, 0.0, 0.0), aperture=1.0), dict(focus=2.0, K=(1.0, 1.0, 0.0, 0.0)),
                dict(focus=2.0, aperture=1.0), dict(focus=2.0, K=(1.0, 1.0), aperture=1.0),
                dict(focus=2.0, K=(1.0, 1.0, 0.0, 0.0), aperture=1.0, space="linear"), dict(focus=2.0, gain=1.0, z_range=(2.0, 1.0)),
                dict(focus=2.0, gain=1.0, coef=(1.0,)), dict(focus=2.0, gain=1.0, mask=torch.ones(3, 3, device="cuda"))):
        with pytest.raises(ValueError, match="refocus"):
            refocus(d, colors, lib=lib, **bad)
    for bad in (colors.cpu(), colors[:-1], colors.float(), None):
        with pytest.raises(ValueError, match="refocus"):
            refocus(d, bad, focus=2.0, gain=1.0, lib=lib)
