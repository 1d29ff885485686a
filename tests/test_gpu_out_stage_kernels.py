"""The depth and normals output stages on a real MI355X, in both library builds: MG_OP_COLORIZE with its optional clipped / 16-bit
outputs (``mg_depth_visualize``) and ``mg_normals_finish`` (MG_OP_NORMALS_VIS's kernel with the clipped map).

Every bound is equality.  The clip and the integer casts have no rounding to allow for: ``np.clip`` selects one of its three
arguments, the 16-bit value is one fp32 product (exact to compare: numpy multiplies float32 by float32) truncated, the colour is a
table entry.  NaN: numpy's cast of NaN to an integer is undefined, the kernels give 0 (MG_OP_IID_VIS's convention), so the 16-bit
values and the pictures are compared on the non-NaN elements and must be 0 where the input is NaN.

Shapes: 64 x 128 (a lane owns four elements), 37 x 53 (odd n: one element per lane), 64 x 128 starting one element into every buffer
(unaligned: one per lane), n = 4 and n = 1.  Every output lies between guard elements that must come back untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BUILDS = [False, True]   # the fp16-operand library?
BUILD_IDS = ["bf16lib", "fp16lib"]
GUARD = 16               # untouched elements either side of every output
CASES = [("64x128", 64 * 128, 0), ("37x53", 37 * 53, 0), ("unaligned", 64 * 128, 1), ("n4", 4, 0), ("n1", 1, 0)]


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {False: L.init(0), True: L.init(0, True)}


@pytest.fixture(scope="module")
def lut():
    """A table whose 256 entries all differ (the kernels index it; which colours it holds does not matter)."""
    g = np.random.default_rng(5)
    t = g.integers(0, 256, size=(256, 3), dtype=np.uint8)
    t[:, 0] = g.permutation(256).astype(np.uint8)
    return t


def _specials_depth():
    f = np.float32
    edges = np.arange(257, dtype=np.float32) / f(256)                      # every table edge k / 256 and its two fp32 neighbours
    steps = np.array([0, 1, 2, 255, 256, 32767, 32768, 65534, 65535], dtype=np.float32) / f(65535.0)   # 16-bit boundaries j / 65535
    v = np.concatenate([edges, np.nextafter(edges, f(-1)), np.nextafter(edges, f(2)), steps, np.nextafter(steps, f(-1)), np.nextafter(steps, f(2)),
                        np.array([0.0, -0.0, 1.0, np.nextafter(f(1), f(0)), np.inf, -np.inf, np.nan, -np.nan, 1.5, -0.5], dtype=np.float32)])
    return v.astype(np.float32)


def _depth_input(n, seed):
    """Random values in [-0.5, 1.5] with the special values planted at random places (all of them when they fit)."""
    g = np.random.default_rng(seed)
    x = g.uniform(-0.5, 1.5, size=n).astype(np.float32)
    sp = _specials_depth()
    if n >= 2 * sp.size:
        x[g.choice(n, size=sp.size, replace=False)] = sp
    elif n == 4:
        x[:] = np.array([np.nan, -0.0, 1.0, 0.3], dtype=np.float32)
    return x


def _normals_input(hw, seed):
    g = np.random.default_rng(seed)
    x = g.uniform(-1.5, 1.5, size=(3, hw)).astype(np.float32)
    f = np.float32
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)), np.nextafter(f(-1), f(0)),
                   np.nextafter(f(-1), f(-2)), 1.5, -1.5], dtype=np.float32)
    sp = np.concatenate([sp, (np.arange(256, dtype=np.float32) / f(127.5) - f(1))])   # around every byte boundary of (x + 1) * 127.5
    if hw >= 2 * sp.size:
        for c in range(3):
            x[c, g.choice(hw, size=sp.size, replace=False)] = g.permutation(sp)
    elif hw == 4:
        x[0] = [np.nan, -0.0, 1.0, 0.3]
        x[1] = [2.0, np.nan, -2.0, -1.0]
        x[2] = [np.inf, -np.inf, 0.5, np.nan]
    return x


class _Guarded:
    """A tensor of ``n`` elements inside a buffer of sentinels; the data start ``misalign`` elements past a 16-byte boundary."""

    def __init__(self, n, dtype, misalign, fill):
        per16 = 16 // torch.empty(0, dtype=dtype).element_size()
        self.lead = per16 * -(-GUARD // per16) + misalign
        self.fill = fill
        if dtype == torch.uint16:   # (filled as int16: the unsigned type has few device kernels)
            self.buf = torch.full((self.lead + n + GUARD,), fill, dtype=torch.int16, device="cuda").view(torch.uint16)
        else:
            self.buf = torch.full((self.lead + n + GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.buf[self.lead:self.lead + n]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == misalign * self.t.element_size() % 16

    def intact(self):
        lead, tail = self.buf[:self.lead].cpu().numpy(), self.buf[self.lead + self.t.numel():].cpu().numpy()
        return bool((lead == self.fill).all()) and bool((tail == self.fill).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- depth -----------------------------------------------------------------------------------------------------------------------


def _run_depth(lib, x, lut_dev, mis, want=("clipped", "u16", "out"), in_place=False, through_call=False):
    """One launch over a copy of ``x`` -> dict of the outputs asked for (numpy) + "depth" = the input buffer afterwards."""
    from marigold_amd import _lib as L, ops as O
    n = x.size
    d = _Guarded(n, torch.float32, mis, -7.0)
    d.t.copy_(torch.from_numpy(x))
    c = d if in_place else (_Guarded(n, torch.float32, mis, -7.0) if "clipped" in want else None)
    u = _Guarded(n, torch.uint16, mis, 77) if "u16" in want else None
    o = _Guarded(3 * n, torch.uint8, mis, 77) if "out" in want else None
    ptr = lambda g: None if g is None else g.t   # noqa: E731
    if through_call:
        L.check(lib.mg_depth_visualize(d.t.data_ptr(), lut_dev.data_ptr() if o else None, n, c.t.data_ptr() if c else None,
                                       u.t.data_ptr() if u else None, o.t.data_ptr() if o else None, O.current_stream_handle()), "mg_depth_visualize", lib)
    else:
        O.launch(O.colorize(d.t, lut_dev if o else None, ptr(o), n=n, clipped=ptr(c), u16=ptr(u)), lib=lib)
    torch.cuda.synchronize()
    assert all(g is None or g.intact() for g in (d, c, u, o)), "a store outside an output"
    res = {"depth": d.t.cpu().numpy().copy()}
    if c:
        res["clipped"] = c.t.cpu().numpy().copy()
    if u:
        res["u16"] = u.t.cpu().numpy().copy()
    if o:
        res["out"] = o.t.cpu().numpy().reshape(n, 3).copy()
    return res


@pytest.fixture(scope="module")
def depth_cases():
    """Inputs and numpy references, computed once."""
    cases = {}
    for k, (name, n, _mis) in enumerate(CASES):
        xs = [_depth_input(n, 100 + k)]
        if n == 1:
            xs = [np.array([v], dtype=np.float32) for v in (np.nan, 1.5, -0.0, 0.5)]
        refs = []
        for x in xs:
            with np.errstate(invalid="ignore"):
                clipped = np.clip(x, 0, 1)
                u16 = (clipped * np.float32(65535.0)).astype(np.uint16)
                idx = np.minimum((np.where(np.isnan(x), np.float32(0), clipped) * np.float32(256.0)).astype(np.int64), 255)   # (a NaN is black: no entry)
            refs.append((x, clipped, u16, idx, np.isnan(x)))
        cases[name] = refs
    return cases


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_depth_stage(libs, lut, depth_cases, case, f16):
    lib = libs[f16]
    name, n, mis = case
    lut_dev = torch.from_numpy(lut).cuda()
    for x, clipped, u16, idx, nan in depth_cases[name]:
        assert x.size == n and (n < 1000 or (nan.sum() >= 2 and np.isinf(x).sum() >= 2 and (np.signbit(x) & (x == 0)).any()))
        colour = np.where(nan[:, None], np.uint8(0), lut[idx])
        # the op as it was (no new output): the numpy table look-up, a NaN black
        old = _run_depth(lib, x, lut_dev, mis, want=("out",))
        assert np.array_equal(old["out"], colour) and np.array_equal(_bits(old["depth"]), _bits(x))
        got = _run_depth(lib, x, lut_dev, mis)
        assert np.array_equal(_bits(got["clipped"]), _bits(clipped))          # bitwise np.clip: NaN where NaN, -0.0 where numpy keeps it
        assert np.array_equal(np.isnan(got["clipped"]), nan)
        assert np.array_equal(got["u16"][~nan], u16[~nan]) and not got["u16"][nan].any()
        assert np.array_equal(got["out"], old["out"])                          # byte for byte the existing op's picture
        assert np.array_equal(_bits(got["depth"]), _bits(x))                   # the input is not written
        # in place: P_CLIPPED == P_DEPTH
        inp = _run_depth(lib, x, lut_dev, mis, in_place=True)
        assert np.array_equal(_bits(inp["depth"]), _bits(clipped)) and np.array_equal(inp["u16"], got["u16"]) and np.array_equal(inp["out"], got["out"])
        # each output alone
        for only in ("clipped", "u16", "out"):
            one = _run_depth(lib, x, lut_dev, mis, want=(only,))
            a, b = one[only], got[only]
            assert np.array_equal(_bits(a), _bits(b)) if only == "clipped" else np.array_equal(a, b), only
        # the call
        call = _run_depth(lib, x, lut_dev, mis, through_call=True)
        assert np.array_equal(_bits(call["clipped"]), _bits(got["clipped"])) and np.array_equal(call["u16"], got["u16"])
        assert np.array_equal(call["out"], got["out"])


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_depth_stage_mixed_alignment(libs, lut, f16):
    """Only ONE pointer off its vector alignment sends the launch to the one-element form: same results, nothing outside."""
    from marigold_amd import ops as O
    lib = libs[f16]
    n = 64 * 128
    x = _depth_input(n, 7)
    lut_dev = torch.from_numpy(lut).cuda()
    want = _run_depth(lib, x, lut_dev, 0)
    for which in ("d", "c", "u", "o"):
        d = _Guarded(n, torch.float32, int(which == "d"), -7.0)
        d.t.copy_(torch.from_numpy(x))
        c = _Guarded(n, torch.float32, int(which == "c"), -7.0)
        u = _Guarded(n, torch.uint16, int(which == "u"), 77)
        o = _Guarded(3 * n, torch.uint8, int(which == "o"), 77)
        O.launch(O.colorize(d.t, lut_dev, o.t, n=n, clipped=c.t, u16=u.t), lib=lib)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (d, c, u, o)), which
        assert np.array_equal(_bits(c.t.cpu().numpy()), _bits(want["clipped"])) and np.array_equal(u.t.cpu().numpy(), want["u16"]), which
        assert np.array_equal(o.t.cpu().numpy().reshape(n, 3), want["out"]), which


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_depth_stage_refusals(libs, lut, f16):
    from marigold_amd import _lib as L, ops as O
    lib = libs[f16]
    d = torch.rand(64, device="cuda")
    keep = d.clone()
    c, u = torch.full((64,), -7.0, device="cuda"), torch.full((64,), 77, dtype=torch.int16, device="cuda").view(torch.uint16)
    o = torch.full((64, 3), 77, dtype=torch.uint8, device="cuda")
    lut_dev = torch.from_numpy(lut).cuda()
    for kw in (dict(clipped=c, lo=0.0, hi=2.0), dict(u16=u, lo=0.5, hi=1.0), dict(clipped=c, u16=u, lo=-1.0, hi=1.0)):
        with pytest.raises(L.MarigoldHipError, match=r"range \(0, 1\)"):
            O.launch(O.colorize(d, lut_dev, o, n=64, **kw), lib=lib)
    with pytest.raises(L.MarigoldHipError, match="null"):
        O.launch(O.colorize(d, lut_dev, None, n=64), lib=lib)      # all three outputs NULL
    with pytest.raises(L.MarigoldHipError, match="null"):
        O.launch(O.colorize(d, None, o, n=64), lib=lib)            # a picture without a table
    torch.cuda.synchronize()
    assert torch.equal(d, keep) and bool((c == -7.0).all()) and bool((u.cpu().numpy() == 77).all()) and bool((o == 77).all())
    # any other range still colours, as before
    O.launch(O.colorize(d, lut_dev, o, n=64, lo=0.25, hi=0.75), lib=lib)
    torch.cuda.synchronize()
    x = keep.cpu().numpy()
    idx = np.minimum((np.clip((x - np.float32(0.25)) * np.float32(1.0 / 0.5), 0, 1) * np.float32(256.0)).astype(np.int64), 255)
    assert np.array_equal(o.cpu().numpy(), lut[idx])


def test_depth_output_device_helper(libs):
    """``util.image_util.depth_output_device``: the three results of one launch; the picture is ``colorize_depth_device``'s."""
    from marigold_amd.util.image_util import colorize_depth_device, depth_output_device
    x = _depth_input(64 * 128, 3).reshape(64, 128)
    d = torch.from_numpy(x).cuda()
    clipped, u16, pic = depth_output_device(d)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        want = np.clip(x, 0, 1)
        w16 = (want * np.float32(65535.0)).astype(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(_bits(clipped.cpu().numpy()), _bits(want)) and np.array_equal(_bits(d.cpu().numpy()), _bits(x))
    assert np.array_equal(u16.cpu().numpy()[~nan], w16[~nan]) and not u16.cpu().numpy()[nan].any()
    assert torch.equal(pic, colorize_depth_device(d))
    c2, u2, p2 = depth_output_device(d, cmap=None, in_place=True)
    torch.cuda.synchronize()
    assert c2 is d and p2 is None and np.array_equal(u2.cpu().numpy(), u16.cpu().numpy()) and np.array_equal(_bits(d.cpu().numpy()), _bits(want))


# ---- normals ---------------------------------------------------------------------------------------------------------------------

NORMALS_CASES = [("64x128", 64, 128, 0), ("37x53", 37, 53, 0), ("unaligned", 64, 128, 1), ("2x2", 2, 2, 0), ("1x1", 1, 1, 0)]


def _run_normals(lib, x, H, W, mis, want=("clipped", "out"), in_place=False):
    from marigold_amd import _lib as L, ops as O
    hw = H * W
    p = _Guarded(3 * hw, torch.float32, mis, -7.0)
    p.t.copy_(torch.from_numpy(x.reshape(-1)))
    c = p if in_place else (_Guarded(3 * hw, torch.float32, mis, -7.0) if "clipped" in want else None)
    o = _Guarded(3 * hw, torch.uint8, mis, 77) if "out" in want else None
    L.check(lib.mg_normals_finish(p.t.data_ptr(), H, W, c.t.data_ptr() if c else None, o.t.data_ptr() if o else None, O.current_stream_handle()),
            "mg_normals_finish", lib)
    torch.cuda.synchronize()
    assert all(g is None or g.intact() for g in (p, c, o)), "a store outside an output"
    res = {"pred": p.t.cpu().numpy().reshape(3, hw).copy()}
    if c:
        res["clipped"] = c.t.cpu().numpy().reshape(3, hw).copy()
    if o:
        res["out"] = o.t.cpu().numpy().reshape(hw, 3).copy()
    return res


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("case", NORMALS_CASES, ids=[c[0] for c in NORMALS_CASES])
def test_normals_stage(libs, case, f16):
    from marigold_amd import ops as O
    lib = libs[f16]
    name, H, W, mis = case
    hw = H * W
    xs = [_normals_input(hw, 200 + H)]
    if hw == 1:
        xs = [np.array(v, dtype=np.float32).reshape(3, 1) for v in ([np.nan, 2.0, -2.0], [0.25, -0.0, np.inf])]
    for x in xs:
        nan = np.isnan(x)
        assert hw < 1000 or (nan.sum() >= 3 and np.isinf(x).sum() >= 6)
        with np.errstate(invalid="ignore"):
            clipped = np.clip(x, -1, 1)
            pic = ((clipped + 1) * 127.5).astype(np.uint8)   # float32 throughout: the pipeline's line on a float32 array
        assert clipped.dtype == np.float32 and ((clipped + 1) * 127.5).dtype == np.float32
        # the existing launch (MG_OP_NORMALS_VIS), on the same bytes
        p = _Guarded(3 * hw, torch.float32, mis, -7.0)
        p.t.copy_(torch.from_numpy(x.reshape(-1)))
        o = _Guarded(3 * hw, torch.uint8, mis, 77)
        O.launch(O.normals_vis(p.t, o.t, H=H, W=W), lib=lib)
        torch.cuda.synchronize()
        assert o.intact() and p.intact() and np.array_equal(_bits(p.t.cpu().numpy()), _bits(x.reshape(-1)))
        old = o.t.cpu().numpy().reshape(hw, 3)
        assert np.array_equal(old.T[~nan], pic[~nan]) and not old.T[nan].any()
        got = _run_normals(lib, x, H, W, mis)
        assert np.array_equal(_bits(got["clipped"]), _bits(clipped)) and np.array_equal(np.isnan(got["clipped"]), nan)
        assert np.array_equal(got["out"], old) and np.array_equal(_bits(got["pred"]), _bits(x))
        inp = _run_normals(lib, x, H, W, mis, in_place=True)
        assert np.array_equal(_bits(inp["pred"]), _bits(clipped)) and np.array_equal(inp["out"], old)
        for only in ("clipped", "out"):
            one = _run_normals(lib, x, H, W, mis, want=(only,))
            assert np.array_equal(_bits(one[only]) if only == "clipped" else one[only], _bits(got[only]) if only == "clipped" else got[only]), only
        # mg_normals_visualize forwards
        o2 = _Guarded(3 * hw, torch.uint8, mis, 77)
        assert lib.mg_normals_visualize(p.t.data_ptr(), H, W, o2.t.data_ptr(), O.current_stream_handle()) == 0
        torch.cuda.synchronize()
        assert o2.intact() and np.array_equal(o2.t.cpu().numpy().reshape(hw, 3), old)


def test_normals_stage_refusals_and_helper(libs):
    from marigold_amd import _lib as L, ops as O
    from marigold_amd.util.image_util import normals_output_device, normals_visualization_device
    lib = libs[False]
    x = _normals_input(64 * 128, 9).reshape(3, 64, 128)
    p = torch.from_numpy(x).cuda()
    assert lib.mg_normals_finish(p.data_ptr(), 64, 128, None, None, O.current_stream_handle()) != 0 and b"null" in lib.mg_last_error()
    with pytest.raises(L.MarigoldHipError, match="null"):
        O.launch(O.normals_vis(p, None, H=64, W=128), lib=lib)
    clipped, pic = normals_output_device(p)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(clipped.cpu().numpy()), _bits(np.clip(x, -1, 1))) and torch.equal(pic, normals_visualization_device(p))
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(x))
    c2, p2 = normals_output_device(p, in_place=True)
    torch.cuda.synchronize()
    assert c2 is p and torch.equal(p2, pic) and np.array_equal(_bits(p.cpu().numpy()), _bits(np.clip(x, -1, 1)))
