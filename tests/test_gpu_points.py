"""``mg_depth_points`` / ``mg_depth_normals`` (csrc/points.hip) on a real MI355X, both operand libraries, against the numpy float64
restatement of tests/points_reference.py.

The ladder: maps of 1x1, 1x2, 2x1, 3x3, 1x63, 1x64, 1x65, 7x65 (rows that straddle waves), C - 1, C and C + 1 pixels as single rows
(C = 2048, the chunk of the count and the scatter), 97x127 (several chunks, a part-filled last one, rows that straddle chunks) and
513x1025 (257 chunks: more than the S = 256 lanes of the scan launch, so its lanes own two chunks each).  Each carries a smooth
surface with steps, NaN and +-inf planted, values at and just beyond z_min and z_max; each small shape meets six masks - none, all
zero, every second pixel, a random half with arbitrary non-zero bytes, one pixel per chunk, only the last pixel - and the options
rotate over the cases so that every combination of coef / no coef, edge_rel 0 / 0.05, both frames and both colour layouts occurs.
Before anything runs on the device the restatement is asked whether the scenes do their job: every rule removes pixels somewhere,
every tangent form occurs.

Equality everywhere but the normals: count, index, rgb, valid and the fp32 bits of xyz (fp64 products, differences and quotients are
correctly rounded on both sides, then one rounding to fp32).  The normals get 1 fp32 ulp: the one operation not known to be correctly
rounded on both sides is the fp64 square root, and a last-place fp64 difference of the quotient moves the fp32 rounding by one step
at the most.  The test prints how many components differ at all.  Records past `written` and the pads around every output and the
workspace keep their canaries; a capacity below the kept pixels cuts the records and not the count; two runs and the two libraries
give the same bytes; pointers one element off a 16-byte boundary change nothing; coef straight from mg_depth_align_fit is coef
uploaded; and the Python layer returns what the raw calls write."""
import functools
import math

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests.points_reference import CENTRAL, HIGH_ONLY, LOW_ONLY, NONE, points_reference

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
CHUNK, SCAN_LANES = 2048, 256   # POINTS_CHUNK, POINTS_SCAN_LANES of csrc/points.hip
SMALL = ((1, 1), (1, 2), (2, 1), (3, 3), (1, 63), (1, 64), (1, 65), (7, 65), (1, CHUNK - 1), (1, CHUNK), (1, CHUNK + 1), (97, 127))
BIG = (513, 1025)
assert math.ceil(BIG[0] * BIG[1] / CHUNK) > SCAN_LANES
MASKS = ("none", "zero", "second", "half", "per_chunk", "last")
Z_RANGE = (1.5, 3.6)
COEF = (1.25, -0.5)            # z = 1.25 d - 0.5
OPTIONS = [(coef, edge, frame, hwc) for coef in (None, COEF) for edge in (0.0, 0.05) for frame in ("camera", "marigold") for hwc in (True, False)]
CANARY = {np.dtype(np.float32): -12345.5, np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.int64): -7777777,
          np.dtype(np.float64): -5.5}
PAD_BYTES = 64


def _camera(h, w):
    f = 0.9 * max(h, w) + 3.0
    return (f, 1.1 * f, (w - 1) / 2 + 0.3, (h - 1) / 2 - 0.2)


def _scene(h, w, coef):
    """depth fp32 [h, w] whose z - under ``coef`` or without - is a smooth surface inside Z_RANGE with a 30 % step down the middle
    column and a 20 % step across the middle row, NaN and infinities planted, and values at and just beyond both ends of Z_RANGE"""
    g = np.random.default_rng(7000 + 31 * h + w)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = 2.0 + 0.12 * np.sin(xs / 7.0) + 0.1 * np.cos(ys / 5.0) + 0.002 * g.standard_normal((h, w))
    z[:, w // 2:] *= 1.3
    z[h // 2:, :] *= 1.2
    d = (z if coef is None else (z - coef[1]) / coef[0]).astype(np.float32)
    n = h * w
    if n >= 63:
        flat = d.reshape(-1)
        lo, hi = (np.float32(v if coef is None else (v - coef[1]) / coef[0]) for v in Z_RANGE)
        where = g.permutation(n)[:11]
        flat[where[:3]] = (np.nan, np.inf, -np.inf)
        flat[where[3:7]] = (lo, np.nextafter(lo, np.float32(np.inf)), hi, np.nextafter(hi, np.float32(np.inf)))
        flat[where[7:9]] = (np.float32(0.0), np.float32(-1.0))
        flat[where[9:11]] = (lo * np.float32(0.5), hi * np.float32(2.0))
    colors = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return d, colors


def _mask(kind, h, w):
    n = h * w
    g = np.random.default_rng(900 + n)
    if kind == "none":
        return None
    m = np.zeros(n, np.uint8)
    if kind == "second":
        m[::2] = 1
    elif kind == "half":
        pick = g.random(n) < 0.5
        m[pick] = g.integers(1, 256, int(pick.sum()), dtype=np.uint8)   # any non-zero byte counts
    elif kind == "per_chunk":
        for c in range(0, n, CHUNK):
            m[c + int(g.integers(0, min(CHUNK, n - c)))] = 255
    elif kind == "last":
        m[-1] = 1
    return m.reshape(h, w)


@functools.lru_cache(maxsize=None)
def _cases():
    """[(name, d, colors in the option's layout, mask, K, options, the restatement's result)] - computed once, on the CPU"""
    cases, k = [], 0
    for (h, w), masks in [(s, MASKS) for s in SMALL] + [(BIG, ("none", "half"))]:
        for kind in masks:
            coef, edge, frame, hwc = opt = OPTIONS[k % len(OPTIONS)]
            k += 5   # (5 and 16 are coprime: the rotation visits every combination)
            d, colors = _scene(h, w, coef)
            mask, K = _mask(kind, h, w), _camera(h, w)
            want = points_reference(d, K, colors=colors, hwc=True, mask=mask, coef=coef, z_range=Z_RANGE, edge_rel=edge, frame=frame)
            lay = colors if hwc else np.ascontiguousarray(colors.transpose(2, 0, 1))
            cases.append((f"{h}x{w}/{kind}/{opt}", d, lay, mask, K, opt, want))
    return cases


def test_the_scenes_do_their_job():
    """asked of the restatement alone, before the device is trusted with anything"""
    cases = _cases()
    assert {c[5] for c in cases} == set(OPTIONS)
    for rule in ("mask", "nonfinite", "range", "edge"):
        assert sum(c[6].removed[rule] for c in cases) > 0, rule
    for form in (CENTRAL, HIGH_ONLY, LOW_ONLY, NONE):
        assert any(((c[6].form_u == form) & c[6].kept).any() for c in cases), ("u", form)
        assert any(((c[6].form_v == form) & c[6].kept).any() for c in cases), ("v", form)
    assert any((c[6].kept & (c[6].valid == 0)).any() for c in cases)          # a kept pixel without a normal
    assert any(c[6].count[0] == 0 for c in cases) and any(c[6].count[0] == c[1].size for c in cases)   # nothing kept; everything kept
    big = [c for c in cases if c[1].shape == BIG]
    assert big and all(c[6].count[0] > SCAN_LANES for c in big)


def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


class _Padded:
    """a device buffer of ``count`` elements between two pads of canaries; ``off`` elements off the 16-byte boundary"""

    def __init__(self, dtype, count, off=0, fill=None):
        self.dtype, self.count = np.dtype(dtype), count
        self.pad = PAD_BYTES // self.dtype.itemsize
        self.start = self.pad + off
        whole = np.full(count + 2 * self.pad + off, CANARY[self.dtype], self.dtype)
        if fill is not None:
            whole[self.start:self.start + count] = np.asarray(fill, self.dtype).reshape(-1)
        self.whole = torch.from_numpy(whole).cuda()
        self.view = self.whole[self.start:self.start + count]
        assert (self.view.data_ptr() % 16 == 0) == (off * self.dtype.itemsize % 16 == 0)

    def ptr(self):
        return self.view.data_ptr()

    def read(self):
        """-> the payload; the pads are checked on the way"""
        whole = self.whole.cpu().numpy()
        canary = np.asarray(CANARY[self.dtype], self.dtype)
        assert (whole[:self.start] == canary).all() and (whole[self.start + self.count:] == canary).all(), "a pad was written"
        return whole[self.start:self.start + self.count]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _points(lib, d, colors, mask, K, opt, capacity, off=0, coef_dev=None, stream=None):
    """one raw mg_depth_points -> dict of the outputs as numpy (whole buffers of ``capacity`` records, canaries past ``written``)"""
    coef, edge, frame, hwc = opt
    h, w = d.shape
    n = h * w
    dd = _Padded(np.float32, n, off, d)
    cc, mm = _dev(colors), _dev(mask)
    if coef_dev is None and coef is not None:
        coef_buf = _Padded(np.float64, 2, off, coef)
        coef_dev = coef_buf.view
    need = lib.mg_depth_points_workspace_bytes(n)
    assert need > 0
    ws = _Padded(np.uint8, need)
    xyz, rgb, nrm = _Padded(np.float32, 3 * capacity, off), _Padded(np.uint8, 3 * capacity, off), _Padded(np.float32, 3 * capacity, off)
    index, count = _Padded(np.int32, capacity, off), _Padded(np.int64, 2, off)
    rc = lib.mg_depth_points(dd.ptr(), _ptr(cc), int(hwc), _ptr(mm), _ptr(coef_dev), h, w, *K, Z_RANGE[0], Z_RANGE[1], edge, L.NORMALS_FRAME[frame],
                             capacity, xyz.ptr(), rgb.ptr(), nrm.ptr(), index.ptr(), count.ptr(), ws.ptr(), need, stream)
    assert rc == 0, lib.mg_last_error().decode()
    torch.cuda.synchronize()
    ws.read()
    assert np.array_equal(dd.read().view(np.uint32), d.reshape(-1).view(np.uint32))   # the input is left alone
    return dict(xyz=xyz.read().reshape(capacity, 3), rgb=rgb.read().reshape(capacity, 3), nrm=nrm.read().reshape(capacity, 3), index=index.read(),
                count=count.read())


def _normals(lib, d, mask, K, opt, off=0, stream=None):
    coef, edge, frame, _ = opt
    h, w = d.shape
    dd, mm = _Padded(np.float32, h * w, off, d), _dev(mask)
    cf = None if coef is None else _Padded(np.float64, 2, off, coef)
    out, valid = _Padded(np.float32, 3 * h * w, off), _Padded(np.uint8, h * w, off)
    rc = lib.mg_depth_normals(dd.ptr(), _ptr(mm), None if cf is None else cf.ptr(), h, w, *K, Z_RANGE[0], Z_RANGE[1], edge, L.NORMALS_FRAME[frame],
                              out.ptr(), valid.ptr(), stream)
    assert rc == 0, lib.mg_last_error().decode()
    torch.cuda.synchronize()
    return out.read().reshape(3, h, w), valid.read().reshape(h, w)


@functools.lru_cache(maxsize=None)
def _ladder(f16):
    """every case on the device -> [(points dict, dense normals, valid)]; the capacity leaves three records past the map's pixels"""
    lib = _lib(f16)
    return [(_points(lib, d, colors, mask, K, opt, d.size + 3),) + _normals(lib, d, mask, K, opt) for _, d, colors, mask, K, opt, _ in _cases()]


def _ulps(got, want):
    """the distance of fp32 arrays in representable steps (+0 and -0 are one value)"""
    def ordered(a):
        i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(got) - ordered(want))


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _canaries_past(got, written):
    return all((got[k][written:] == np.asarray(CANARY[got[k].dtype], got[k].dtype)).all() for k in ("xyz", "rgb", "nrm", "index"))


@LIBS
def test_the_ladder_against_the_restatement(f16):
    cases, runs = _cases(), _ladder(f16)
    differing = components = records = 0
    for (name, d, _, _, _, _, want), (got, dense, valid) in zip(cases, runs):
        kept, written = want.count
        assert got["count"].tolist() == [kept, written], name
        assert np.array_equal(got["index"][:written], want.index), name
        assert np.array_equal(got["rgb"][:written], want.rgb), name
        assert _same_bits(got["xyz"][:written], want.xyz), name
        assert _canaries_past(got, written), name
        assert np.array_equal(valid, want.valid), name
        for g, r in ((got["nrm"][:written], want.nrm), (dense, want.dense)):
            u = _ulps(g, r)
            assert np.isfinite(g).all() and u.max(initial=0) <= 1, (name, int(u.max(initial=0)))
            differing += int((u != 0).sum())
            components += u.size
        assert not (dense[:, valid == 0] != 0).any(), name
        records += written
    print(f"[points] {len(cases)} cases, {records} records, {components} normal components compared, {differing} differ from the "
          f"restatement (by one fp32 step)")


def test_two_runs_and_the_two_libraries_give_the_same_bytes():
    def raw(runs):
        return [np.ascontiguousarray(a).tobytes() for got, dense, valid in runs for a in (*[got[k] for k in sorted(got)], dense, valid)]
    a = raw(_ladder(False))
    _ladder.cache_clear()
    assert raw(_ladder(False)) == a and raw(_ladder(True)) == a


@LIBS
def test_a_capacity_below_the_kept_pixels(f16):
    lib = _lib(f16)
    tried = 0
    for name, d, colors, mask, K, opt, want in _cases():
        kept = want.count[0]
        if d.shape not in ((7, 65), (1, CHUNK + 1), (97, 127)) or kept < 3:
            continue
        for capacity in (kept - 1, 1):
            got = _points(lib, d, colors, mask, K, opt, capacity)   # (the pads behind the last record stand for "past the capacity")
            assert got["count"].tolist() == [kept, capacity], (name, capacity)
            assert np.array_equal(got["index"], want.index[:capacity]) and _same_bits(got["xyz"], want.xyz[:capacity]), (name, capacity)
            assert np.array_equal(got["rgb"], want.rgb[:capacity]) and _ulps(got["nrm"], want.nrm[:capacity]).max() <= 1, (name, capacity)
            tried += 1
    assert tried >= 12


@LIBS
def test_pointers_one_element_off_a_16_byte_boundary(f16):
    lib = _lib(f16)
    picked = [i for i, c in enumerate(_cases()) if c[1].shape in ((7, 65), (97, 127)) and c[6].count[0] > 0]
    assert len(picked) >= 6
    for i in picked:
        name, d, colors, mask, K, opt, _ = _cases()[i]
        got, dense, valid = _ladder(f16)[i]
        off = _points(lib, d, colors, mask, K, opt, d.size + 3, off=1)
        assert all(np.array_equal(off[k].view(np.uint8), got[k].view(np.uint8)) for k in got), name
        dense1, valid1 = _normals(lib, d, mask, K, opt, off=1)
        assert _same_bits(dense1, dense) and np.array_equal(valid1, valid), name


@LIBS
def test_coef_straight_from_the_alignment_fit(f16):
    """the device coefficients mg_depth_align_fit leaves feed the unprojection; the same two numbers uploaded give the same cloud"""
    lib = _lib(f16)
    h, w = 97, 127
    d, colors = _scene(h, w, COEF)
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
    straight = _points(lib, d, colors, None, K, opt, h * w, coef_dev=coef)
    s, t = coef.cpu().tolist()
    assert flag.item() == 0 and abs(s - 1.3) < 0.05 and abs(t + 0.45) < 0.05
    uploaded = _points(lib, d, colors, None, K, ((s, t),) + opt[1:], h * w)
    assert all(np.array_equal(straight[k].view(np.uint8), uploaded[k].view(np.uint8)) for k in straight)
    want = points_reference(d, K, colors=colors, coef=(s, t), z_range=Z_RANGE, edge_rel=0.05, frame="marigold")
    written = want.count[1]
    assert straight["count"].tolist() == list(want.count) and written > h * w // 2
    assert _same_bits(straight["xyz"][:written], want.xyz) and np.array_equal(straight["index"][:written], want.index)


@LIBS
def test_the_python_layer_returns_what_the_raw_calls_write(f16):
    from marigold_amd import Intrinsics, depth_to_normals, depth_to_points
    lib = _lib(f16)
    picked = [i for i, c in enumerate(_cases()) if c[1].shape in ((3, 3), (7, 65), (97, 127))]
    for i in picked:
        name, d, colors, mask, K, (coef, edge, frame, hwc), want = _cases()[i]
        got, dense, valid = _ladder(f16)[i]
        written = want.count[1]
        coef_arg = coef if i % 2 else (None if coef is None else torch.tensor(coef, dtype=torch.float64, device="cuda"))
        mask_arg = None if mask is None else (_dev(mask) if i % 2 else _dev(mask) != 0)
        if d.shape == (3, 3) and not hwc:
            colors = colors.transpose(1, 2, 0)   # ([3, 3, 3] is read as [h, w, 3])
        cloud = depth_to_points(_dev(d), Intrinsics(*K), colors=_dev(colors), mask=mask_arg, coef=coef_arg, z_range=Z_RANGE, edge_rel=edge,
                                normals=True, frame=frame, index=True, lib=lib)
        assert cloud.xyz.shape == (d.size, 3) and cloud.count.dtype == torch.int64 and cloud.count.is_cuda
        host = cloud.to_host()
        assert (host.kept, host.written) == want.count, name
        assert _same_bits(host.xyz, got["xyz"][:written]) and _same_bits(host.normals, got["nrm"][:written]), name
        assert np.array_equal(host.rgb, got["rgb"][:written]) and np.array_equal(host.index, got["index"][:written]), name
        bare = depth_to_points(_dev(d), K, mask=mask_arg, coef=coef_arg, z_range=Z_RANGE, edge_rel=edge, capacity=max(1, written // 2), lib=lib)
        assert bare.rgb is None and bare.normals is None and bare.index is None
        half = bare.to_host()
        assert (half.kept, half.written) == (want.count[0], min(want.count[0], max(1, written // 2))), name
        assert _same_bits(half.xyz, got["xyz"][:half.written]), name
        n_dev, v_dev = depth_to_normals(_dev(d), K, mask=mask_arg, coef=coef_arg, z_range=Z_RANGE, edge_rel=edge, frame=frame, lib=lib)
        assert v_dev.dtype == torch.bool and _same_bits(n_dev.cpu().numpy(), dense) and np.array_equal(v_dev.cpu().numpy(), valid != 0), name
    d = _dev(_cases()[picked[-1]][1])
    K = _cases()[picked[-1]][4]
    for bad in (dict(z_range=(2.0, 1.0)), dict(z_range=(-1.0, 2.0)), dict(edge_rel=-0.1), dict(frame="world"), dict(capacity=0),
                dict(coef=(1.0,)), dict(mask=torch.ones(3, 3, device="cuda")), dict(colors=torch.zeros(3, 3, 3, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError, match="depth_to_points"):
            depth_to_points(d, K, lib=lib, **bad)
    with pytest.raises(ValueError, match="depth_to_normals"):
        depth_to_normals(d, (0.0, 1.0, 0.0, 0.0), lib=lib)
    with pytest.raises(ValueError, match="depth_to_normals"):
        depth_to_normals(d.cpu(), K, lib=lib)
