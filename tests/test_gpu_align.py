"""``mg_depth_align_fit`` / ``mg_depth_align_apply`` (csrc/align.hip) on a real MI355X, both operand libraries, against the numpy fp64
restatement of tests/align_reference.py.

The fit over a size ladder - 1, 2, 3, 63, 64, 65, 4095, 4096, 4097 (the kernel's chunk is 4096 pixels: one block, its edge, two
blocks), 12 293 (four blocks, the last part-filled) and a 24 x 40 map - with and without a mask that drops a fifth of the pixels, with
and without NaN and +-inf planted in ``d`` and in ``ref``, with and without the shift, for 0, 1, 4 and 8 solves from (1, 0) and 4 from
an unweighted start.  The bound is the tile fit's: 1e-9 relative to max(1, |value|) on s and t.  That is a condition on the inputs, not
a measurement: kernel and restatement differ only in the order of fp64 sums, so a case is used only if the restatement summed in
reversed pixel order agrees with itself within 1e-11 - on this ladder every case does (the largest self-difference seen is 1.7e-15), and
the test asserts that none drops out.  Everything else is equality: the flags and the exact (1, 0) of degenerate fits, the apply bit
for bit, canaries around every output, two runs and the two libraries giving the same bits."""
import functools

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests.align_reference import align_apply_reference, align_fit_reference, robustness_scene

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
CHUNK = 4096   # ALIGN_CHUNK of csrc/align.hip
SIZES = (1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 12293, 24 * 40)
MODES = ((0, (1.0, 0.0)), (1, (1.0, 0.0)), (4, (1.0, 0.0)), (8, (1.0, 0.0)), (4, "ls"))   # (iters, start)
DELTA = 0.05
REL, SELF = 1e-9, 1e-11


def _scene(n, masked, planted):
    g = np.random.default_rng(1000 + n)
    ref = g.random(n).astype(np.float32)
    d = ((ref.astype(np.float64) - 0.07) / 0.8 + 0.01 * g.standard_normal(n)).astype(np.float32)
    d[:n // 5] = 0.05
    mask = None
    if masked:
        mask = np.ones(n, np.uint8)
        mask[g.permutation(n)[:n // 5]] = 0
        mask[mask != 0] = g.integers(1, 256, int(mask.sum()), dtype=np.uint8)   # any non-zero byte counts
    if planted and n >= 63:
        d[[1, n // 2, n - 1]] = (np.nan, np.inf, -np.inf)
        ref[[2, n // 3, n - 2]] = (np.inf, np.nan, -np.inf)
    return d, ref, mask


@functools.lru_cache(maxsize=None)
def _cases():
    """[(d, ref, mask, fit_shift, iters, start, (s, t, flag) of the restatement, its self-difference)] - computed once, on the CPU"""
    cases = []
    for n in SIZES:
        for masked in (False, True):
            for planted in (False, True):
                if planted and n < 63:
                    continue
                d, ref, mask = _scene(n, masked, planted)
                for fit_shift in (1, 0):
                    for iters, start in MODES:
                        kw = dict(fit_shift=fit_shift, iters=iters, start=start, delta=DELTA)
                        want = align_fit_reference(d, ref, mask, **kw)
                        back = align_fit_reference(d, ref, mask, reverse=True, **kw)
                        diff = max(abs(want[0] - back[0]) / max(1.0, abs(want[0])), abs(want[1] - back[1]) / max(1.0, abs(want[1])))
                        diff = float("inf") if want[2] != back[2] else diff
                        cases.append((d, ref, mask, fit_shift, iters, start, want, diff))
    return cases


def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _fit(lib, d, ref, mask, fit_shift, iters, start, coef, flag, ws, delta=DELTA, stream=None):
    mode, s0, t0 = (L.ALIGN_START_LS, 1.0, 0.0) if start == "ls" else (L.ALIGN_START_GIVEN,) + tuple(start)
    rc = lib.mg_depth_align_fit(d.data_ptr(), ref.data_ptr(), None if mask is None else mask.data_ptr(), d.numel(), fit_shift, iters, mode, s0, t0,
                                delta, coef.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, lib.mg_last_error().decode()


@functools.lru_cache(maxsize=None)
def _ladder(f16):
    """every case of the ladder on the device -> (coef [cases, 2] fp64, flag [cases] int32) as numpy, read back once"""
    lib, cases = _lib(f16), _cases()
    coef = torch.full((len(cases), 2), float("nan"), dtype=torch.float64, device="cuda")
    flag = torch.full((len(cases),), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mg_depth_align_workspace_bytes(max(SIZES)), dtype=torch.uint8, device="cuda")
    uploaded = {}
    for i, (d, ref, mask, fit_shift, iters, start, _, _) in enumerate(cases):
        key = id(d)
        if key not in uploaded:
            uploaded[key] = (_dev(d), _dev(ref), _dev(mask))
        dd, rr, mm = uploaded[key]
        _fit(lib, dd, rr, mm, fit_shift, iters, start, coef[i], flag[i:i + 1], ws)
    torch.cuda.synchronize()
    return coef.cpu().numpy(), flag.cpu().numpy()


@LIBS
def test_the_fit_over_the_size_ladder(f16):
    cases = _cases()
    coef, flag = _ladder(f16)
    skipped, worst = 0, 0.0
    for i, (d, _, mask, fit_shift, iters, start, want, diff) in enumerate(cases):
        if not diff <= SELF:
            skipped += 1
            continue
        err = max(abs(coef[i, 0] - want[0]) / max(1.0, abs(want[0])), abs(coef[i, 1] - want[1]) / max(1.0, abs(want[1])))
        worst = max(worst, err)
        what = (len(d), mask is not None, fit_shift, iters, start)
        assert flag[i] == want[2], (what, flag[i], want)
        assert err <= REL, (what, coef[i], want, err)
        if want[2]:
            assert tuple(coef[i]) == (1.0, 0.0), what
        if not fit_shift:
            assert coef[i, 1] == 0.0, what
    print(f"[align] {len(cases)} fits, {skipped} not conditioned well enough, the largest self-difference of the restatement "
          f"{max(c[-1] for c in cases):.2e}, the kernel's largest error {worst:.2e}")
    assert skipped <= 0
    assert sum(1 for c in cases if c[6][2] == 0) > len(cases) // 2   # the ladder is about fits that succeed


def test_two_runs_and_the_two_libraries_give_the_same_bits():
    a = _ladder(False)
    _ladder.cache_clear()
    b = _ladder(False)
    c = _ladder(True)
    for other in (b, c):
        assert np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64)) and np.array_equal(a[1], other[1])


@LIBS
def test_degenerate_fits_give_exactly_one_and_zero(f16):
    lib = _lib(f16)
    g = np.random.default_rng(11)
    ref = g.random(300).astype(np.float32)
    d = ((ref - 0.1) / 2 + 0.01 * g.standard_normal(300)).astype(np.float32)
    scenes = {"a constant d": (np.full(300, 0.3, np.float32), ref, None), "one pixel": (d[:1], ref[:1], None),
              "everything masked": (d, ref, np.zeros(300, np.uint8)), "ref = -d": (d, -d, None),
              "an all-NaN ref": (d, np.full(300, np.nan, np.float32), None),
              "one pixel left by the mask": (d, ref, np.eye(1, 300, 17, dtype=np.uint8)[0])}
    ws = torch.empty(lib.mg_depth_align_workspace_bytes(300), dtype=torch.uint8, device="cuda")
    runs = []
    for name, (dd, rr, mm) in scenes.items():
        dd, rr, mm = _dev(np.ascontiguousarray(dd)), _dev(np.ascontiguousarray(rr)), _dev(mm)
        for fit_shift in (1, 0):
            if name == "a constant d" and not fit_shift:
                continue   # (a constant d is no obstacle to a fit of the scale alone)
            for iters, start in MODES:
                coef = torch.full((2,), 123.0, dtype=torch.float64, device="cuda")
                flag = torch.full((1,), -7, dtype=torch.int32, device="cuda")
                _fit(lib, dd, rr, mm, fit_shift, iters, start, coef, flag, ws)
                runs.append(((name, fit_shift, iters, start), coef, flag))
    # a fit that is fine must say so
    good_c, good_f = torch.full((2,), 123.0, dtype=torch.float64, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _fit(lib, _dev(d), _dev(ref), None, 1, 4, (1.0, 0.0), good_c, good_f, ws)
    torch.cuda.synchronize()
    for what, coef, flag in runs:
        assert coef.tolist() == [1.0, 0.0] and flag.item() == 1, what
    assert good_f.item() == 0 and abs(good_c[0].item() - 2.0) < 0.05 and abs(good_c[1].item() - 0.1) < 0.05


def _bits_equal(got, want):
    """fp32 arrays: the same NaN positions, the same bits everywhere else"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@LIBS
def test_the_apply_bit_for_bit_with_canaries(f16):
    lib = _lib(f16)
    d, ref, _ = _scene(12293, False, False)
    coef_fit = torch.empty(2, dtype=torch.float64, device="cuda")
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mg_depth_align_workspace_bytes(12293), dtype=torch.uint8, device="cuda")
    _fit(lib, _dev(d), _dev(ref), None, 1, 4, (1.0, 0.0), coef_fit, flag, ws)
    coefs = [coef_fit, torch.tensor([3.7, -1.2], dtype=torch.float64, device="cuda"), torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda"),
             torch.tensor([1e30, 1e300], dtype=torch.float64, device="cuda")]
    g = np.random.default_rng(7)
    CANARY, PAD = -12345.5, 8
    checked = 0
    for n in (1, 3, 4, 5, 63, 24 * 40, 4097, (1 << 21) + 5 * 1024 + 3):   # (the last: past the grid's 2048 x 256 x 4, the stride loop)
        x = (g.random(n) * 3 - 1).astype(np.float32)
        if n >= 63:
            x[[0, 5, 9, 17, n - 1]] = (np.nan, np.inf, -np.inf, -0.0, np.nan)
        for coef in coefs if n < 1 << 21 else coefs[:1]:
            host_coef = coef.cpu().numpy()
            for use_shift in (1, 0):
                for clip in (None, (0.0, 1.0), (-0.25, 0.25), (1.0, 0.0)):
                    for off_x, off_out, in_place in ((0, 0, False), (1, 1, False), (0, 1, False), (1, 0, False), (0, 0, True), (1, 1, True)):
                        if n >= 1 << 21 and (clip == (-0.25, 0.25) or off_x != off_out):
                            continue
                        base = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
                        src = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
                        xs = src[PAD + off_x:PAD + off_x + n]
                        xs.copy_(torch.from_numpy(x))
                        out = xs if in_place else base[PAD + off_out:PAD + off_out + n]
                        assert (xs.data_ptr() % 16 == 0) == (off_x == 0)
                        lo, hi = (1.0, 0.0) if clip is None else clip
                        rc = lib.mg_depth_align_apply(xs.data_ptr(), n, coef.data_ptr(), use_shift, lo, hi, out.data_ptr(), None)
                        assert rc == 0, lib.mg_last_error().decode()
                        want = align_apply_reference(x, host_coef, bool(use_shift), clip)
                        whole = (src if in_place else base).cpu().numpy()
                        start = PAD + (off_x if in_place else off_out)
                        what = (n, host_coef.tolist(), use_shift, clip, off_x, off_out, in_place)
                        assert _bits_equal(whole[start:start + n], want), what
                        assert (whole[:start] == CANARY).all() and (whole[start + n:] == CANARY).all(), what
                        if not in_place:
                            assert _bits_equal(src.cpu().numpy()[PAD + off_x:PAD + off_x + n], x), what   # the input is left alone
                        checked += 1
    assert torch.equal(coefs[1].cpu(), torch.tensor([3.7, -1.2], dtype=torch.float64))
    # NaN stays NaN under the clamp; infinities meet the bounds
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.5], device="cuda")
    out = torch.empty_like(x)
    assert lib.mg_depth_align_apply(x.data_ptr(), 4, coefs[2].data_ptr(), 1, 0.0, 1.0, out.data_ptr(), None) == 0
    got = out.cpu().numpy()
    assert np.isnan(got[0]) and got[1:].tolist() == [1.0, 0.0, 0.5]
    print(f"[align] {checked} applies checked bit for bit")


@LIBS
def test_the_fit_writes_nothing_but_its_outputs(f16):
    lib = _lib(f16)
    for n in (65, CHUNK + 1, 12293):
        d, ref, mask = _scene(n, True, True)
        need = lib.mg_depth_align_workspace_bytes(n)
        room = torch.full((need + 128,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = room[64:64 + need]
        assert ws.data_ptr() % 16 == 0
        cbuf = torch.full((6,), 777.0, dtype=torch.float64, device="cuda")
        fbuf = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        dd, rr, mm = _dev(d), _dev(ref), _dev(mask)
        keep = (dd.clone(), rr.clone(), mm.clone())
        rc = lib.mg_depth_align_fit(dd.data_ptr(), rr.data_ptr(), mm.data_ptr(), n, 1, 4, L.ALIGN_START_LS, 1.0, 0.0, DELTA, cbuf[2:4].data_ptr(),
                                    fbuf[2:3].data_ptr(), ws.data_ptr(), need, None)
        assert rc == 0, lib.mg_last_error().decode()
        torch.cuda.synchronize()
        room = room.cpu()
        assert (room[:64] == 0xA5).all() and (room[64 + need:] == 0xA5).all()
        assert cbuf[:2].tolist() == [777.0, 777.0] and cbuf[4:].tolist() == [777.0, 777.0] and fbuf.tolist()[:2] + fbuf.tolist()[3:] == [-7] * 4
        assert fbuf[2].item() == 0 and 0.7 < cbuf[2].item() < 0.9
        for now, before in zip((dd, rr, mm), keep):
            assert torch.equal(now.view(torch.uint8), before.view(torch.uint8))   # the inputs are left alone


@LIBS
def test_robust_where_least_squares_is_not(f16):
    lib = _lib(f16)
    d, ref, s_true = robustness_scene()
    ws = torch.empty(lib.mg_depth_align_workspace_bytes(len(d)), dtype=torch.uint8, device="cuda")
    coef = torch.empty(2, 2, dtype=torch.float64, device="cuda")
    flag = torch.empty(2, dtype=torch.int32, device="cuda")
    dd, rr = _dev(d), _dev(ref)
    _fit(lib, dd, rr, None, 1, 4, (1.0, 0.0), coef[0], flag[0:1], ws)
    _fit(lib, dd, rr, None, 1, 0, (1.0, 0.0), coef[1], flag[1:2], ws)
    assert flag.tolist() == [0, 0]
    assert abs(coef[0, 0].item() - s_true) <= 0.03
    assert abs(coef[1, 0].item() - s_true) > 0.2


@LIBS
def test_align_depth_on_a_map(f16):
    """The Python entry point on a 24 x 40 map: a bool mask, the unweighted start, the clip, ``out=`` - against the restatement; and
    the sparse-anchor use of its docstring."""
    from marigold_amd import align_depth
    lib = _lib(f16)
    d, ref, mask = _scene(24 * 40, True, True)
    pred, target, valid = _dev(d).reshape(24, 40), _dev(ref).reshape(24, 40), _dev(mask).reshape(24, 40) != 0
    aligned, coef, flag = align_depth(pred, target, valid, start="ls", lib=lib)
    assert aligned.shape == pred.shape and aligned.dtype == torch.float32 and coef.dtype == torch.float64 and flag.dtype == torch.int32
    s, t, fl = align_fit_reference(d, ref, mask, iters=4, start="ls", delta=0.05)
    got = coef.cpu().numpy()
    assert flag.item() == fl == 0 and abs(got[0] - s) <= REL * max(1, abs(s)) and abs(got[1] - t) <= REL * max(1, abs(t))
    assert _bits_equal(aligned.cpu().numpy().reshape(-1), align_apply_reference(d, got))
    out = torch.empty_like(pred)
    clipped, coef2, _ = align_depth(pred, target, valid, start="ls", clip=(0, 1), out=out, lib=lib)
    assert clipped is out and torch.equal(coef2, coef) and _bits_equal(out.cpu().numpy().reshape(-1), align_apply_reference(d, got, clip=(0, 1)))
    # sparse anchors: forty metric depths, anything elsewhere in ref
    g = np.random.default_rng(3)
    rel = g.random((24, 40)).astype(np.float32)
    metric = (2.5 * rel + 1.5).astype(np.float32)
    where = np.zeros((24, 40), bool)
    where.reshape(-1)[g.permutation(960)[:40]] = True
    sparse = np.where(where, metric, np.float32(-1e9)).astype(np.float32)
    fitted, coef, flag = align_depth(_dev(rel), _dev(sparse), _dev(where), start="ls", delta=0.1, lib=lib)
    assert flag.item() == 0 and np.abs(fitted.cpu().numpy() - metric).max() <= 1e-4
    for bad in (dict(iters=40), dict(delta=0), dict(start="median"), dict(clip=(1, 0))):
        with pytest.raises(ValueError, match="align_depth"):
            align_depth(pred, target, lib=lib, **bad)
    with pytest.raises(ValueError, match="align_depth"):
        align_depth(pred, target[:, :39], lib=lib)
    with pytest.raises(ValueError, match="mask"):
        align_depth(pred, target, valid.float(), lib=lib)
