"""MG_OP_ENS_IID (csrc/ensemble.hip) on a real MI355X against ``marigold_amd.ensemble.ensemble_iid`` - the route the Python pipeline
takes, MG_OP_ENS_DEPTH_MEDIAN without alignment - on the same input.

The bound is equality: the op restates that kernel's per-element arithmetic operation for operation (same selection, same summation
order, no FMA contraction), so every finite value must carry the same bits, and a NaN must stand where the reference has one (NaN
compares equal to NaN here, whatever its payload).  Shapes: n = 210 (not a multiple of 4: one element per lane), 768 (four per
lane), the same through views offset by one float (unaligned: one per lane again, same bits), 24 576 (24 workgroups of the four-per-
lane form, 96 of the other) and 24 576 + 4 x 300 (a part-filled last workgroup).  Ensemble sizes: the issue's 2, 3, 4, 5, 10, 11
and, on the small shapes, one size in every further kernel the launcher chooses between (1, 16, 17, 33, 130)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8   # untouched floats either side of every output
SHAPES = [(6, 5, 7), (6, 8, 16), (3, 64, 128)]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _members(E, shape, nonfinite):
    """[E, *shape] in [0, 1) on the GPU (seeded; read-only).  ``nonfinite``: NaN, +inf and -inf sprinkled over single members of
    about one element in 13 each, two members of one element both infinite with opposite signs, and every member of element 5 NaN."""
    g = torch.Generator().manual_seed(1000 * E + shape[0] * shape[1] * shape[2])
    x = torch.rand((E,) + shape, generator=g)
    if nonfinite:
        flat = x.view(E, -1)
        n = flat.shape[1]
        for k, bad in enumerate((NAN, INF, -INF)):
            cols = torch.arange(3 + 4 * k, n, 13)
            flat[(cols * 7 + k) % E, cols] = bad
        flat[0, 20], flat[E - 1, 20] = INF, -INF
        flat[:, 5] = NAN
    return x.cuda()


@functools.lru_cache(maxsize=None)
def _reference(E, shape, nonfinite, reduction):
    """``ensemble_iid`` with the uncertainty, computed once per input and shared (the prediction does not depend on whether the
    uncertainty is asked for: checked in test_reference_prediction_is_the_same_without_uncertainty)."""
    from marigold_amd.ensemble import ensemble_iid
    pred, unc = ensemble_iid(_members(E, shape, nonfinite), output_uncertainty=True, reduction=reduction)
    torch.cuda.synchronize()
    return pred.flatten(), unc.flatten()


def _same(a, b):
    """Bit equality where neither is NaN, NaN where the other has one."""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    an, bn = torch.isnan(a), torch.isnan(b)
    return bool((an == bn).all()) and torch.equal(a.view(torch.int32)[~an], b.view(torch.int32)[~bn])


def _guarded(n, misalign=0):
    """A destination of n floats ``misalign`` floats past a 16-byte boundary, inside a sentinel-filled buffer -> (buffer, view, lead)."""
    lead = GUARD + misalign
    buf = torch.full((lead + n + GUARD,), 77.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lead:lead + n], lead


def _run(lib, x, reduction, want_unc, mis_in=0, mis_pred=0, mis_unc=0, wrapper=False):
    """One launch on members ``x`` [E, ...] -> (pred [n], unc [n] | None); the outputs' guards must come back untouched."""
    from marigold_amd import ops as O
    E, n = x.shape[0], x[0].numel()
    src = x.reshape(E, n)
    if mis_in:
        hold = torch.empty(E * n + 4 + mis_in, device="cuda")
        src = hold[4 + mis_in:4 + mis_in + E * n].view(E, n)
        src.copy_(x.reshape(E, n))
    assert src.is_contiguous() and src.data_ptr() % 16 == 4 * mis_in % 16
    pb, pred, pl = _guarded(n, mis_pred)
    ub, unc, ul = _guarded(n, mis_unc) if want_unc else (None, None, 0)
    red = 0 if reduction == "median" else 1
    if wrapper:
        rc = lib.mg_ensemble_iid(src.data_ptr(), E, n, red, pred.data_ptr(), None if unc is None else unc.data_ptr(), O.current_stream_handle())
        assert rc == 0, lib.mg_last_error()
    else:
        O.launch(O.ens_iid(src, pred, unc, E=E, n=n, reduction=red), lib=lib)
    torch.cuda.synchronize()
    for buf, lead in ((pb, pl), (ub, ul)):
        if buf is not None:
            assert bool((buf[:lead] == 77.0).all()) and bool((buf[lead + n:] == 77.0).all()), "a store outside the output"
    return pred.clone(), None if unc is None else unc.clone()


def _check(lib, E, shape, nonfinite, reduction, **kw):
    x = _members(E, shape, nonfinite)
    want_pred, want_unc = _reference(E, shape, nonfinite, reduction)
    tag = (E, shape, nonfinite, reduction, kw)
    pred, unc = _run(lib, x, reduction, True, **kw)
    assert _same(pred, want_pred) and _same(unc, want_unc), tag
    pred, unc = _run(lib, x, reduction, False, **kw)   # the uncertainty pointer NULL
    assert unc is None and _same(pred, want_pred), tag
    return pred


@pytest.mark.parametrize("reduction", ["median", "mean"])
@pytest.mark.parametrize("E", [2, 3, 4, 5, 10, 11])
def test_matches_ensemble_iid(lib, E, reduction):
    for nonfinite in (False, True):
        for shape in SHAPES:
            pred = _check(lib, E, shape, nonfinite, reduction)
            if nonfinite:   # the input did what it was built for: NaN where a member has one, and numbers elsewhere
                x = _members(E, shape, True).reshape(E, -1)
                assert bool(torch.isnan(pred[5])) and bool(torch.isnan(pred)[torch.isnan(x).any(0)].all()) and bool(torch.isfinite(pred).any())
            else:
                assert bool(torch.isfinite(pred).all())
        # the four-per-lane shape through views one float off a 16-byte boundary: one element per lane, the same bits
        for kw in (dict(mis_in=1), dict(mis_pred=1), dict(mis_unc=1), dict(mis_in=1, mis_pred=1, mis_unc=1), dict(mis_in=2, mis_pred=3, mis_unc=1)):
            _check(lib, E, (6, 8, 16), nonfinite, reduction, **kw)


@pytest.mark.parametrize("reduction", ["median", "mean"])
def test_part_filled_last_workgroup(lib, reduction):
    """n = 24 576 + 4 x 300: the last workgroup of the four-per-lane form is part filled; n + 1: the same for one element per lane."""
    for shape in ((1, 1, 24576 + 1200), (1, 1, 24576 + 1201)):
        for E in (3, 10):
            _check(lib, E, shape, True, reduction)


@pytest.mark.parametrize("reduction", ["median", "mean"])
@pytest.mark.parametrize("E", [1, 16, 17, 33, 130])
def test_the_other_kernels_of_the_launcher(lib, E, reduction):
    """One size in each kernel the issue's sizes do not reach: the 16- and 32-member register forms, the rank count and the bitwise
    selection from memory (> 32, > 128 members) - each against the kernel the depth op runs at that size."""
    for nonfinite in (False, True):
        for shape in SHAPES[:2]:
            _check(lib, E, shape, nonfinite, reduction)


def test_reference_prediction_is_the_same_without_uncertainty(lib):
    from marigold_amd.ensemble import ensemble_iid
    for reduction in ("median", "mean"):
        x = _members(5, (6, 8, 16), True)
        pred, unc = ensemble_iid(x, output_uncertainty=False, reduction=reduction)
        assert unc is None and _same(pred.flatten(), _reference(5, (6, 8, 16), True, reduction)[0])


def test_the_named_wrapper_and_determinism(lib):
    """``mg_ensemble_iid`` is the op; two launches on the same input give identical bytes (NaN payloads included)."""
    for reduction in ("median", "mean"):
        for E, shape in ((10, (3, 64, 128)), (3, (6, 5, 7)), (33, (6, 8, 16))):
            x = _members(E, shape, True)
            a = _run(lib, x, reduction, True)
            b = _run(lib, x, reduction, True, wrapper=True)
            c = _run(lib, x, reduction, True)
            for u, v, w in zip(a, b, c):
                assert torch.equal(u.view(torch.int32), v.view(torch.int32)) and torch.equal(u.view(torch.int32), w.view(torch.int32))
            assert _same(a[0], _reference(E, shape, True, reduction)[0])


def test_input_is_left_unchanged(lib):
    x = _members(4, (6, 8, 16), True)
    before = x.clone()
    _run(lib, x, "median", True)
    assert torch.equal(before.view(torch.int32), x.view(torch.int32))
