"""The output stage on a real MI355X: everything after the decoder's last convolution - the MG_POST_* tails
(csrc/misc.hip), the ensembling kernels (csrc/ensemble.hip) and the colour table (csrc/resize.hip) - op by op through
the C ABI (``ops.launch``) against plain torch on the CPU: ``oracle.ensemble`` where it restates the operation, float64
torch where an fp32 summation order is involved.

What is covered that the other modules do not launch: every member-count form of ``mg_launch_ensemble`` (templates
for E <= 4, 8, 10, 16, 32; the LDS form for 33 ... 128; the bitwise selection beyond) at its boundaries, the 16-byte
vector path and its scalar tail (HW % 4, pointer alignment), the grid-stride loops, the statistics kernel's column
chunks of 32 members, the extremal pixel's tie-break, the post tails without a convolution in front - and non-finite
input: the mask of non-finite outputs must be the reference's (torch's clip, median, min and max keep NaN).

Every output is a window of a NaN-filled buffer: the cells before and after it must still be NaN after the launch.
"""
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
U32 = 2.0 ** -24      # fp32 unit roundoff
GUARD = 4             # floats in front of an output window: keeps the window 16-byte aligned


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from marigold_amd import _lib
    _lib.init(0)
    return torch.device("cuda:0")


def _run(op):
    from marigold_amd import ops
    ops.launch(op)
    torch.cuda.synchronize()


class _Out:
    """An output window of ``n`` elements inside a NaN-filled buffer, ``off`` elements in (off % 4 == 0: 16-byte aligned)."""

    def __init__(self, n, dev, off=GUARD, dtype=torch.float32):
        self.n, self.off = n, off
        self.buf = torch.full((off + n + GUARD,), NAN, device=dev, dtype=dtype)
        self.view = self.buf[off:off + n]

    def get(self, name):
        b = self.buf.cpu()
        assert torch.isnan(b[:self.off]).all() and torch.isnan(b[self.off + self.n:]).all(), f"{name}: wrote outside its output"
        return b[self.off:self.off + self.n].clone()


def _same(name, got, ref):
    """Bit-equal as values, NaN at the same places."""
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), (f"{name}: {int((rn & ~gn).sum())} of {int(rn.sum())} elements that are NaN in the reference are not, "
                                 f"{int((gn & ~rn).sum())} are NaN that should not be")
    bad = (got != ref) & ~rn
    assert not bad.any(), (f"{name}: {int(bad.sum())} / {got.numel()} elements differ from the reference, first at {int(bad.nonzero()[0])}: "
                           f"{got[bad][0].item()!r} vs {ref[bad][0].item()!r}")


def _same_mask(name, got, ref):
    """The reference's non-finite mask, kind by kind (NaN, +inf, -inf)."""
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    for what, f in (("NaN", torch.isnan), ("+inf", torch.isposinf), ("-inf", torch.isneginf)):
        g, r = f(got), f(ref)
        assert torch.equal(g, r), (f"{name}: {int((r & ~g).sum())} of {int(r.sum())} outputs that are {what} in the reference are not, "
                                   f"{int((g & ~r).sum())} are {what} that should not be")


def _within(name, got, ref64, bound):
    """|got - ref| <= bound on the finite elements of the float64 reference; the same non-finite mask.  -> max error"""
    got, ref64 = got.reshape(-1), ref64.reshape(-1)
    _same_mask(name, got, ref64.float())
    fin = torch.isfinite(ref64)
    err = float((got.double() - ref64)[fin].abs().max()) if fin.any() else 0.0
    assert err <= bound, f"{name}: max|err| {err:.4e} > bound {bound:.4e}"
    return err


# --------------------------------------------------------------------------- the median / mean pass
ALIGNS = ("none", "scale", "affine")


def _members(E, HW, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(1, HW, generator=g)
    return (base + 0.15 * torch.randn(E, HW, generator=g)) * (0.6 + 0.8 * torch.rand(E, 1, generator=g)) - 0.1


def _param(E, align, seed):
    """float64 copies of fp32 scales / shifts, as the oracle's ``depth_align`` takes them; None without alignment."""
    if align == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    s = (0.7 + 0.6 * torch.rand(E, generator=g)).double().numpy()
    t = (0.1 * torch.randn(E, generator=g)).double().numpy()
    return s if align == "scale" else np.concatenate([s, t])


def _aligned(d, param, align):
    """[E,1,1,HW] fp32: the members as the kernel must see them - two separately rounded fp32 operations."""
    from oracle import ensemble as oens
    x = d.reshape(d.shape[0], 1, 1, d.shape[1])
    return x if param is None else oens.depth_align(x, param, True, align == "affine")


def _median_pass(dev, d, param, align, reduction, want_unc, want_med=True, off=GUARD, d_off=0, name=""):
    """One MG_OP_ENS_DEPTH_MEDIAN launch -> (med, unc | None, minmax) on the CPU, guards checked.
    ``d_off``: the members start that many floats into their allocation (1: not 16-byte aligned)."""
    from marigold_amd import ops
    E, HW = d.shape
    dbuf = torch.full((d_off + E * HW,), NAN, device=dev)
    dbuf[d_off:] = d.reshape(-1).to(dev)
    dd = dbuf[d_off:].view(E, HW)
    st = None
    if param is not None:
        p = np.asarray(param, dtype=np.float64)
        p = p if align == "affine" else np.concatenate([p, np.full(E, NAN)])   # has_shift = 0: the shifts must not be read
        st = torch.from_numpy(p).float().to(dev)
    med = _Out(HW, dev, off) if want_med else None
    unc = _Out(HW, dev, off) if want_unc else None
    mm = _Out(2 + 2 * E, dev)
    scratch = torch.empty(12288, dtype=torch.uint8, device=dev)
    _run(ops.ens_depth_median(dd, st, med.view if med else None, unc.view if unc else None, mm.view, scratch, E=E, HW=HW,
                              reduction=0 if reduction == "median" else 1, has_shift=align == "affine"))
    return (med.get(name + " med") if med else None, unc.get(name + " unc") if unc else None, mm.get(name + " minmax"))


def _first(mask):
    return int(mask.reshape(-1).nonzero()[0])


def _check_minmax(name, mm, pred, d):
    """minmax = [min, max, members at the first pixel of the minimum, members at the first pixel of the maximum]; a NaN
    prediction makes min and max NaN (torch's .min() / .max()); the members beside them are pixel 0's (csrc/ensemble.hip: the
    sub-gradient they feed means nothing on a NaN cost, but they must be values of the map)."""
    E = d.shape[0]
    pred = pred.reshape(-1)
    _same(f"{name} minmax[0:2] = (min, max) of the prediction", mm[:2], torch.stack([pred.min(), pred.max()]))
    nan = torch.isnan(pred)
    pmin = 0 if nan.any() else _first(pred == pred.min())
    pmax = 0 if nan.any() else _first(pred == pred.max())
    _same(f"{name} minmax: members at the lowest pixel of the minimum ({pmin})", mm[2:2 + E], d[:, pmin])
    _same(f"{name} minmax: members at the lowest pixel of the maximum ({pmax})", mm[2 + E:], d[:, pmax])


def _check_median_case(dev, name, d, param, align, reduction, want_unc, **kw):
    """One launch against the oracle; -> dict of the figures worth printing."""
    from oracle import ensemble as oens
    E, HW = d.shape
    a = _aligned(d, param, align)
    pred, unc = oens.depth_reduce(a, reduction, want_unc)
    med, u, mm = _median_pass(dev, d, param, align, reduction, want_unc, name=name, **kw)
    fig = {}
    if reduction == "median":
        # the value of rank (E - 1) // 2 does not depend on how ties are broken: bit-equal
        _same(f"{name} median", med, pred)
        if want_unc:
            _same(f"{name} MAD", u, unc)
        _check_minmax(name, mm, pred, d)
    else:
        a64 = a.double().reshape(E, HW)
        fin = torch.isfinite(a64)
        amax = float(a64[fin].abs().max()) if fin.any() else 0.0
        mean_bound = E * 2.0 ** -23 * amax      # sequential fp32 sum of E terms + the divide, worst case
        fig["mean_err"] = _within(f"{name} mean", med, a64.mean(0), mean_bound)
        fig["mean_bound"] = mean_bound
        if want_unc:
            # torch.std of one member is NaN (0 / 0); the kernel divides by max(E - 1, 1): 0.  Both are "no spread known";
            # the engine never asks for the uncertainty of one member (pipeline: ensemble_size > 1)
            std64 = a64.std(0) if E > 1 else torch.zeros(HW, dtype=torch.float64)
            ok = torch.isfinite(std64)
            own = float((unc.reshape(-1).double() - std64)[ok].abs().max()) if (E > 1 and ok.any()) else 0.0
            std_bound = max(4.0 * own, mean_bound)
            fig["std_err"] = _within(f"{name} std", u, std64, std_bound)
            fig["std_own"], fig["std_bound"] = own, std_bound
        # min / max and the extremal pixel: exact, of the map this launch returned (itself held to the float64 bound above -
        # torch's fp32 mean need not sum in the kernel's order, so its min could differ in the last bit)
        _check_minmax(name, mm, med, d)
    return fig, (med, u, mm)


E_LIST = [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 16, 17, 31, 32, 33, 64, 128, 129, 257]
HW_SCALAR = [1, 3, 255, 256, 257, 1023]     # HW % 4 != 0, or too short for anything but the tail ... (256: vector path, one block)
HW_VECTOR = [1024, 1280]


@pytest.mark.parametrize("reduction", ["median", "mean"])
@pytest.mark.parametrize("E", E_LIST)
def test_depth_median_every_member_count(dev, E, reduction):
    """1a: every dispatch form x alignment x with / without the uncertainty output x scalar tail and vector path."""
    for align in ALIGNS:
        worst = {}
        for HW in HW_SCALAR + HW_VECTOR:
            d = _members(E, HW, 1000 * E + HW)
            param = _param(E, align, 7 * E + HW)
            name = f"ens_depth_median E={E} {reduction} align={align} HW={HW}"
            fig, (med1, _, mm1) = _check_median_case(dev, name + " +unc", d, param, align, reduction, True)
            fig0, (med0, _, mm0) = _check_median_case(dev, name + " -unc", d, param, align, reduction, False)
            # without the uncertainty output: the same map and the same min / max
            _same(name + ": med with and without the uncertainty output", med0, med1)
            _same(name + ": minmax with and without the uncertainty output", mm0, mm1)
            # the optimiser's form: no map at all
            _, _, mmn = _median_pass(dev, d, param, align, reduction, False, want_med=False, name=name + " no outputs")
            _same(name + ": minmax without any map output", mmn, mm1)
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
        path = f"scalar HW={HW_SCALAR} vector HW={HW_VECTOR}"
        if reduction == "median":
            print(f"[parity] ens_depth_median E={E} median align={align}: median, MAD, min/max and extremal pixels bit-equal to the oracle; {path}")
        else:
            print(f"[parity] ens_depth_median E={E} mean align={align}: mean max|err| {worst['mean_err']:.3e} (bound E*2^-23*max|a| up to "
                  f"{worst['mean_bound']:.3e}); std max|err| {worst['std_err']:.3e}, torch fp32 std's own {worst['std_own']:.3e}, "
                  f"bound {worst['std_bound']:.3e}; {path}")


def _tied_members(E, HW, seed):
    """Multiples of 1/8 in [0.625, 1.375], about a third of the members copies of another one, plus a slow wave, clamped to [0.5, 1.5]:
    the median sits on the plateau 1.5 over a stretch that begins some way into the map, and on 0.5 over a later one - the
    first pixel of either is in the interior, not pixel 0."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(5, 12, (E, HW), generator=g).float() / 8
    for e in range(1, E, 3):
        d[e] = d[int(torch.randint(0, e, (1,), generator=g))]
    wave = (1.25 * torch.sin(torch.linspace(0.0, 3.0 * math.pi, HW)) * 8).round() / 8
    return (d + wave).clamp_min(0.5).clamp_max(1.5)


@pytest.mark.parametrize("E", [4, 9, 10, 16, 40, 129])
def test_depth_median_ties_and_plateaus(dev, E):
    """1b: equal values within a pixel (rank counting's index tie-break, the sorting network, the bitwise selection) and equal
    extrema across threads, waves and blocks (the lowest pixel wins)."""
    for HW in (1023, 3072):
        d = _tied_members(E, HW, 50 + E)
        for align, param in (("none", None), ("affine", np.concatenate([np.full(E, 2.0), np.full(E, 0.25)]))):
            name = f"ens_depth_median ties E={E} HW={HW} align={align}"
            _, (med, mad, mm) = _check_median_case(dev, name, d, param, align, "median", True)
            nmin, nmax = int((med == med.min()).sum()), int((med == med.max()).sum())
            assert nmin > 8 and nmax > 8, f"{name}: the plateau did not form ({nmin}, {nmax} pixels)"
            assert _first(med == med.min()) > 64 and _first(med == med.max()) > 4, f"{name}: a plateau begins at the first pixels"
            print(f"[parity] {name}: bit-equal; {nmin} pixels share the minimum, {nmax} the maximum, lowest pixel reported; "
                  f"{int((mad == 0).sum())} pixels with MAD 0")


@pytest.mark.parametrize("E", [5, 10, 17, 40, 129])
def test_depth_median_misaligned_buffers(dev, E):
    """1c: an HW % 4 == 0 map whose members, median and MAD start one float past a 16-byte boundary takes the scalar path
    and gives the aligned run's bits."""
    HW = 1280
    d = _members(E, HW, 77 + E)
    param = _param(E, "affine", 78 + E)
    for reduction in ("median", "mean"):
        name = f"ens_depth_median misaligned E={E} {reduction}"
        _, (med, unc, mm) = _check_median_case(dev, name + " aligned", d, param, "affine", reduction, True)
        _, (med1, unc1, mm1) = _check_median_case(dev, name + " offset by one float", d, param, "affine", reduction, True,
                                                  off=GUARD + 1, d_off=1)
        _same(name + " med", med1, med)
        _same(name + " unc", unc1, unc)
        _same(name + " minmax", mm1, mm)
        print(f"[parity] {name}: scalar path (views offset by one float) bit-equal to the vector path")


@pytest.mark.parametrize("HW,path", [(769 * 771, "scalar"), (768 * 768, "vector")])
@pytest.mark.parametrize("E", [5, 17])
def test_depth_median_grid_stride(dev, E, HW, path):
    """1c: more pixels than one trip of the grid covers (512 blocks x 256 threads x 1 or 4 pixels), with plateaus so that the
    extremal value ties across blocks and trips."""
    d = _tied_members(E, HW, 90 + E)
    name = f"ens_depth_median grid stride E={E} HW={HW} ({path} path)"
    _, (med, mad, mm) = _check_median_case(dev, name, d, None, "none", "median", True)
    d = _members(E, HW, 92 + E)
    _check_median_case(dev, name + " affine", d, _param(E, "affine", 93 + E), "affine", "median", True)
    print(f"[parity] {name}: median, MAD, min/max bit-equal; {int((med == med.min()).sum())} pixels share the minimum")


# --------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("E", [1, 2, 31, 32, 33, 64, 65, 100, 257])
def test_depth_stats(dev, E):
    """1d: MG_OP_ENS_DEPTH_STATS across its column chunks of 32 members and its pixel-block caps, against float64."""
    from marigold_amd import ops
    for HW in (1, 255, 257, 40000):
        d = _members(E, HW, 300 + E + HW)
        nblk = min(-(-HW // 256), 32 if E > 256 else 128)
        scratch = torch.empty(nblk * E * (E + 3), dtype=torch.float64, device=dev)
        out = _Out(3 * E + E * E, dev, dtype=torch.float64)
        dd = d.to(dev)
        _run(ops.ens_depth_stats(dd, scratch, out.view, E=E, HW=HW))
        st = out.get(f"ens_depth_stats E={E} HW={HW}")
        d64 = d.double()
        name = f"ens_depth_stats E={E} HW={HW}"
        _same(name + " min", st[:E], d64.min(1).values)
        _same(name + " max", st[E:2 * E], d64.max(1).values)
        dmax = float(d64.abs().max())
        mean_bound = 2.0 ** -50 * HW * dmax
        mean_err = float((st[2 * E:3 * E] - d64.mean(1)).abs().max())
        assert mean_err <= mean_bound, f"{name}: mean max|err| {mean_err:.3e} > {mean_bound:.3e}"
        cen = d64 - d64.mean(1, keepdim=True)
        Cref = cen @ cen.t() / HW
        # products and partial sums of up to 64 of them are fp32: 65 roundings of relative 2^-24 on terms of size |d_i d_j|
        bound = 65 * U32 * (d64.abs() @ d64.abs().t() / HW)
        ratio = float(((st[3 * E:].reshape(E, E) - Cref).abs() / bound).max())
        print(f"[parity] {name}: min/max exact, mean max|err| {mean_err:.2e} (bound {mean_bound:.2e}), "
              f"C max|err| / (65 * 2^-24 * mean|d_i d_j|) = {ratio:.3f}")
        assert ratio <= 1.0, f"{name}: C off by {ratio:.3f} x its bound"


# --------------------------------------------------------------------------- normals
def _normals_members(E, HW, seed):
    """[E,3,HW] fp32 members of length 0.8 ... 0.95 around a common direction (the cosines stay clear of the ill-conditioned
    arccos near +-1), resampled wherever - in float64 - the two best cosines are closer than 1e-4: fp32 rounding cannot
    decide the closest member there.  Pixel 0: all members the same vector of length 1.2 (cosine 1.2: the clamp); pixel 1 at
    E = 2: a vector and its negative (zero mean: the 1e-6 floor of the norm)."""
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        base = F.normalize(torch.randn(1, 3, n, generator=g, dtype=torch.float64), dim=1)
        x = F.normalize(base + 0.35 * torch.randn(E, 3, n, generator=g, dtype=torch.float64), dim=1)
        return (x * (0.8 + 0.15 * torch.rand(E, 1, n, generator=g, dtype=torch.float64))).float()

    n = draw(HW)
    for _ in range(16):
        if E == 1:
            break
        x = n.double()
        mean = x.mean(0, keepdim=True)
        mean = mean / mean.norm(dim=1, keepdim=True).clamp(min=1e-6)
        top = (mean * x).sum(1).clamp(-1, 1).topk(2, dim=0).values
        bad = (top[0] - top[1]) < 1e-4
        if not bad.any():
            break
        n[:, :, bad] = draw(int(bad.sum()))
    n[:, :, 0] = 1.2 * F.normalize(torch.tensor([1.0, -2.0, 0.5]), dim=0)
    if E == 2 and HW > 1:
        n[1, :, 1] = -n[0, :, 1]
    return n


NORMALS_CASES = [(E, HW) for E in (1, 2, 3, 10, 40) for HW in (1, 257, 1280)] + [(3, 769 * 771)]


@pytest.mark.parametrize("E,HW", NORMALS_CASES)
def test_normals(dev, E, HW):
    """1e: MG_OP_ENS_NORMALS, both reductions, against the oracle on inputs where the oracle's own fp32 and float64
    evaluations pick the same member at every pixel (asserted: the 0.1 % allowance is never spent by the reference)."""
    from marigold_amd import ops
    from oracle import ensemble as oens
    n = _normals_members(E, HW, 400 + E)
    x = n.reshape(E, 3, 1, HW)
    ref, unc = oens.ensemble_normals(x, output_uncertainty=True, reduction="closest")
    ref64, unc64 = oens.ensemble_normals(x.double(), output_uncertainty=True, reduction="closest")
    assert torch.equal(ref.double(), ref64), "the oracle's fp32 and float64 evaluations pick different members on this input"
    mean, _ = oens.ensemble_normals(x, reduction="mean")
    own = float((unc.double() - unc64).abs().max())
    nd = n.to(dev)
    name = f"ens_normals E={E} HW={HW}"
    out, u = _Out(3 * HW, dev), _Out(HW, dev)
    _run(ops.ens_normals(nd, out.view, u.view, E=E, HW=HW, reduction=0))
    got, gu = out.get(name + " closest"), u.get(name + " unc")
    same = float((got.reshape(3, HW) == ref.reshape(3, HW)).all(0).float().mean())
    uerr = _within(name + " uncertainty", gu, unc.double(), 1e-5)
    out2, u2 = _Out(3 * HW, dev), _Out(HW, dev)
    _run(ops.ens_normals(nd, out2.view, u2.view, E=E, HW=HW, reduction=1))
    merr = _within(name + " mean", out2.get(name + " mean"), mean.double(), 1e-5)
    _same(name + " uncertainty of the mean reduction", u2.get(name + " unc (mean)"), gu)
    out3 = _Out(3 * HW, dev)
    _run(ops.ens_normals(nd, out3.view, None, E=E, HW=HW, reduction=0))
    _same(name + " closest without the uncertainty output", out3.get(name + " closest, no unc"), got)
    print(f"[parity] {name}: identical closest member on {same * 100:.3f}% of pixels; uncertainty max|err| {uerr:.2e} "
          f"(the oracle's fp32 vs float64: {own:.2e}), mean max|err| {merr:.2e}")
    assert same >= 0.999


# --------------------------------------------------------------------------- post tails
def _post_ref(x, post, Cout, scale, dtype):
    """The torch expressions the header cites (marigold_depth_pipeline.py:515,473-475; marigold_normals_pipeline.py:438-440;
    marigold_iid_pipeline.py:523-526) on x [B,HW,Cout] -> NCHW [B,C',HW]."""
    from marigold_amd import _lib as L
    v = (x.to(dtype) * (1.0 if scale == 0 else scale)).permute(0, 2, 1)
    if post == L.POST_DEPTH:
        return (torch.clip(v.mean(dim=1, keepdim=True), -1.0, 1.0) + 1.0) / 2.0
    if post == L.POST_NORMALS:
        v = torch.clip(v, -1.0, 1.0)
        return v / torch.norm(v, dim=1, keepdim=True).clamp(min=1e-6)
    if post == L.POST_UNIT:
        return (torch.clip(v, -1.0, 1.0) + 1.0) / 2.0
    return v


def _post_modes():
    from marigold_amd import _lib as L
    return [("none", L.POST_NONE, (1, 3, 4)), ("depth", L.POST_DEPTH, (1, 3, 4)), ("normals", L.POST_NORMALS, (3,)),
            ("unit", L.POST_UNIT, (1, 3, 4))]


def _post_run(dev, x, post, Cout, ldi, scale, name):
    """x [B,HW,Cout] fp32 -> the kernel's NCHW output on the CPU; the padding columns of the input hold NaN."""
    from marigold_amd import _lib as L, ops
    B, HW, _ = x.shape
    inp = torch.full((B * HW, ldi), NAN)
    inp[:, :Cout] = x.reshape(B * HW, Cout)
    Co = 1 if post == L.POST_DEPTH else Cout
    out, inp = _Out(B * Co * HW, dev), inp.to(dev)
    _run(ops.post_nchw(inp, out.view, B=B, HW=HW, Cout=Cout, ldi=ldi, post=post, scale=scale))
    return out.get(name).reshape(B, Co, HW)


def _post_check(dev, x, mode, post, Cout, ldi, scale, name):
    from marigold_amd import _lib as L
    got = _post_run(dev, x, post, Cout, ldi, scale, name)
    ref32, ref64 = _post_ref(x, post, Cout, scale, torch.float32), _post_ref(x, post, Cout, scale, torch.float64)
    _same_mask(name + " vs torch fp32", got, ref32)
    fin = torch.isfinite(ref64)
    scale_ref = float(ref64[fin].abs().max()) if fin.any() else 0.0
    bound = 2 * 2.0 ** -23 * scale_ref      # 2 ulp of the fp32 result: at most four rounded operations per element
    own = float((ref32.double() - ref64)[fin].abs().max()) if fin.any() else 0.0
    if post == L.POST_NORMALS:              # product, squares, sum, sqrt, divide: twice the torch fp32 expression's own error
        bound = max(bound, 2 * own)
    err = _within(name, got, ref64, bound)
    return err, bound, own


def _post_values(B, HW, Cout, seed):
    """Values on both sides of +-1, exactly +-1, zero vectors."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, Cout, generator=g) * 0.9
    if HW >= 8:
        x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 1.0, -1.0, 0.0, 2.5
        x[-1, -1], x[-1, -2] = -3.0, 1e-8
        x[0, 4, 0], x[0, 5, 0] = 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23
    else:
        # the bound is relative to max|ref|: a map of one or two pixels must hold a value of the output's natural size, or it
        # measures the cancellation in (m + 1) near m = -1, which the torch expression has as well
        x[0, 0] = 0.75
    return x


def test_post_tails_on_their_own(dev):
    """1f: MG_OP_POST_NCHW fed directly - no convolution in front, whose 1.5e-2 tolerance would hide a wrong constant."""
    for mode, post, couts in _post_modes():
        for Cout in couts:
            for ldi in (4, 8):
                for scale in (0.0, 1.0 / 0.18215, 0.37):
                    for B, HW in ((1, 1), (2, 1), (2, 37), (3, 1000)):
                        x = _post_values(B, HW, Cout, 500 + Cout + ldi + HW)
                        if scale > 1:
                            x = x / scale      # keep values on both sides of +-1 after the scale
                        name = f"post_nchw/{mode} Cout={Cout} ldi={ldi} scale={scale:.4g} B={B} HW={HW}"
                        err, bound, own = _post_check(dev, x, mode, post, Cout, ldi, scale, name)
                print(f"[parity] post_nchw/{mode} Cout={Cout} ldi={ldi}: last case max|err| {err:.3e} bound {bound:.3e} "
                      f"(torch fp32 vs float64: {own:.3e})")


def test_post_tails_grid_stride(dev):
    """1f: more pixels than 8192 blocks x 256 threads cover in one trip; B > 1 with an odd HW."""
    B, HW = 3, 700001
    assert B * HW > 8192 * 256
    for mode, post, couts in _post_modes():
        Cout = couts[-1] if mode != "depth" else 3
        x = _post_values(B, HW, Cout, 600 + Cout)
        err, bound, own = _post_check(dev, x, mode, post, Cout, 4, 0.0, f"post_nchw/{mode} grid stride")
        print(f"[parity] post_nchw/{mode} Cout={Cout} B*HW={B * HW}: max|err| {err:.3e} bound {bound:.3e}")


# --------------------------------------------------------------------------- non-finite input: the reference's mask
@pytest.mark.parametrize("bad", [NAN, INF, -INF], ids=["nan", "+inf", "-inf"])
def test_nonfinite_post_tails(dev, bad):
    """1g: a non-finite value in one channel of one pixel: torch.clip keeps NaN (and clips +-inf to +-1), clamp(min=eps) of a
    NaN norm is NaN - every mode's non-finite outputs are exactly the reference's."""
    for mode, post, couts in _post_modes():
        for Cout in couts:
            B, HW = 2, 300
            x = _post_values(B, HW, Cout, 700 + Cout)
            x[1, 123, Cout - 1] = bad
            x[0, 7, 0] = bad
            name = f"post_nchw/{mode} Cout={Cout} with {bad} in one channel of two pixels"
            ref = _post_ref(x, post, Cout, 0.5, torch.float32)
            err, bound, _ = _post_check(dev, x, mode, post, Cout, 4, 0.5, name)
            print(f"[parity] {name}: {int((~torch.isfinite(ref)).sum())} non-finite outputs as in the reference, "
                  f"rest max|err| {err:.3e} (bound {bound:.3e})")


@pytest.mark.parametrize("bad", [NAN, INF], ids=["nan", "+inf"])
@pytest.mark.parametrize("E", [3, 10, 16, 40, 129])
def test_nonfinite_median_pass(dev, E, bad):
    """1g: one non-finite value in one member at one pixel.  torch.median, mean, std, .min() and .max() propagate NaN: the
    map is NaN where the oracle's is, and min / max of a map with a NaN are NaN."""
    from oracle import ensemble as oens
    for HW, px in ((1023, 517), (1280, 1279)):
        for reduction in ("median", "mean"):
            for align in ("none", "affine"):
                d = _members(E, HW, 800 + E)
                d[E // 2, px] = bad
                name = f"ens_depth_median E={E} {reduction} align={align} HW={HW} with {bad} in member {E // 2} at pixel {px}"
                param = _param(E, align, 801 + E)
                pred, unc = oens.depth_reduce(_aligned(d, param, align), reduction, True)
                _, (_, _, mm_full) = _check_median_case(dev, name, d, param, align, reduction, True)
                if bad != bad:
                    assert torch.isnan(mm_full[:2]).all(), f"{name}: min / max of a map with a NaN must be NaN, got {mm_full[:2].tolist()}"
                _, _, mm = _median_pass(dev, d, param, align, reduction, False, want_med=False, name=name)
                _same(name + ": minmax in the optimiser's form (no map output)", mm, mm_full)
                print(f"[parity] {name}: prediction NaN at {int(torch.isnan(pred).sum())} pixels, uncertainty at "
                      f"{int(torch.isnan(unc).sum())}, min/max ({pred.min().item()}, {pred.max().item()}) - as the oracle")


def _depth_members_2d(E, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = 0.2 + 0.6 * (0.5 * yy + 0.5 * xx * yy)
    s = 0.5 + torch.rand(E, 1, 1, 1, generator=g)
    t = 0.2 * torch.randn(E, 1, 1, 1, generator=g)
    return (base[None, None] + 0.02 * torch.randn(E, 1, H, W, generator=g)) * s + t


@pytest.mark.parametrize("bad", [NAN, INF], ids=["nan", "+inf"])
@pytest.mark.parametrize("E", [5, 40])
def test_nonfinite_ensemble_depth(dev, E, bad):
    """1g: the whole ``ensemble_depth`` with one non-finite pixel in one member: the reference's alignment ends on a NaN cost
    and its output and uncertainty are NaN everywhere - never a finite, normalised, plausible map.  The call returns within
    the iterations it was given."""
    from marigold_amd import ensemble as ens
    from oracle import ensemble as oens
    x = _depth_members_2d(E, 24, 32, 900 + E)
    x[E // 2, 0, 11, 17] = bad
    for reduction in ("median", "mean"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref, runc = oens.ensemble_depth(x.clone(), True, True, output_uncertainty=True, reduction=reduction, max_iter=5)
            got, unc, info = ens.ensemble_depth(x.to(dev), True, True, output_uncertainty=True, reduction=reduction, max_iter=5,
                                                return_info=True)
        name = f"ensemble_depth E={E} {reduction} with {bad} at one pixel of member {E // 2}"
        print(f"[parity] {name}: oracle non-finite at {int((~torch.isfinite(ref)).sum())} / {ref.numel()} pixels, engine at "
              f"{int((~torch.isfinite(got)).sum())}; {info['n_iter']} iterations, {info['n_eval']} evaluations, status {info.get('status')}")
        assert not torch.isfinite(ref).any(), "the oracle is expected to give an all-NaN map here (tests/test_oracle_ensemble.py)"
        _same_mask(name + " map", got.cpu(), ref)
        _same_mask(name + " uncertainty", unc.cpu(), runc)
        assert info["n_iter"] <= 5


@pytest.mark.parametrize("bad", [NAN, INF], ids=["nan", "+inf"])
def test_nonfinite_ensemble_iid_and_normals(dev, bad):
    """1g: ``ensemble_iid`` (median + MAD, mean + std) and ``ensemble_normals`` (closest, mean) on the same pattern."""
    from marigold_amd import ensemble as ens
    from oracle import ensemble as oens
    g = torch.Generator().manual_seed(950)
    for E in (5, 40):
        t = torch.rand(E, 3, 24, 32, generator=g)
        t[E // 2, 1, 11, 17] = bad
        for reduction in ("median", "mean"):
            ref, runc = oens.ensemble_iid(t.clone(), True, reduction)
            got, unc = ens.ensemble_iid(t.to(dev), True, reduction)
            name = f"ensemble_iid E={E} {reduction} with {bad}"
            if bad != bad or reduction == "mean":   # (one +inf of E sorts last: median and MAD stay numbers)
                assert (~torch.isfinite(ref)).any() and (~torch.isfinite(runc)).any()
            _same_mask(name + " prediction", got.cpu(), ref)
            _same_mask(name + " uncertainty", unc.cpu(), runc)
            fin = torch.isfinite(ref)
            assert float((got.cpu() - ref)[fin].abs().max()) <= E * 2.0 ** -23
        n = _normals_members(E, 24 * 32, 960 + E).reshape(E, 3, 24, 32).contiguous()
        n[E // 2, 2, 11, 17] = bad
        for reduction in ("closest", "mean"):
            ref, runc = oens.ensemble_normals(n.clone(), True, reduction)
            got, unc = ens.ensemble_normals(n.to(dev), True, reduction)
            name = f"ensemble_normals E={E} {reduction} with {bad}"
            assert (~torch.isfinite(runc)).any()
            _same_mask(name + " prediction", got.cpu(), ref)
            _same_mask(name + " uncertainty", unc.cpu(), runc)
            if reduction == "closest":   # all cosines NaN: torch's argmax and the kernel both take member 0
                _same(name + " vector at the non-finite pixel", got.cpu()[0, :, 11, 17], ref[0, :, 11, 17])
            print(f"[parity] {name}: prediction non-finite at {int((~torch.isfinite(ref)).sum())} elements, uncertainty at "
                  f"{int((~torch.isfinite(runc)).sum())} - as the oracle")


def test_nonfinite_end_to_end(dev):
    """1g: the tiny synthetic depth pipeline, E = 3, a caller-supplied initial latent with one NaN in member 1.  The oracle
    pipeline returns an all-NaN map; the engine's ``depth_np`` has the same non-finite mask."""
    import marigold_amd as M
    from marigold_amd import schedulers as S, synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.modules import AutoencoderKLHIP, UNet2DConditionModelHIP
    from oracle import pipeline as opipe
    from oracle.schedulers import DDIMScheduler as ODDIM
    from oracle.sd2_unet import UNet2DConditionModel
    from oracle.sd2_vae import AutoencoderKL
    usd, vsd = syn.synthetic_unet_state_dict(TINY_UNET), syn.synthetic_vae_state_dict(TINY_VAE)
    ounet = UNet2DConditionModel(block_out_channels=TINY_UNET.block_out_channels, attention_head_dim=TINY_UNET.heads,
                                 cross_attention_dim=TINY_UNET.cross_attention_dim).eval()
    ounet.load_state_dict(usd)
    ovae = AutoencoderKL(block_out_channels=TINY_VAE.block_out_channels).eval()
    ovae.load_state_dict(vsd)
    ctx = syn.synthetic_text_embedding(TINY_UNET.cross_attention_dim)
    eunet = UNet2DConditionModelHIP(usd, TINY_UNET).to("cuda:0")
    eunet.set_context(ctx)
    evae = AutoencoderKLHIP(vsd, TINY_VAE).to("cuda:0")
    pipe = M.MarigoldDepthPipeline(unet=eunet, vae=evae, scheduler=S.DDIMScheduler(), empty_text_embed=ctx,
                                   default_denoising_steps=4, default_processing_resolution=0)
    img = syn.synthetic_image(64, 128, seed=0)
    lat0 = syn.synthetic_latents(3, 8, 16, seed=2024)
    lat0[1, 2, 3, 5] = NAN
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, _, preds = opipe.predict("depth", ounet, ovae, ODDIM(), img, lat0, ctx, 2)
        out = pipe(img, denoising_steps=2, ensemble_size=3, processing_res=0, color_map=None, show_progress_bar=False,
                   init_latents=lat0)
    ref = ref.squeeze()
    got = torch.from_numpy(out.depth_np)
    print(f"[parity] pipeline depth E=3 with a NaN in member 1's initial latent: oracle members non-finite at "
          f"{[int((~torch.isfinite(p)).sum()) for p in preds]} pixels, oracle map at {int((~torch.isfinite(ref)).sum())} / {ref.numel()}, "
          f"engine map at {int((~torch.isfinite(got)).sum())}")
    assert not torch.isfinite(ref).any(), "the oracle pipeline is expected to return an all-NaN map here"
    _same_mask("pipeline depth_np", got, ref.float())
