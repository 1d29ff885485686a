"""Normalisation statistics where the mean dwarfs the spread.  Every normalisation in the engine takes (sum, sum of squares) in
one pass - fp32 partials, fp64 for the last combine - and var = E[x^2] - mean^2 loses digits as (mean / sigma)^2.  The ladder of
tests/norm_ladder.py (r = |mean| / sigma in {0, 4, 16, 32, 64}) runs through every site that takes such statistics and through
every consumer of them: GN_STATS -> GN_FINALIZE -> GN_APPLY (and the fused finalize), GN_SLAB's six register forms and its
statistics-only form, the patch convolution's GroupNorm by-product, ln_out of the tile GEMM, MG_EPI_XATTN2, MG_OP_ROWGEMM's four
sites, the folded LayerNorm in ops.linear / ops.rowgemm and the GroupNorm fix-up fused into conv3x3 / rowgemm.

References are float64, from the operands as stored; every element is compared; outputs start as NaN.  Bounds (none taken from
what the kernels give): 16-bit and fp32 outputs - what the suite uses for that form at every rung (1.5e-2, 2e-2 with the folded
LayerNorm, 2e-3 for the fp32 epilogue); statistics (rstd, GroupNorm scale, LayerNorm mean) - relative to max|ref|,
2e-4 * max(1, (r / 32)^2): the suite's statistics bound, times the growth of var's condition number past the anchor rung;
GroupNorm (scale, shift) also as the map they define, evaluated at mean_g + {-2, 0, 2} sigma_g of every channel; a constant group
(var <= 0, the clamp) - the output within 1.5e-2 max|beta| of beta.  Measured figures: docs/history/norm_conditioning.md."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import norm_ladder as NL
from tests.test_gpu_kernels import F16, OP16, _bf, _close, _nhwc, _run, dev  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
TAG = "fp16" if F16 else "bf16"
NAN = float("nan")
RUNGS = list(NL.RUNGS)


def _name(site, form, r):
    return f"normcond | {site} | {form} | r={r} | {TAG}"


def _out(site, form, r, got, ref, tol=1.5e-2):
    _close(_name(site, form, r), got, ref, tol)


def _stat(site, form, r, got, ref, bound=None):
    """A statistic against float64: max|err| <= bound * max|ref|, bound = 2e-4 * max(1, (r / 32)^2) unless given."""
    bound = NL.stats_bound(r) if bound is None else bound
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{site}/{form}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{site}/{form}: non-finite statistic"
    scale = max(ref.abs().max().item(), 1e-12)
    err = (got - ref).abs().max().item()
    print(f"[parity] {_name(site, form, r)}: max|err|={err:.3e} scale={scale:.3e} rel={err / scale:.3e} bound={bound:.1e}")
    assert err <= bound * scale, f"{_name(site, form, r)}: max|err| {err:.4e} > {bound} * {scale:.4e}"


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


def _check_ss(site, form, r, ss, refs, skip=None):
    """GroupNorm (scale, shift) [B][2][C] against float64: the scale, and the map scale * x + shift at the data.  ``skip`` =
    (image, group): the constant group, judged by its output alone."""
    mean, var, sc_ref, sh_ref, _ = refs
    B, C = sc_ref.shape
    cpg = C // NL.GROUPS
    ssd = ss.detach().double().cpu()
    assert torch.isfinite(ssd).all(), f"{site}/{form}: non-finite scale / shift"
    pts = NL.gn_map_points(mean, var, cpg)
    got_map = ssd[:, 0, :, None] * pts + ssd[:, 1, :, None]
    ref_map = sc_ref[:, :, None] * pts + sh_ref[:, :, None]
    got_sc = ssd[:, 0]
    if skip is not None:
        keep = torch.ones(B, C, dtype=torch.bool)
        keep[skip[0], skip[1] * cpg:(skip[1] + 1) * cpg] = False
        got_sc, sc_ref, got_map, ref_map = got_sc[keep], sc_ref[keep], got_map[keep], ref_map[keep]
    _stat(site, form + "/scale", r, got_sc, sc_ref)
    _stat(site, form + "/map", r, got_map, ref_map)


def _check_const_group(site, form, r, out_nchw, ref_nchw, beta, const):
    """out / ref [B, C, H, W]: the constant group within 1.5e-2 max|beta| of beta, every other element to the usual bound."""
    b, gi = const
    cpg = out_nchw.shape[1] // NL.GROUPS
    sl = slice(gi * cpg, (gi + 1) * cpg)
    got = out_nchw.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{site}/{form}: non-finite output"
    want = beta.double()[sl, None, None].expand_as(got[b, sl])
    assert (ref_nchw[b, sl] - want).abs().max().item() <= 1e-9, "the float64 reference of a constant group is beta"
    err = (got[b, sl] - want).abs().max().item()
    bound = 1.5e-2 * beta.abs().max().item()
    print(f"[parity] {_name(site, form + '/constant group', r)}: max|out - beta|={err:.3e} bound={bound:.3e}")
    assert err <= bound, f"{_name(site, form, r)}: constant group off beta by {err:.3e} > {bound:.3e}"
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[b, sl] = False
    _out(site, form + "/other groups", r, got[keep], ref_nchw[keep])


def _gn_inputs(shape, r, const=None):
    B, H, W, C0, C1 = shape
    C = C0 + C1
    x = NL.ladder((B, C, H, W), r, 1, OP16, NL.gn_seed(B, H, W, C), groups=NL.GROUPS, const=const)
    gamma, beta = _affine(C, C)
    return x, gamma, beta


def _sources(x, C0, C1, dev):
    xn = _nhwc(x)
    x0 = xn[..., :C0].contiguous().to(dev, OP16)
    x1 = xn[..., C0:].contiguous().to(dev, OP16) if C1 else None
    return x0, x1


# --------------------------------------------------------------------------- GN_STATS -> GN_FINALIZE -> GN_APPLY
def _gn_chunked(dev, shape, r, eps, silu, const=None):
    from marigold_amd import ops, routes
    B, H, W, C0, C1 = shape
    C, HW = C0 + C1, H * W
    x, gamma, beta = _gn_inputs(shape, r, const)
    refs = NL.gn_reference(x, gamma, beta, eps)
    ref_out = F.silu(refs[4]) if silu else refs[4]
    x0, x1 = _sources(x, C0, C1, dev)
    gd, bd = gamma.to(dev), beta.to(dev)
    nsrc = 2 if C1 else 1
    cnt = torch.zeros(1024, dtype=torch.int32, device=dev)
    for chunks in sorted({routes.gn_stats_chunks(B, HW), 1}, reverse=True):
        slots = nsrc * chunks
        form = f"{B}x{H}x{W}x{C0}+{C1}/chunks{chunks}"
        kw = dict(B=B, HW=HW, C=C0, chunks=chunks, groups=NL.GROUPS, Ctot=C, coff=0, slot0=0, slots=slots, x1=x1, C1=C1)
        part = torch.full((B, slots, NL.GROUPS, 2), NAN, device=dev)
        ss = torch.full((B, 2, C), NAN, device=dev)
        _run(ops.gn_stats(x0, part, **kw))
        _run(ops.gn_finalize(part, gd, bd, ss, B=B, C=C, groups=NL.GROUPS, slots=slots, HW=HW, eps=eps))
        out = torch.full((B, H, W, C), NAN, device=dev, dtype=OP16)
        _run(ops.gn_apply(x0, ss, out, B=B, HW=HW, C=C, silu=silu, x1=x1, C0=C0))
        _check_ss("gn_stats+finalize", form, r, ss, refs, skip=const)
        if const is None:
            _out("gn_apply", form, r, out.float().permute(0, 3, 1, 2), ref_out)
        else:
            _check_const_group("gn_apply", form, r, out.float().permute(0, 3, 1, 2), ref_out, beta, const)
        # the image's last statistics block finalizes: same checks, counters (the tickets) back at zero
        runs = []
        for _ in range(2):
            part.fill_(NAN)
            ss2 = torch.full((B, 2, C), NAN, device=dev)
            _run(ops.gn_stats(x0, part, gamma=gd, beta=bd, ss=ss2, counters=cnt, eps=eps, **kw))
            assert int(cnt.abs().sum()) == 0, "tickets not back at zero"
            runs.append(ss2)
        assert torch.equal(runs[0], runs[1]), "fused finalize not bit-stable"
        _check_ss("gn_stats fused finalize", form, r, runs[0], refs, skip=const)


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("shape", NL.STATS_SHAPES, ids=lambda s: "{}x{}x{}x{}+{}".format(*s))
def test_groupnorm_chunked_statistics(dev, shape, r):
    """One source and two (the group that straddles 640 + 320 gets a share from each), ``chunks`` as the program builder picks
    them and 1 (a thread's longest chain).  chunks = 1 is what found the biased fp32 chains of gn_stats_kernel: before its
    per-batch fp64 totals the scale at 96 x 96 x 320 was off by 1.5e-3 / 6.4e-3 / 3.2e-2 at r = 16 / 32 / 64 on bf16 operands."""
    _gn_chunked(dev, shape, r, eps=1e-5, silu=True)


@pytest.mark.parametrize("r", [0, 32])
def test_groupnorm_chunked_statistics_constant_group(dev, r):
    _gn_chunked(dev, (2, 24, 24, 2560, 0), r, eps=1e-6, silu=False, const=(1, 5))


# --------------------------------------------------------------------------- GN_SLAB
def _slab_id(case):
    (B, H, W, C0, C1, _, _), (nt, rows) = case
    need = NL.slab_form(H * W, C0 + C1)[2]
    cpg = (C0 + C1) // NL.GROUPS
    win = cpg if cpg % 4 == 0 else (2 * cpg if cpg % 2 == 0 else 4 * cpg)     # the window: lcm(channels per group, 4)
    return f"{B}x{H}x{W}x{C0}+{C1}-slab{H * W * win * 2}B-need{need}-form<{nt},{rows}>"


def _gn_slab(dev, case, r, const=None):
    from marigold_amd import ops
    (B, H, W, C0, C1, silu, eps), want_form = case
    if const is not None:
        silu = False
    C, HW = C0 + C1, H * W
    nt, rows, need = NL.slab_form(HW, C)
    assert (nt, rows) == want_form
    form = f"{B}x{H}x{W}x{C0}+{C1}/<{nt},{rows}>"
    x, gamma, beta = _gn_inputs((B, H, W, C0, C1), r, const)
    refs = NL.gn_reference(x, gamma, beta, eps)
    ref_out = F.silu(refs[4]) if silu else refs[4]
    x0, x1 = _sources(x, C0, C1, dev)
    gd, bd = gamma.to(dev), beta.to(dev)
    runs = []
    for _ in range(2):
        ss = torch.full((B, 2, C), NAN, device=dev)
        out = torch.full((B, HW, C), NAN, device=dev, dtype=OP16)
        _run(ops.gn_slab(x0, out, ss, B=B, HW=HW, C=C, groups=NL.GROUPS, gamma=gd, beta=bd, eps=eps, silu=silu, x1=x1, C0=C0))
        ss2 = torch.full((B, 2, C), NAN, device=dev)
        _run(ops.gn_slab(x0, None, ss2, B=B, HW=HW, C=C, groups=NL.GROUPS, gamma=gd, beta=bd, eps=eps, x1=x1, C0=C0))
        runs.append((ss, out, ss2))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "two launches must be bit-identical"
    ss, out, ss2 = runs[0]
    _check_ss("gn_slab", form, r, ss, refs, skip=const)
    _check_ss("gn_slab statistics only", form.replace(f",{rows}>", ",0>"), r, ss2, refs, skip=const)
    got = out.reshape(B, H, W, C).float().permute(0, 3, 1, 2)
    if const is None:
        _out("gn_slab", form + "/out", r, got, ref_out)
    else:
        _check_const_group("gn_slab", form, r, got, ref_out, beta, const)


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("case", NL.SLAB_SHAPES, ids=_slab_id)
def test_groupnorm_one_launch_forms(dev, case, r):
    """One shape per register form of gn_slab_kernel (the id names the form ``need`` and the slab size select), the
    statistics-only form on each, two launches bit for bit."""
    _gn_slab(dev, case, r)


@pytest.mark.parametrize("r", [0, 32])
def test_groupnorm_one_launch_constant_group(dev, r):
    _gn_slab(dev, NL.SLAB_SHAPES[3], r, const=(1, 5))


# --------------------------------------------------------------------------- the patch convolution's by-product
BYPRODUCT_CASES = [   # tests/test_gpu_kernels.py::test_conv3x3_patch_output_groupnorm_statistics
    (2, 48, 32, 128, 128, 8, True, True, False),
    (1, 50, 37, 64, 128, 8, False, False, False),
    (2, 24, 32, 128, 256, 9, True, True, False),
    (1, 24, 16, 64, 512, 9, False, False, False),
    (1, 13, 21, 64, 256, 9, False, False, True),
    (2, 18, 33, 128, 256, 1, False, False, True),
    (1, 32, 16, 64, 256, 1, True, True, False),
]


def _conv_byproduct(dev, case, r, const=None):
    """The group means ride in the bias (per channel: every image carries image 0's) and, where the case has a residual, half in
    the bias and the rest - per image - in the residual.  ``const``: that group's weights are zero, its bias and residual
    constant - the stored output is one value."""
    from marigold_amd import ops, weights as Wm
    B, H, W, Cin, N, variant, fused, use_res, subpix = case
    g = torch.Generator().manual_seed(H * W + N)
    cpg = N // NL.GROUPS
    x = _bf(torch.randn(B, Cin, H, W, generator=g))
    w = _bf(torch.randn(N, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    m = NL.group_means(B, r, H * W + N)                                    # [B, 32] float64
    bias_m = 0.5 * m[0] if use_res else m[0]
    bias = 0.5 * torch.randn(N, generator=g) + bias_m.repeat_interleave(cpg).float()
    ss_in = (torch.stack([1.0 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)], dim=1).to(dev).contiguous()
             if fused else None)
    Ho, Wo = (2 * H, 2 * W) if subpix else (H, W)
    res = None
    if use_res:
        res = torch.randn(B, Ho, Wo, N, generator=g) + (m - bias_m[None]).repeat_interleave(cpg, 1).float()[:, None, None, :]
    if const is not None:
        b, gi = const
        sl = slice(gi * cpg, (gi + 1) * cpg)
        w[sl] = 0.0
        bias[sl] = float(bias_m[gi])
        if use_res:
            res[b, :, :, sl] = float(m[b, gi] - bias_m[gi])
    bias = bias.to(dev)
    res = None if res is None else res.to(dev, OP16)
    xd = _nhwc(x).to(dev, OP16)
    wd = (Wm.pack_conv3x3_subpix(w) if subpix else Wm.pack_conv3x3(w)).to(dev, OP16)
    kw = dict(B=B, H=H, W=W, C0=Cin, N=N, ss=ss_in, silu=fused, bias=bias, residual=res, subpix=subpix, wz=N * 4 * Cin if subpix else 0,
              variant=variant)
    slots = ops.conv3x3_gn_slots(ops.conv3x3(xd, wd, torch.empty(B, Ho, Wo, N, device=dev, dtype=OP16), **kw), F16)
    assert slots > 0
    HW, eps = Ho * Wo, 1e-6
    gamma, beta = _affine(N, N)
    gd, bd = gamma.to(dev), beta.to(dev)
    stored = torch.full((B, Ho, Wo, N), NAN, device=dev, dtype=OP16)
    part = torch.full((B, slots, NL.GROUPS, 2), NAN, device=dev)
    _run(ops.conv3x3(xd, wd, stored, gn_part=part, gn_cpg=cpg, gn_slots=slots, **kw))
    sn = stored.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(sn).all()
    refs = NL.gn_reference(sn, gamma, beta, eps)
    mean, var = refs[0], refs[1]
    form = f"{B}x{H}x{W}x{Cin}->{N}/v{variant}" + ("/fused" if fused else "") + ("/res" if use_res else "") + ("/subpix" if subpix else "")
    if const is not None:
        assert float(var[const]) == 0.0, "the planted group is not constant in the stored output"
    else:
        ratio = mean.abs() / var.sqrt()
        print(f"[ladder] conv by-product {form} r={r}: stored var [{float(var.min()):.3f}, {float(var.max()):.3f}] "
              f"|mean|/sigma [{float(ratio.min()):.2f}, {float(ratio.max()):.2f}]")
        assert r == 0 or (0.5 * r <= float(ratio.min()) and float(ratio.max()) <= 1.4 * r), "the rung is not what it claims"
    ss = torch.full((B, 2, N), NAN, device=dev)
    _run(ops.gn_finalize(part, gd, bd, ss, B=B, C=N, groups=NL.GROUPS, slots=slots, HW=HW, eps=eps))
    chunks = 8
    part2 = torch.full((B, chunks, NL.GROUPS, 2), NAN, device=dev)
    ss2 = torch.full((B, 2, N), NAN, device=dev)
    _run(ops.gn_stats(stored, part2, B=B, HW=HW, C=N, chunks=chunks, groups=NL.GROUPS))
    _run(ops.gn_finalize(part2, gd, bd, ss2, B=B, C=N, groups=NL.GROUPS, slots=chunks, HW=HW, eps=eps))
    _check_ss("conv3x3 by-product+finalize", form, r, ss, refs, skip=const)
    _check_ss("gn_stats+finalize of the conv output", form, r, ss2, refs, skip=const)
    if const is not None:
        for which, s in (("conv3x3 by-product+finalize", ss), ("gn_stats+finalize of the conv output", ss2)):
            out = torch.full((B, Ho, Wo, N), NAN, device=dev, dtype=OP16)
            _run(ops.gn_apply(stored, s, out, B=B, HW=HW, C=N, silu=False))
            _check_const_group(which, form, r, out.float().permute(0, 3, 1, 2), refs[4], beta, const)


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("case", BYPRODUCT_CASES, ids=lambda c: "{}x{}x{}x{}-{}-v{}".format(*c[:6]))
def test_conv3x3_patch_output_statistics(dev, case, r):
    """The by-product table -> GN_FINALIZE, and GN_STATS -> GN_FINALIZE over the stored tensor, each against float64 of the
    stored tensor.  (Their 1e-5 agreement with each other is asserted where it was, at ratio ~ 0.)"""
    _conv_byproduct(dev, case, r)


@pytest.mark.parametrize("r", [0, 32])
@pytest.mark.parametrize("case", [BYPRODUCT_CASES[0], BYPRODUCT_CASES[1]], ids=["fused_res", "ragged_plain"])
def test_conv3x3_patch_output_statistics_constant_group(dev, case, r):
    _conv_byproduct(dev, case, r, const=(0, 5))


# --------------------------------------------------------------------------- row statistics: the tile GEMM
# The cross-attention sites round their probabilities to the 16-bit operand of the second MFMA stage.  At a large mean the scores
# carry an fp32 error of ~1e-5, so now and then the kernel and float64 round a probability to neighbouring values - one ulp, inside
# every output bound, but it moves that row (by ulp * a column of the value table) and with it the row's float64 rstd: measured
# with a value table of the residual's own size, bf16 ulps shifted rstd by 2 - 4.5e-4 of it at r = 16 .. 64 (fp16: 4 - 9e-5)
# while every row without such a flip agreed to 1e-6.  That is the reference's rounding, not the statistics.  The value tables of
# these tests are therefore 1/16 of the residual's spread: the statistics still run over rows of the full magnitude, the flips
# stay 16 times under the statistics bound.
VO_SCALE = 1.0 / 16


def _row_stats_ref(ref):
    mean, _, rstd = NL.ln_reference(ref)
    return mean, rstd


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("N", [320, 1280])
def test_igemm_ln_out(dev, N, r):
    """ln_out of MG_OP_IGEMM: out = a w^T + b + res with the row means planted in the residual; the 32-column slots, then (mean,
    rstd) as the row block's last column tile reduces them - every tile variant of test_igemm_layernorm_fold."""
    from marigold_amd import ops
    M, K0 = 700, 192
    g = torch.Generator().manual_seed(21 + N)
    a = _bf(torch.randn(M, K0, generator=g))
    w0 = _bf(torch.randn(N, K0, generator=g) / math.sqrt(K0))
    b0 = torch.randn(N, generator=g) * 0.1
    res = NL.ladder((M, N), r, -1, OP16, M + N)
    ref0 = a.double() @ w0.double().t() + b0.double() + res.double()
    mean, rstd = _row_stats_ref(ref0)
    ns = N // 32
    want = torch.stack([ref0.reshape(M, ns, 32).sum(-1), (ref0 ** 2).reshape(M, ns, 32).sum(-1)], dim=-1)
    ad, wd, bd, rd = a.to(dev, OP16), w0.to(dev, OP16), b0.to(dev), res.to(dev, OP16)
    for variant in (0, 46, 51, 35, 24, 25, 26, 62, 72, 73):
        runs = []
        for _ in range(2):   # the tickets reset themselves: the second launch finalizes again, to the same bits
            out = torch.full((M, N), NAN, device=dev, dtype=OP16)
            st = torch.full((M * (ns + 1), 2), NAN, device=dev)
            _run(ops.linear(ad, wd, out, M=M, K=K0, N=N, bias=bd, residual=rd, ln_out=st, variant=variant))
            runs.append((out, st))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"v{variant}: launches differ"
        out, st = runs[0]
        form = f"N{N}/v{variant}"
        _out("igemm ln_out", form + "/out", r, out, ref0)
        _stat("igemm ln_out", form + "/slots", r, st[:M * ns].reshape(M, ns, 2), want)
        mr = st[M * ns:]
        _stat("igemm ln_out", form + "/mean", r, mr[:, 0], mean)
        _stat("igemm ln_out", form + "/rstd", r, mr[:, 1], rstd)


def _fold_ref(x, wp, c):
    """The folded LayerNorm in float64 from the operands as stored: LN(x) without its affine (that is inside ``wp`` / ``c``)."""
    mean, _, rstd = NL.ln_reference(x)
    return ((x.double() - mean[:, None]) * rstd[:, None]) @ wp.double().t() + c.double()


def _stx(x, dev):
    """(mean, rstd) of the rows in float64, cast to fp32: what a perfect producer would have written."""
    mean, _, rstd = NL.ln_reference(x)
    return torch.stack([mean, rstd], dim=-1).float().to(dev).contiguous()


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("M,C,heads", [(900, 320, 5), (333, 640, 10), (130, 1280, 20), (128, 64, 1)])
def test_igemm_fused_cross_attention_statistics(dev, M, C, heads, r):
    """MG_EPI_XATTN2 (the launch of test_igemm_fused_cross_attention) with the residual stream carrying the row means: the new
    rows, and their (mean, rstd)."""
    from marigold_amd import _lib as L, ops, weights as Wm
    g = torch.Generator().manual_seed(41 + C)
    npad = 64
    x = NL.ladder((M, C), r, -1, OP16, M + C)
    gamma, beta = _affine(C, C + 1)
    wqk = torch.zeros(npad, C)
    wqk[:2 * heads] = torch.randn(2 * heads, C, generator=g) * (3.0 / math.sqrt(C))
    vot = torch.zeros(C, npad)
    vot[:, :2 * heads] = torch.randn(C, 2 * heads, generator=g) * 0.5 * VO_SCALE
    vot = _bf(vot)
    bias = torch.randn(C, generator=g) * 0.1
    scale = 1.0 / math.sqrt(64)
    wp, gv, cv = Wm.fold_layernorm(wqk, None, gamma, beta)
    sc = _fold_ref(x, wp, cv)[:, :2 * heads].reshape(M, heads, 2) * scale
    P = torch.zeros(M, npad, dtype=torch.float64)
    P[:, :2 * heads] = torch.softmax(sc, dim=-1).reshape(M, 2 * heads)
    ref = P.to(OP16).double() @ vot.double().t() + bias.double() + x.double()
    mean, rstd = _row_stats_ref(ref)
    keep = (wp.to(dev), gv.to(dev), cv.to(dev), vot.to(dev, OP16), bias.to(dev), _stx(x, dev))
    runs = []
    for _ in range(2):
        h = x.to(dev, OP16).clone()
        mr = torch.full((M, 2), NAN, device=dev)
        _run(ops.linear(h, keep[0], h, M=M, K=C, N=npad, epi=L.EPI_XATTN2, ln_in=keep[5], ln_g=keep[1], ln_c=keep[2], sm_scale=scale,
                        sm_cols=2 * heads, out2=keep[3], c2=C, ldo=C, bias=keep[4], residual=h, ldr=C, ln_out=mr))
        runs.append((h, mr))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "not bit-repeatable"
    h, mr = runs[0]
    form = f"M{M} C{C}"
    _out("igemm XATTN2", form + "/rows", r, h, ref)
    _stat("igemm XATTN2", form + "/mean", r, mr[:, 0], mean)
    _stat("igemm XATTN2", form + "/rstd", r, mr[:, 1], rstd)


# --------------------------------------------------------------------------- row statistics: the row-resident GEMM
@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("C,waves", [(320, 12), (320, 8), (320, 4), (640, 8)])
def test_rowgemm_ln_out_forms(dev, C, waves, r):
    """MG_OP_ROWGEMM's ln_out forms: proj_in (GroupNorm scale / shift from float64 applied while the rows are loaded - the tokens
    are a GroupNorm ladder - + bias + row statistics; the bias is per column, so every row carries the same planted mean r) and
    to_out (bias + residual in place + row statistics, the row means planted in the residual).  M = 2112 is no multiple of the
    workgroup's 384 / 256 / 128 rows."""
    from marigold_amd import ops, weights as Wm
    g = torch.Generator().manual_seed(31 + waves + C)
    B, T = 2, 1056
    M = B * T
    # proj_in
    xg = NL.ladder((B, C, T), r, 1, OP16, C + T, groups=NL.GROUPS)                 # [B, C, T]
    gng, gnb = _affine(C, C + 2)
    _, _, sc64, sh64, _ = NL.gn_reference(xg, gng, gnb, 1e-6)
    ss = torch.stack([sc64, sh64], 1).float().contiguous()                          # [B][2][C] as the kernel reads them
    x = xg.permute(0, 2, 1).reshape(M, C).contiguous()
    w = _bf(torch.randn(C, C, generator=g) / math.sqrt(C))
    b = 0.1 * torch.randn(C, generator=g) + float(r)
    pk, ssd, xd = Wm.pack_rowgemm(w, b).to(dev), ss.to(dev), x.to(dev, OP16)
    out, so = torch.full((M, C), NAN, device=dev, dtype=OP16), torch.full((M, 2), NAN, device=dev)
    _run(ops.rowgemm(xd, pk, out, M=M, K=C, N=C, gn_ss=ssd, tokens=T, ln_out=so, waves=waves))
    xn = (x.double().view(B, T, C) * ss[:, 0, None, :].double() + ss[:, 1, None, :].double()).to(OP16).double().view(M, C)
    ref = xn @ w.double().t() + b.double()
    mean, rstd = _row_stats_ref(ref)
    form = f"C{C}/{waves}w"
    _out("rowgemm gn_ss+ln_out", form + "/out", r, out, ref)
    _stat("rowgemm gn_ss+ln_out", form + "/mean", r, so[:, 0], mean)
    _stat("rowgemm gn_ss+ln_out", form + "/rstd", r, so[:, 1], rstd)
    # to_out
    xr = _bf(torch.randn(M, C, generator=g))
    h0 = NL.ladder((M, C), r, -1, OP16, M + C + waves)
    b2 = 0.1 * torch.randn(C, generator=g)
    pk2 = Wm.pack_rowgemm(w, b2).to(dev)
    h, so = h0.to(dev, OP16).clone(), torch.full((M, 2), NAN, device=dev)
    _run(ops.rowgemm(xr.to(dev, OP16), pk2, h, M=M, K=C, N=C, residual=h, ln_out=so, waves=waves))
    ref = xr.double() @ w.double().t() + b2.double() + h0.double()
    mean, rstd = _row_stats_ref(ref)
    _out("rowgemm residual+ln_out", form + "/out", r, h, ref)
    _stat("rowgemm residual+ln_out", form + "/mean", r, so[:, 0], mean)
    _stat("rowgemm residual+ln_out", form + "/rstd", r, so[:, 1], rstd)


def _xattn_setup(C, heads, g, x, gamma, beta):
    """-> (float64 reference of x + attn2(LN(x)) from the operands as stored, folded tables) for the collapsed cross-attention."""
    from marigold_amd import weights as Wm
    ctx = torch.randn(2, 1024, generator=g)
    wq, wo = torch.randn(C, C, generator=g) / math.sqrt(C), torch.randn(C, C, generator=g) * (VO_SCALE / math.sqrt(C))
    wk, wv = torch.randn(C, 1024, generator=g) / 32, torch.randn(C, 1024, generator=g) / 32
    bo = 0.1 * torch.randn(C, generator=g)
    wqk, vot, npad = Wm.cross_attention_tables(wq, wk, wv, wo, ctx, heads)
    wp, lg, lc = Wm.fold_layernorm(wqk, None, gamma, beta)
    M = x.shape[0]
    sc = _fold_ref(x, wp, lc)[:, :2 * heads].reshape(M, heads, 2) / math.sqrt(C // heads)
    P = torch.zeros(M, npad, dtype=torch.float64)
    P[:, :2 * heads] = torch.softmax(sc, dim=-1).reshape(M, 2 * heads)
    ref = P.to(OP16).double() @ vot.to(OP16).double().t() + bo.double() + x.double()
    return ref, (wp, lg, lc, vot, bo)


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("C,heads,waves", [(320, 5, 12), (320, 5, 8), (640, 10, 0), (1280, 20, 0)])
def test_rowgemm_cross_attention_statistics(dev, C, heads, waves, r):
    """MG_OP_ROWGEMM form RG_XATTN (C = 320) and its K-split form (640 / 1280), in place on rows that carry the means."""
    from marigold_amd import _lib as L, ops, weights as Wm
    g = torch.Generator().manual_seed(41 + waves + C)
    M = 2112
    x = NL.ladder((M, C), r, -1, OP16, M + C + waves)
    gamma, beta = _affine(C, C + 3)
    ref, (wp, lg, lc, vot, bo) = _xattn_setup(C, heads, g, x, gamma, beta)
    mean, rstd = _row_stats_ref(ref)
    pk = (Wm.pack_rowgemm_xattn if C == 320 else Wm.pack_rowgemm_xattn_ksplit)(wp.float(), lc, lg, vot, bo).to(dev)
    stx = _stx(x, dev)
    h = x.to(dev, OP16).clone()
    so = torch.full((M, 2), NAN, device=dev)
    _run(ops.rowgemm(h, pk, h, M=M, K=C, N=64, form=L.RG_XATTN, ln_in=stx, ln_out=so, sm_cols=2 * heads,
                     sm_scale=1.0 / math.sqrt(C // heads), waves=waves))
    site = "rowgemm RG_XATTN" if C == 320 else "rowgemm RG_XATTN K-split"
    form = f"C{C}/{waves}w"
    _out(site, form + "/rows", r, h, ref)
    _stat(site, form + "/mean", r, so[:, 0], mean)
    _stat(site, form + "/rstd", r, so[:, 1], rstd)


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("waves", [12, 8, 4])
def test_rowgemm_cross_attention_geglu_prologue_statistics(dev, waves, r):
    """The cross-attention as the GEGLU form's prologue: the statistics of the updated rows never leave the registers - they show
    in the hidden activations (LN3 folded into the GEGLU projection).  The projection's operand is the updated row as stored (16
    bits: at r = 64 a grid of sigma / 2 in bf16), its statistics those of the row before that rounding (weights.fold_layernorm),
    so the float64 reference of the hidden activations takes the stored rows - checked against float64 first - and the float64
    statistics of the unrounded ones."""
    from marigold_amd import _lib as L, ops, weights as Wm
    C, heads = 320, 5
    g = torch.Generator().manual_seed(53 + waves)
    M = 2112
    x = NL.ladder((M, C), r, -1, OP16, M + C + waves + 1)
    g2, b2 = _affine(C, C + 4)
    g3, b3 = _affine(C, C + 5)
    x2, (wpx, lgx, lcx, vot, bo) = _xattn_setup(C, heads, g, x, g2, b2)
    wg, bg = torch.randn(8 * C, C, generator=g) / math.sqrt(C), 0.1 * torch.randn(8 * C, generator=g)
    pkx = Wm.pack_rowgemm_xattn(wpx.float(), lcx, lgx, vot, bo).to(dev)
    order = Wm.rowgemm_geglu_order(8 * C)
    wpg, lgg, lcg = Wm.fold_layernorm(wg[order], bg[order], g3, b3)
    pkg = Wm.pack_rowgemm(wpg.float(), lcg, lgg).to(dev)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(8 * C)
    stx = _stx(x, dev)
    runs = []
    for _ in range(2):
        h_b, hid_b = x.to(dev, OP16).clone(), torch.full((M, 4 * C), NAN, device=dev, dtype=OP16)
        _run(ops.rowgemm(h_b, pkg, hid_b, M=M, K=C, N=8 * C, form=L.RG_GEGLU, ln_in=stx, waves=waves, xattn=pkx, xout=h_b,
                         sm_cols=2 * heads, sm_scale=1.0 / math.sqrt(C // heads)))
        runs.append((h_b, hid_b))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "repeat launches differ"
    form = f"C{C}/{waves}w"
    _out("rowgemm xattn+GEGLU prologue", form + "/rows", r, runs[0][0], x2)
    mean, _, rstd = NL.ln_reference(x2)
    y3 = (runs[0][0].double().cpu() - mean[:, None]) * rstd[:, None]
    u, gt = (y3 @ wpg.double().t() + lcg.double())[:, inv].chunk(2, dim=-1)
    ref_hid = u * F.gelu(gt)
    _out("rowgemm xattn+GEGLU prologue", form + "/hidden", r, runs[0][1], ref_hid, tol=2e-2)


# --------------------------------------------------------------------------- consumers of the statistics
@pytest.mark.parametrize("r", RUNGS)
def test_linear_folded_layernorm_consumers(dev, r):
    """ops.linear's folded LayerNorm, acc * rstd - rstd * mean * g + c, fed the float64 (mean, rstd) cast to fp32: bf16, fp32 and
    GEGLU epilogues and the transposed (V^T) section."""
    from marigold_amd import _lib as L, ops, weights as Wm
    g = torch.Generator().manual_seed(21)
    M, C = 700, 320
    x = NL.ladder((M, C), r, -1, OP16, M + C + 7)
    gamma, beta = _affine(C, C + 6)
    xd, stx = x.to(dev, OP16), _stx(x, dev)
    N = 640
    w, b = torch.randn(N, C, generator=g) / math.sqrt(C), torch.randn(N, generator=g) * 0.1
    wp, gv, cv = Wm.fold_layernorm(w, b, gamma, beta)
    ref = _fold_ref(x, wp, cv)
    keep = (wp.to(dev), gv.to(dev), cv.to(dev))
    for variant in (0, 36, 46, 51, 62, 72, 73):
        out = torch.full((M, N), NAN, device=dev, dtype=OP16)
        _run(ops.linear(xd, keep[0], out, M=M, K=C, N=N, ln_in=stx, ln_g=keep[1], ln_c=keep[2], variant=variant))
        _out("linear ln_in", f"16-bit/v{variant}", r, out, ref, tol=2e-2)
    outf = torch.full((M, N), NAN, device=dev)
    _run(ops.linear(xd, keep[0], outf, M=M, K=C, N=N, epi=L.EPI_F32, ln_in=stx, ln_g=keep[1], ln_c=keep[2]))
    _out("linear ln_in", "fp32 epilogue", r, outf, ref, tol=2e-3)
    # GEGLU
    wg, bg = torch.randn(8 * C, C, generator=g) / math.sqrt(C), torch.randn(8 * C, generator=g) * 0.1
    wpk, bpk = Wm.pack_geglu(wg, bg)
    wpg, gg, cg = Wm.fold_layernorm(wpk, bpk, gamma, beta)
    yg = _fold_ref(x, wpg, cg).reshape(M, 8 * C // 32, 2, 16)      # groups of 32 rows of the packed weight: 16 values, their 16 gates
    refg = (yg[:, :, 0] * F.gelu(yg[:, :, 1])).reshape(M, 4 * C)
    keepg = (wpg.to(dev), gg.to(dev), cg.to(dev))
    for variant in (0, 51, 62, 72, 73):
        og = torch.full((M, 4 * C), NAN, device=dev, dtype=OP16)
        _run(ops.linear(xd, keepg[0], og, M=M, K=C, N=8 * C, epi=L.EPI_GEGLU, ln_in=stx, ln_g=keepg[1], ln_c=keepg[2], variant=variant))
        _out("linear ln_in", f"GEGLU/v{variant}", r, og, refg, tol=2e-2)
    # fused QKV with the transposed V section
    B, T = 2, 350
    wq = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
    wpq, gq, cq = Wm.fold_layernorm(wq, None, gamma, beta)
    refq = _fold_ref(x, wpq, cq)
    ldt = 384
    keepq = (wpq.to(dev), gq.to(dev), cq.to(dev))
    qk = torch.full((M, 2 * C), NAN, device=dev, dtype=OP16)
    vt = torch.zeros((B, C, ldt), device=dev, dtype=OP16)
    _run(ops.igemm(xd, keepq[0], qk, B=B, H=T, W=1, Cin=C, Ho=T, Wo=1, N=3 * C, ldo=2 * C, out2=vt, trans_from=2 * C, ldt=ldt,
                   ln_in=stx, ln_g=keepq[1], ln_c=keepq[2]))
    _out("linear ln_in", "QKV/qk", r, qk, refq[:, :2 * C], tol=2e-2)
    _out("linear ln_in", "QKV/V^T", r, vt[:, :, :T], refq[:, 2 * C:].reshape(B, T, C).permute(0, 2, 1), tol=2e-2)
    assert (vt[:, :, T:] == 0).all()


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("C,waves", [(320, 12), (320, 8), (320, 4), (640, 8)])
def test_rowgemm_folded_layernorm_consumers(dev, C, waves, r):
    """ops.rowgemm's ln_in forms (QKV with the permuted V^T, plain, GEGLU) fed the float64 (mean, rstd) cast to fp32."""
    from marigold_amd import _lib as L, ops, weights as Wm
    g = torch.Generator().manual_seed(61 + waves + C)
    B, T = 2, 1056
    M = B * T
    x = NL.ladder((M, C), r, -1, OP16, M + C + waves + 2)
    gamma, beta = _affine(C, C + 7)
    xd, stx = x.to(dev, OP16), _stx(x, dev)
    form = f"C{C}/{waves}w"
    nan16 = lambda *sh: torch.full(sh, NAN, device=dev, dtype=OP16)
    # QKV
    wq = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
    wp, lg, lc = Wm.fold_layernorm(wq, None, gamma, beta)
    pk = Wm.pack_rowgemm(wp.float(), lc, lg).to(dev)
    ldt = T + 32
    qk, vt = nan16(M, 2 * C), torch.zeros(B, C, ldt, device=dev, dtype=OP16)
    _run(ops.rowgemm(xd, pk, qk, M=M, K=C, N=3 * C, form=L.RG_QKV, ldo=2 * C, ln_in=stx, vt=vt, tokens=T, ldt=ldt, trans_from=2 * C, waves=waves))
    ref = _fold_ref(x, wp, lc)
    _out("rowgemm ln_in", form + "/QKV/qk", r, qk, ref[:, :2 * C], tol=2e-2)
    want_vt = ops.permute_vt_keys(ref[:, 2 * C:].view(B, T, C).transpose(1, 2).contiguous())
    _out("rowgemm ln_in", form + "/QKV/V^T", r, vt[:, :, :T], want_vt, tol=2e-2)
    assert not vt[:, :, T:].any(), "V^T pad columns were written"
    # plain
    wl, bl = torch.randn(2 * C, C, generator=g) / math.sqrt(C), 0.1 * torch.randn(2 * C, generator=g)
    wp, lg, lc = Wm.fold_layernorm(wl, bl, gamma, beta)
    pk = Wm.pack_rowgemm(wp.float(), lc, lg).to(dev)
    out = nan16(M, 2 * C)
    _run(ops.rowgemm(xd, pk, out, M=M, K=C, N=2 * C, ln_in=stx, waves=waves))
    _out("rowgemm ln_in", form + "/plain", r, out, _fold_ref(x, wp, lc), tol=2e-2)
    # GEGLU
    wg, bg = torch.randn(8 * C, C, generator=g) / math.sqrt(C), 0.1 * torch.randn(8 * C, generator=g)
    order = Wm.rowgemm_geglu_order(8 * C)
    wp, lg, lc = Wm.fold_layernorm(wg[order], bg[order], gamma, beta)
    pk = Wm.pack_rowgemm(wp.float(), lc, lg).to(dev)
    hid = nan16(M, 4 * C)
    _run(ops.rowgemm(xd, pk, hid, M=M, K=C, N=8 * C, form=L.RG_GEGLU, ln_in=stx, waves=waves))
    inv = torch.empty_like(order)
    inv[order] = torch.arange(8 * C)
    u, gt = _fold_ref(x, wp, lc)[:, inv].chunk(2, dim=-1)
    _out("rowgemm ln_in", form + "/GEGLU", r, hid, u * F.gelu(gt), tol=2e-2)


CONV_CONSUMERS = [(2, 24, 32, 320, 320, 0), (2, 24, 32, 320, 320, 6), (1, 48, 32, 256, 128, 8)]


@pytest.mark.parametrize("r", RUNGS)
@pytest.mark.parametrize("case", CONV_CONSUMERS, ids=lambda c: "{}x{}x{}x{}-{}-v{}".format(*c))
def test_conv3x3_fused_groupnorm_consumer(dev, case, r):
    """The GroupNorm fix-up fused into conv3x3's operand staging (``ss``, ``silu``), fed scale / shift from float64: the
    normalised activation is x * scale + shift with both terms ~ r and their sum ~ 1."""
    from marigold_amd import ops, weights as Wm
    B, H, W, Cin, N, variant = case
    g = torch.Generator().manual_seed(H + W + N + variant)
    x = NL.ladder((B, Cin, H, W), r, 1, OP16, NL.gn_seed(B, H, W, Cin), groups=NL.GROUPS)
    gamma, beta = _affine(Cin, Cin + 8)
    _, _, sc64, sh64, _ = NL.gn_reference(x, gamma, beta, 1e-5)
    ss = torch.stack([sc64, sh64], 1).float().contiguous()
    w = _bf(torch.randn(N, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    bias = torch.randn(N, generator=g) * 0.1
    h = x.double() * ss[:, 0].double()[:, :, None, None] + ss[:, 1].double()[:, :, None, None]
    h = (h * torch.sigmoid(h)).to(OP16).double()
    ref = F.conv2d(h, w.double(), bias.double(), padding=1)
    out = torch.full((B, H, W, N), NAN, device=dev, dtype=OP16)
    keep = (_nhwc(x).to(dev, OP16), Wm.pack_conv3x3(w).to(dev, OP16), ss.to(dev), bias.to(dev))
    _run(ops.conv3x3(keep[0], keep[1], out, B=B, H=H, W=W, C0=Cin, N=N, ss=keep[2], silu=True, bias=keep[3], variant=variant))
    _out("conv3x3 ss+silu", "{}x{}x{}x{}->{}/v{}".format(*case), r, out.float().permute(0, 3, 1, 2), ref)
