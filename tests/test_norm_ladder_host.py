"""The ladder of tests/norm_ladder.py is what it claims, and the references it is judged by are not what is being tested: for
every rung and both 16-bit operand types the stored variance of each statistics domain, the achieved |mean| / sigma, and torch's
fp32 group_norm / layer_norm against float64 (1e-5 of max|ref|: 1/20 of the tightest bound the GPU tests assert).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ladder as NL

DTYPES = [torch.bfloat16, torch.float16]
GN_SHAPES = sorted({s[:5] for s, _ in NL.SLAB_SHAPES} | set(NL.STATS_SHAPES))
LN_SHAPES = [(700, 320), (700, 1280), (2112 + 37, 640)]


def _seed(*dims):
    return sum(dims)


def _check_ratio(mean, var, r, what):
    ratio = (mean.abs() / var.sqrt())
    lo, hi = float(ratio.min()), float(ratio.max())
    print(f"[ladder] {what} r={r}: var [{float(var.min()):.3f}, {float(var.max()):.3f}]  |mean|/sigma [{lo:.3f}, {hi:.3f}]")
    assert 0.9 <= float(var.min()) and float(var.max()) <= 1.6, (what, r, float(var.min()), float(var.max()))
    if r == 0:
        # nothing is planted: what is left is the sample mean of the data itself (GroupNorm: of the group's cpg jitters,
        # 0.5 / sqrt(cpg) * N(0, 1)), well under one sigma
        assert hi <= 1.0, (what, r, hi)
    else:
        assert 0.5 * r <= lo and hi <= 1.4 * r, (what, r, lo, hi)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("r", NL.RUNGS)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_ladder(shape, r, dtype):
    B, H, W, C0, C1 = shape
    C = C0 + C1
    x = NL.ladder((B, C, H, W), r, 1, dtype, NL.gn_seed(B, H, W, C), groups=NL.GROUPS)
    assert torch.equal(x, x.to(dtype).float()), "values must be representable in the operand type"
    g = torch.Generator().manual_seed(C)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    mean, var, _, _, ref = NL.gn_reference(x, gamma, beta, 1e-5)
    _check_ratio(mean, var, r, f"groupnorm {shape} {dtype}")
    got = F.group_norm(x, NL.GROUPS, gamma, beta, 1e-5).double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"[ladder] groupnorm {shape} {dtype} r={r}: torch fp32 vs float64 {err:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("r", [0, 32])
def test_groupnorm_ladder_constant_group(r, dtype):
    """The edge: one group of one image constant at its planted mean - variance exactly 0 there, the float64 output ``beta``."""
    B, C, H, W = 2, 320, 13, 9
    x = NL.ladder((B, C, H, W), r, 1, dtype, NL.gn_seed(B, H, W, C), groups=NL.GROUPS, const=(1, 5))
    g = torch.Generator().manual_seed(C)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    mean, var, _, _, ref = NL.gn_reference(x, gamma, beta, 1e-5)
    assert float(var[1, 5]) == 0.0 and float(var.flatten()[torch.arange(B * 32) != 37].min()) >= 0.9
    assert torch.equal(ref[1, 50:60], beta[50:60].double()[:, None, None].expand(10, H, W))
    if r:
        assert abs(float(mean[1, 5])) >= 0.74 * r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("r", NL.RUNGS)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layernorm_ladder(shape, r, dtype):
    M, C = shape
    x = NL.ladder((M, C), r, -1, dtype, _seed(M, C))
    assert torch.equal(x, x.to(dtype).float())
    mean, var, rstd = NL.ln_reference(x)
    _check_ratio(mean, var, r, f"layernorm {shape} {dtype}")
    g = torch.Generator().manual_seed(C)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    ref = (x.double() - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    got = F.layer_norm(x, (C,), gamma, beta, 1e-5).double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"[ladder] layernorm {shape} {dtype} r={r}: torch fp32 vs float64 {err:.2e}")
    assert err <= 1e-5


def test_slab_shapes_reach_every_register_form():
    """One shape per register form of gn_slab_kernel: <256, 8 | 24 | 48> and <1024, 12 | 24 | 48>."""
    forms = []
    for (B, H, W, C0, C1, _, _), want in NL.SLAB_SHAPES:
        nt, rows, need = NL.slab_form(H * W, C0 + C1)
        assert (nt, rows) == want, ((B, H, W, C0, C1), nt, rows, need)
        forms.append(want)
    assert sorted(forms) == [(256, 8), (256, 24), (256, 48), (1024, 12), (1024, 24), (1024, 48)]
