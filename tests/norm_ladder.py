"""Inputs whose mean dwarfs their spread, for the one-pass normalisation statistics (var = E[x^2] - mean^2 loses digits as
(mean / sigma)^2): a ladder of rungs r = |mean| / sigma, the planted means, the slab form GN_SLAB picks for a shape, and the
float64 references.  Host only - shared by tests/test_norm_ladder_host.py and tests/test_gpu_norm_conditioning.py.

Every element is ``randn + m`` (LayerNorm: each row's draws scaled to the sample variance 1) with ``m`` constant over one statistics domain - an (image, group) for GroupNorm, a row for
LayerNorm - ``|m| = r * U(0.75, 1.25)``, the sign drawn per domain; GroupNorm adds a per-channel jitter of ``0.5 * randn`` (what
tests/test_gpu_kernels.py::test_groupnorm_one_launch has).  r = 32 is the last power of two at which bf16 stores spread-1 data on a
grid of sigma / 4; r = 64 is one step past it (sigma / 2 in bf16, sigma / 16 in fp16)."""
import torch

RUNGS = (0, 4, 16, 32, 64)
GROUPS = 32
STATS_BOUND = 2e-4            # the suite's statistics bound (tests/test_gpu_kernels.py: ln_out, gn_slab scale / shift)


def stats_bound(r):
    """2e-4 up to the anchor rung r = 32, then the growth of var's condition number 1 + r^2 from (sum, sum of squares): one
    doubling past the anchor may cost a factor four and no more."""
    return STATS_BOUND * max(1.0, (r / 32.0) ** 2)


def planted_means(n, r, seed):
    """[n] float64: |m| = r * U(0.75, 1.25), sign drawn per domain."""
    g = torch.Generator().manual_seed(100003 * seed + 17 * int(r) + 1)
    mag = r * (0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return mag * sign


def _round(x, dtype):
    return x.to(dtype).float()


def ladder(shape, r, axis, dtype, seed, groups=None, const=None):
    """fp32 tensor of ``shape`` holding values representable in ``dtype``.  ``groups`` None: LayerNorm rows - statistics over
    ``axis``, one planted mean per index of the other axes.  ``groups`` = G: GroupNorm on [B, C, ...] with ``axis`` = 1 - one mean
    per (image, group), plus the per-channel jitter.  ``const`` = (image, group): that one domain holds its planted mean exactly
    (spread 0; rounded to ``dtype``)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    nd = len(shape)
    axis %= nd
    if groups is None:
        assert const is None
        rest = [s for i, s in enumerate(shape) if i != axis]
        n = 1
        for s in rest:
            n *= s
        m = planted_means(n, r, seed).reshape([1 if i == axis else s for i, s in enumerate(shape)])
        # a row of n draws has the sample variance 1 +- sqrt(2 / n) (n = 320: 0.75 .. 1.25 over 700 rows), so the rows' noise is
        # scaled to the sample variance 1 - every domain then stores a variance in [0.9, 1.6], as the groups do by their size
        x = x / x.var(axis, unbiased=False, keepdim=True).sqrt()
        return _round(x + m, dtype)
    assert axis == 1 and shape[1] % groups == 0
    B, C = shape[0], shape[1]
    cpg = C // groups
    bc = [1] * nd
    bc[1] = C
    x = x + 0.5 * torch.randn(C, generator=g, dtype=torch.float64).reshape(bc)
    m = planted_means(B * groups, r, seed).reshape(B, groups)
    mc = m.repeat_interleave(cpg, 1).reshape([B, C] + [1] * (nd - 2))
    x = x + mc
    if const is not None:
        b, gi = const
        x[b, gi * cpg:(gi + 1) * cpg] = m[b, gi]
    return _round(x, dtype)


# A 10-channel group's share of the jitter has the sample variance 0.25 * chi2_9 / 10: in a few per cent of tensors one group's
# stored variance leaves [0.9, 1.6].  The seeds the tests use pass over such draws (tests/test_norm_ladder_host.py checks).
_SEED_BUMP = {(1, 13, 9, 320): 2, (2, 13, 9, 320): 4}


def gn_seed(B, H, W, C):
    return C + H + 1000 * _SEED_BUMP.get((B, H, W, C), 0)


def group_means(B, r, seed, groups=GROUPS):
    """The (image, group) means ``ladder`` plants for a GroupNorm tensor of B images with this seed."""
    return planted_means(B * groups, r, seed).reshape(B, groups)


# ---- float64 references, from operands as stored ---------------------------------------------------------------------------
def gn_reference(x, gamma, beta, eps, groups=GROUPS):
    """x [B, C, ...] (any float dtype) -> float64 (mean [B, G], var [B, G], scale [B, C], shift [B, C], normalised x)."""
    xd = x.double()
    B, C = xd.shape[:2]
    cpg = C // groups
    xg = xd.reshape(B, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    scale = rstd.repeat_interleave(cpg, 1) * gamma.double()
    shift = beta.double() - mean.repeat_interleave(cpg, 1) * scale
    bc = [B, C] + [1] * (xd.dim() - 2)
    return mean, var, scale, shift, xd * scale.reshape(bc) + shift.reshape(bc)


def ln_reference(x, eps=1e-5):
    """rows x [M, C] -> float64 (mean [M], var [M], rstd [M])."""
    xd = x.double()
    mean, var = xd.mean(-1), xd.var(-1, unbiased=False)
    return mean, var, (var + eps).rsqrt()


def gn_map_points(mean, var, cpg):
    """[B, C, 3] float64: x = mean_g + {-2, 0, 2} sigma_g of every channel - where scale * x + shift is judged (at the data: a
    shift inconsistent with its scale shows there, a bound relative to max|shift| ~ r would hide it)."""
    mu, sd = mean.repeat_interleave(cpg, 1), var.sqrt().repeat_interleave(cpg, 1)
    return torch.stack([mu - 2 * sd, mu, mu + 2 * sd], dim=-1)


# ---- which kernel form MG_OP_GN_SLAB picks (csrc/norm.hip, case MG_OP_GN_SLAB) ---------------------------------------------
def slab_form(HW, C, groups=GROUPS):
    """-> (threads, rows kept in registers per thread, need) of the launch csrc/norm.hip makes for this shape with an output."""
    cpg = C // groups
    cw = cpg if cpg % 4 == 0 else (2 * cpg if cpg % 2 == 0 else 4 * cpg)
    nt = 1024 if HW * cw * 2 >= 48 * 1024 else 256
    nty = nt // (cw // 4)
    need = -(-HW // nty)
    assert need <= 48
    steps = (12, 24, 48) if nt == 1024 else (8, 24, 48)
    return nt, next(s for s in steps if need <= s), need


# One shape per register form of gn_slab_kernel: (B, H, W, C0, C1, silu, eps) -> <threads, rows>.  The first, fourth and sixth
# are shapes of test_groupnorm_one_launch; the two 24-row forms and <256, 48> need shapes of their own.
SLAB_SHAPES = [
    ((3, 12, 12, 1280, 0, False, 1e-6), (256, 8)),        # 11 KB slab, need 6
    ((1, 24, 24, 320, 0, True, 1e-5), (256, 24)),         # 46 KB slab, need 12
    ((1, 17, 36, 1280, 0, True, 1e-6), (256, 48)),        # 48960-byte slab (just under the 48 KB switch), need 25
    ((2, 24, 24, 1280, 1280, True, 1e-5), (1024, 12)),    # skip concat, 92 KB slab, need 12
    ((1, 56, 56, 640, 0, False, 1e-5), (1024, 24)),       # 125 KB slab, need 16
    ((1, 96, 96, 320, 0, False, 1e-6), (1024, 48)),       # level 0: 369 KB slab, need 46 - the longest fp32 chains
]

# gn_stats -> gn_finalize -> gn_apply: (B, H, W, C0, C1)
STATS_SHAPES = [
    (1, 96, 96, 320, 0),      # longest fp32 chains, 10-channel groups
    (2, 24, 24, 2560, 0),
    (1, 13, 9, 320, 0),       # ragged tail batch
    (1, 48, 48, 640, 320),    # two sources, 30-channel groups: group 21 (channels 630 .. 659) straddles the sources
    (1, 13, 9, 640, 320),
]
