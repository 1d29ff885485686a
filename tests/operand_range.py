"""Helpers of tests/test_gpu_operand_range.py and tests/test_operand_range_host.py (CPU only, float64): what a 16-bit store of an
exact value must give in each library build, the classes an output element falls into near the fp16 limit, the seeded input
ladder whose outputs cross that limit, and the arithmetic of the fixed-reference attention kernels' fp16 window.

DESIGN.md "Operand types": the bf16 build rounds (1e5 is a number, an overflow is inf); the fp16 build converts and then clamps with
IEEE minimum / maximum, so every 16-bit store saturates at +-65504 and keeps NaN (csrc/common.h::cvt_pk_bf16_f32)."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0
F16_OVER = 65520.0        # the first magnitude that fp16 rounds to inf: what the clamp brings back to 65504
F16_BELOW = 65472.0       # fp16 neighbour of 65504
BAND = 2.0 ** -9          # half-width of the guard band around the limit (fp32 accumulation over K <= 11520 terms ~ K * 2^-24)
SAT_LO = F16_MAX * (1.0 - BAND)
SAT_HI = F16_OVER * (1.0 + BAND)
LOG2E = 1.4426950408889634

# mirrors of the kernels' constants (csrc/flash4w.hip, csrc/attention.hip, csrc/flash512.hip), per build (False: bf16, True: fp16)
F4_REF_BIAS = {False: 0.0, True: 6.0}
F4_REDO_THR = {False: 2.0 ** 100, True: 2.0 ** 15}
FA5_THR = {False: 60.0, True: 15.0}


def op16(f16):
    return torch.float16 if f16 else torch.bfloat16


def _round_even(x, mant_bits, emin):
    """Finite float64 -> nearest value with ``mant_bits`` fraction bits and minimum exponent ``emin`` (subnormals below), ties to even."""
    _, e = np.frexp(x)                       # |x| = m * 2^e, 0.5 <= m < 1
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - mant_bits)
    return np.rint(x / q) * q                # x / q is exact (q is a power of two); rint rounds half to even


def store16(ref64, f16):
    """What a 16-bit store of the exact value must hold, as float64.  bf16: round to nearest even, overflow gives inf, NaN stays
    NaN.  fp16: NaN stays NaN, |x| >= 65520 (+-inf included) gives +-65504, otherwise round to nearest even."""
    x = torch.as_tensor(ref64, dtype=torch.float64).detach().cpu().numpy()
    nan = np.isnan(x)
    if f16:
        big = ~nan & (np.abs(x) >= F16_OVER)
        r = _round_even(np.where(big | nan, 0.0, x), 10, -14)
        r = np.where(big, np.copysign(F16_MAX, x), r)
    else:
        fin = np.isfinite(x)
        r = _round_even(np.where(fin, x, 0.0), 7, -126)
        r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, r), r)
        r = np.where(np.isinf(x), x, r)
    r = np.where(nan, np.nan, r)
    return torch.from_numpy(np.ascontiguousarray(r))


def classify(ref64, f16):
    """(saturating, guard, regular, nonfinite) masks of a float64 reference.  Saturating and guard exist in the fp16 build only."""
    ref = torch.as_tensor(ref64, dtype=torch.float64)
    fin = torch.isfinite(ref)
    a = ref.abs()
    if f16:
        sat = fin & (a >= SAT_HI)
        guard = fin & (a > SAT_LO) & ~sat
    else:
        sat = torch.zeros_like(fin)
        guard = torch.zeros_like(fin)
    return sat, guard, fin & ~sat & ~guard, ~fin


def case_conditions(ref64, packs_along_rows=False):
    """The input conditions of a Part A case, from its float64 reference [rows][columns] alone (fp16 limits, whichever build
    the operands were rounded for).  ``packs_along_rows``: the reference is laid out with the ladder over its rows where the
    kernel's eight-wide packs run down a column (the column-ladder cases, checked transposed)."""
    ref = torch.as_tensor(ref64, dtype=torch.float64)
    sat, guard, reg, nonfin = classify(ref, True)
    assert not nonfin.any()
    if packs_along_rows:
        assert ref.dim() == 2 and ref.shape[0] % 8 == 0
        packs_sat = sat.reshape(-1, 8, ref.shape[1]).any(1)
        packs_reg = reg.reshape(-1, 8, ref.shape[1]).any(1)
    else:
        assert ref.dim() == 2 and ref.shape[1] % 8 == 0
        packs_sat = sat.reshape(ref.shape[0], -1, 8).any(-1)
        packs_reg = reg.reshape(ref.shape[0], -1, 8).any(-1)
    return dict(pos=int((sat & (ref > 0)).sum()), neg=int((sat & (ref < 0)).sum()), guard=int(guard.sum()), regular=int(reg.sum()),
                mixed_packs=int((packs_sat & packs_reg).sum()), regular_rows=int(reg.all(-1).sum()), rows=ref.shape[0])


def assert_case_conditions(name, ref64, packs_along_rows=False):
    c = case_conditions(ref64, packs_along_rows)
    assert c["pos"] >= 100 and c["neg"] >= 100, (name, c)
    assert c["mixed_packs"] >= 100, (name, c)
    assert 4 * c["regular_rows"] >= c["rows"], (name, c)
    assert c["guard"] <= 0.02 * (c["pos"] + c["neg"]), (name, c)
    return c


def check_store(name, got, ref64, f16, tol=1.5e-2):
    """A kernel's 16-bit output [rows][columns] against ``store16`` of its float64 reference, class by class (module docstring of
    tests/test_gpu_operand_range.py).  Returns the counts and the worst regular error for the measured tables."""
    got = got.detach().cpu()
    assert got.dtype == op16(f16), (name, got.dtype)
    got = got.double()
    ref = torch.as_tensor(ref64, dtype=torch.float64)
    assert got.shape == ref.shape and ref.dim() == 2, (name, tuple(got.shape), tuple(ref.shape))
    sat, guard, reg, nonfin = classify(ref, f16)
    want = store16(ref, f16)
    sign = torch.sign(ref)
    if f16:
        assert not torch.isinf(got).any(), f"{name}: {int(torch.isinf(got).sum())} fp16 outputs are inf"
    # non-finite reference: NaN stays NaN, +-inf is +-65504 (fp16) or +-inf (bf16); the masks must be equal
    want_nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), want_nan), (f"{name}: NaN mask differs: {int((want_nan & ~torch.isnan(got)).sum())} missing, "
                                                     f"{int((torch.isnan(got) & ~want_nan).sum())} extra")
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], want[inf]), f"{name}: {int((got[inf] != want[inf]).sum())} of {int(inf.sum())} +-inf references not stored as such"
    if not f16:
        assert torch.equal(torch.isinf(got), inf | (torch.isinf(want) & ~want_nan)), f"{name}: inf mask differs"
    exact = int((got[sat] == sign[sat] * F16_MAX).sum())
    assert exact == int(sat.sum()), f"{name}: {int(sat.sum()) - exact} of {int(sat.sum())} saturating outputs are not +-65504"
    # guard band: a value that the store gives for some |ref| (1 +- 2^-9) - 65504 or 65472 at the limit itself
    gs, ga = got[guard] * sign[guard], ref[guard].abs()
    lo, hi = store16(ga * (1.0 - BAND), f16), store16(ga * (1.0 + BAND), f16)
    assert bool(((gs >= lo) & (gs <= hi)).all()), f"{name}: guard-band outputs outside the band: {gs[(gs < lo) | (gs > hi)][:8].tolist()}"
    assert torch.isfinite(got[reg]).all(), f"{name}: non-finite regular outputs"
    scale = torch.where(reg, ref.abs(), torch.zeros_like(ref)).amax(dim=1, keepdim=True).clamp_min(1e-6)
    err = torch.where(reg, (got - ref).abs(), torch.zeros_like(ref)) / scale
    worst = float(err.max())
    st = dict(sat=int(sat.sum()), guard=int(guard.sum()), regular=int(reg.sum()), nonfinite=int(nonfin.sum()), exact=exact, worst=worst)
    print(f"[range] {name} {'fp16' if f16 else 'bf16'}: saturating {st['sat']} (exactly +-65504: {exact}) guard {st['guard']} regular {st['regular']} "
          f"non-finite {st['nonfinite']} worst regular |err| / row scale {worst:.3e}")
    assert worst <= tol, f"{name}: regular error {worst:.4e} of the row scale > {tol} (row {int(err.amax(1).argmax())})"
    return st


# --------------------------------------------------------------------------- the ladder

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ladder_rows(M, K, f16, seed, top=13.0):
    """[M][K] activation, row r with gain 2^(top r / M), rounded to the build's operand type (|x| stays below 2^15)."""
    g = _gen(seed)
    gain = torch.exp2(top * torch.arange(M, dtype=torch.float64) / M)
    x = (torch.randn(M, K, generator=g, dtype=torch.float64) * gain[:, None]).clamp(-32000.0, 32000.0)
    return x.to(op16(f16))


def ladder_weights(N, K, f16, seed, amp=8.0):
    return (torch.randn(N, K, generator=_gen(seed), dtype=torch.float64) * (amp / math.sqrt(K))).to(op16(f16))


def planted_residual(M, N, f16, seed, top=13.0):
    """A residual at each row's own scale with a mean of its own per row, and +-60000 planted in four rows whose products are
    regular by themselves (gain about 2^10: a product of 5600 and more makes the ADD cross the limit)."""
    g = _gen(seed)
    gain = torch.exp2(top * torch.arange(M, dtype=torch.float64) / M)
    res = (torch.randn(M, N, generator=g, dtype=torch.float64) * 2.0 + 3.0 * torch.randn(M, 1, generator=g, dtype=torch.float64)) * gain[:, None]
    res = res.clamp(-50000.0, 50000.0)
    col = torch.arange(N)
    for r in [int(M * f) for f in (0.74, 0.755, 0.77, 0.785)]:
        res[r, col % 16 < 4] = 60000.0
        res[r, (col % 16 >= 8) & (col % 16 < 12)] = -60000.0
    return res.to(op16(f16))


LINEAR_FORMS = ("plain", "bias", "rowvec", "residual")
CONV_SHAPE = (2, 12, 20, 320, 320)        # B, H, W, Cin, Cout
CONV_AMP = 12.0
CONV_FUSED_AMP = 16.0                    # SiLU removes the negative half of the operand: larger weights bring the counts back
SPLITK_SHAPE = (1, 12, 12, 1280, 128)     # CONV_CASES' g2_auto_splitk: 144 rows only, so more of them have to saturate
SPLITK_AMP = 32.0
FLASH64_G = (10.0, 14.0, 18.0, 20.0, 22.0, 26.0)
FLASH512_G = (8.0, 12.0, 14.9, 15.5, 17.0)


@functools.lru_cache(maxsize=None)
def linear_case(form, f16, M=312, K=320, N=320):
    """MG_OP_IGEMM as a Linear layer on the ladder: out = x w^T [+ bias] [+ row vector] [+ residual]."""
    x, w = ladder_rows(M, K, f16, 1), ladder_weights(N, K, f16, 2)
    c = types.SimpleNamespace(M=M, K=K, N=N, x=x, w=w, bias=None, rowvec=None, res=None)
    ref = x.double() @ w.double().t()
    g = _gen(3)
    if form != "plain":
        c.bias = torch.randn(N, generator=g) * 50.0
        ref = ref + c.bias.double()
    if form == "rowvec":
        c.rowvec = torch.randn(1, N, generator=g) * 50.0
        ref = ref + c.rowvec.double()
    if form == "residual":
        c.res = planted_residual(M, N, f16, 4)
        ref = ref + c.res.double()
    c.ref = ref
    return c


def conv_ladder(B, H, W, C, f16, seed, top=13.0):
    """[B][C][H][W] activation whose pixel rows (image, y, x in raster order) carry the ladder's gains."""
    x = ladder_rows(B * H * W, C, f16, seed, top)
    return x.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def conv_case(f16, B, H, W, Cin, Cout, fused=False, amp=8.0, seed=10):
    """3 x 3 / pad 1 convolution on the ladder (MG_OP_IGEMM with nine taps, MG_OP_CONV3X3): + bias + residual; ``fused``: the
    GroupNorm scale / shift + SiLU on the input, stored as an operand (store16) before the convolution reads it."""
    x = conv_ladder(B, H, W, Cin, f16, seed)
    w = ladder_weights(Cout, 9 * Cin, f16, seed + 1, amp).reshape(Cout, Cin, 3, 3)
    g = _gen(seed + 2)
    bias = torch.randn(Cout, generator=g) * 50.0
    c = types.SimpleNamespace(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x=x, w=w, bias=bias, ss=None)
    h = x.double()
    if fused:
        c.ss = torch.stack([1.0 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)], dim=1).contiguous()
        h = h * c.ss[:, 0].double()[:, :, None, None] + c.ss[:, 1].double()[:, :, None, None]
        h = store16(h * torch.sigmoid(h), f16)
    ref = F.conv2d(h, w.double(), bias.double(), padding=1)
    c.ref = ref.permute(0, 2, 3, 1).reshape(B * H * W, Cout).contiguous()     # rows = pixels, as the kernels store them
    return c


@functools.lru_cache(maxsize=None)
def rowgemm_case(f16, K, M=416, N=320):
    """MG_OP_ROWGEMM form 0: out = x w^T + bias + residual (planted), and the plain bias form."""
    x, w = ladder_rows(M, K, f16, 21 + K), ladder_weights(N, K, f16, 22 + K)
    bias = torch.randn(N, generator=_gen(23)) * 50.0
    res = planted_residual(M, N, f16, 24)
    base = x.double() @ w.double().t() + bias.double()
    return types.SimpleNamespace(M=M, K=K, N=N, x=x, w=w, bias=bias, res=res, ref_bias=base, ref=base + res.double())


@functools.lru_cache(maxsize=None)
def gn_apply_case(f16, B=2, HW=240, C=320):
    """MG_OP_GN_APPLY: x * scale + shift (no SiLU) with the ladder over the pixel rows and
    scales around 8, shifts around 50: the product crosses the limit in the upper rows."""
    g = _gen(31)
    x = ladder_rows(B * HW, C, f16, 30).reshape(B, HW, C)
    sc = 8.0 * (1.0 + 0.3 * torch.randn(B, C, generator=g))
    sh = 50.0 * torch.randn(B, C, generator=g)
    ss = torch.stack([sc, sh], dim=1).float().contiguous()
    ref = x.double() * ss[:, 0].double()[:, None, :] + ss[:, 1].double()[:, None, :]
    return types.SimpleNamespace(B=B, HW=HW, C=C, x=x, ss=ss, ref=ref.reshape(B * HW, C))


@functools.lru_cache(maxsize=None)
def geglu_case(f16, M=312, K=320, Nh=320):
    """MG_OP_IGEMM's GEGLU epilogue: out = u * gelu(g), (u | g) = x w^T + b.  The ladder tops out at 2^6.5, so that neither factor
    comes near the limit (a few thousand) while their product crosses it."""
    x, w = ladder_rows(M, K, f16, 61, top=6.5), ladder_weights(2 * Nh, K, f16, 62)
    b = torch.randn(2 * Nh, generator=_gen(63)) * 5.0
    u, g = (x.double() @ w.double().t() + b.double()).chunk(2, dim=-1)
    gl = F.gelu(g)
    return types.SimpleNamespace(M=M, K=K, Nh=Nh, x=x, w=w, b=b, ref=u * gl, factor_max=max(float(u.abs().max()), float(gl.abs().max())))


@functools.lru_cache(maxsize=None)
def qkv_case(f16, T, B=2, K=320, C=128):
    """MG_OP_IGEMM with the transposed section: columns < 2C to [M][2C...], columns >= 2C to V^T [B][C][ldt].  T % 8 == 0: the
    16-byte store of eight tokens of one channel; otherwise the scalar store."""
    M = B * T
    x, w = ladder_rows(M, K, f16, 71), ladder_weights(3 * C, K, f16, 72)
    b = torch.randn(3 * C, generator=_gen(73)) * 50.0
    return types.SimpleNamespace(B=B, T=T, M=M, K=K, C=C, x=x, w=w, b=b, ref=x.double() @ w.double().t() + b.double())


@functools.lru_cache(maxsize=None)
def subpix_case(f16, B, H, W, Cin, Cout, amp=12.0, seed=80):
    """MG_OP_CONV3X3's sub-pixel form: nearest 2x + conv3x3 as four 2 x 2 convolutions with pre-summed taps.  The operands as
    stored are the PACKED weights (summed in float64 here, then rounded once): the reference convolves with those."""
    from marigold_amd import weights as Wm
    x = conv_ladder(B, H, W, Cin, f16, seed)
    w = torch.randn(Cout, Cin, 3, 3, generator=_gen(seed + 1), dtype=torch.float64) * (amp / math.sqrt(9 * Cin))
    ws = Wm.pack_conv3x3_subpix(w).to(op16(f16))                       # [4][Cout][4 Cin]
    bias = torch.randn(Cout, generator=_gen(seed + 2)) * 50.0
    xp = F.pad(x.double().permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))     # [B][H + 2][W + 2][Cin]
    ref = torch.empty(B, 2 * H, 2 * W, Cout, dtype=torch.float64)
    for z in range(4):
        a_, b_ = z // 2, z % 2
        rows = torch.cat([xp[:, a_ + ty:a_ + ty + H, b_ + tx:b_ + tx + W] for ty in range(2) for tx in range(2)], dim=-1)
        ref[:, a_::2, b_::2] = rows @ ws[z].double().t() + bias.double()
    return types.SimpleNamespace(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x=x, ws=ws, bias=bias, ref=ref.reshape(B * 4 * H * W, Cout))


@functools.lru_cache(maxsize=None)
def im2col_case(B=2, H=12, W=20, C0=4, C1=4, Kp=128):
    """MG_OP_IM2COL_SMALL: fp32 latents around 4e4 with 1e5, -1e5 and both infinities planted -> the 3 x 3 patches as operand rows
    [B H W][Kp], k = tap * (C0 + C1) + c, zero outside the image and past 9 (C0 + C1).  The float64 rows before the store."""
    g = _gen(90)
    a = torch.randn(B, C0, H, W, generator=g) * 4e4
    b = torch.randn(B, C1, H, W, generator=g) * 4e4
    a[0, 1, 3, 4], a[1, 0, 0, 0], b[0, 2, 5, 19], b[1, 3, 11, 7] = 1e5, -1e5, float("inf"), float("-inf")
    xp = F.pad(torch.cat([a, b], dim=1).double().permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
    rows = torch.cat([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=-1).reshape(B * H * W, 9 * (C0 + C1))
    return types.SimpleNamespace(B=B, H=H, W=W, C0=C0, C1=C1, Kp=Kp, a=a, b=b, rows=F.pad(rows, (0, Kp - rows.shape[1])))


@functools.lru_cache(maxsize=None)
def head_case(f16, silu, B=2, H=12, W=20, C=64, Cout=3):
    """MG_OP_CONV3X3_HEAD: the normalised patch x * scale + shift [+ SiLU] is packed to operands on its way into LDS - a 16-bit
    store of values that cross the limit in the ladder's upper pixels (``h``: before that store) - and convolved to fp32 channels."""
    g = _gen(95)
    x = conv_ladder(B, H, W, C, f16, 94)
    w = (torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(9 * C)).to(op16(f16))
    bias = torch.randn(Cout, generator=g) * 0.1
    ss = torch.stack([8.0 * (1.0 + 0.3 * torch.randn(B, C, generator=g)), 50.0 * torch.randn(B, C, generator=g)], dim=1).float().contiguous()
    h = x.double() * ss[:, 0].double()[:, :, None, None] + ss[:, 1].double()[:, :, None, None]
    if silu:
        h = h * torch.sigmoid(h)
    ref = F.conv2d(store16(h, f16), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1).contiguous()     # [B][H][W][Cout]
    return types.SimpleNamespace(B=B, H=H, W=W, C=C, Cout=Cout, x=x, w=w, bias=bias, ss=ss, ref=ref,
                                 h=h.permute(0, 2, 3, 1).reshape(B * H * W, C))


def conv_operand_rows(x):
    """[B][C][H][W] -> the implicit GEMM's operand rows [B H W][9 C], k = tap * C + c (zero outside the image), float64."""
    B, C, H, W = x.shape
    xp = F.pad(x.double().permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
    return torch.cat([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=-1).reshape(B * H * W, 9 * C)


def splitk_partials(c, splits):
    """The float64 partial sums of a convolution case over ``splits`` equal ranges of K: [splits][rows][Cout] (no bias)."""
    rows = conv_operand_rows(c.x)
    w = c.w.double().permute(0, 2, 3, 1).reshape(c.Cout, -1)
    K = rows.shape[1]
    assert K % splits == 0
    step = K // splits
    return torch.stack([rows[:, i * step:(i + 1) * step] @ w[:, i * step:(i + 1) * step].t() for i in range(splits)])


def row_stats(x64, eps=1e-5):
    """(mean, rstd) of every row as the fp32 table a producer hands on: float32 [M][2]."""
    x64 = x64.double()
    return torch.stack([x64.mean(-1), 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + eps)], dim=-1).float().contiguous()


def folded_ln(x16, st, wp, g, c):
    """The folded LayerNorm's own formula in float64 on the operands as stored: rstd (x Wp^T - mean g) + c."""
    st = st.double()
    return st[:, 1:2] * (x16.double() @ wp.double().t() - st[:, 0:1] * g.double()[None, :]) + c.double()[None, :]


def _o1_rows(M, K, f16, seed):
    g = _gen(seed)
    return (torch.randn(M, K, generator=g) * 1.3 + 0.4 * torch.randn(M, 1, generator=g)).to(op16(f16))


@functools.lru_cache(maxsize=None)
def ln_fold_case(f16, geglu, M=416, K=320, Nh=320):
    """The folded LayerNorm (ln_in) in front of a 16-bit epilogue.  The normalisation takes every row to O(1), so the ladder is
    over the output COLUMNS: weight row n has gain 2^(top n / Nh) (the GEGLU pair of a column shares it; top = 13, or 6.5 for the
    product).  ``ref`` is [M][Nh]; it is checked transposed, each column against its own scale."""
    g = _gen(100 + K)
    x = _o1_rows(M, K, f16, 101 + K)
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    gain = torch.exp2((6.5 if geglu else 13.0) * torch.arange(Nh, dtype=torch.float64) / Nh)
    N = 2 * Nh if geglu else Nh
    w = (torch.randn(N, K, generator=g, dtype=torch.float64) * (8.0 / math.sqrt(K)) * gain.repeat(N // Nh)[:, None]).float()
    b = (torch.randn(N, generator=g, dtype=torch.float64) * 5.0 * gain.repeat(N // Nh)).float()
    st = row_stats(x)
    return types.SimpleNamespace(M=M, K=K, Nh=Nh, N=N, x=x, w=w, b=b, gamma=gamma, beta=beta, st=st, geglu=geglu, dtype=op16(f16),
                                 ref_of=lambda wp, gv, cv: _ln_fold_ref(x, st, wp, gv, cv, geglu))


def _ln_fold_ref(x, st, wp, gv, cv, geglu):
    y = folded_ln(x, st, wp, gv, cv)
    if not geglu:
        return y
    u, g = y.chunk(2, dim=-1)
    return u * F.gelu(g)


def ln_fold_operands(c, order=None):
    """(Wp, g, c) of weights.fold_layernorm for the case's rows in ``order`` (None: u rows then gate rows), and the float64
    reference [M][Nh] of the operands as stored - whatever the order, column j of the output is pair j."""
    from marigold_amd import weights as Wm
    wp, gv, cv = Wm.fold_layernorm(c.w, c.b, c.gamma, c.beta, dtype=c.dtype)
    ref = c.ref_of(wp, gv, cv)
    if order is not None:
        wp, gv, cv = wp[order].contiguous(), gv[order].contiguous(), cv[order].contiguous()
    return wp, gv, cv, ref


@functools.lru_cache(maxsize=None)
def xattn_case(f16, M, C=320, heads=5):
    """The collapsed two-token cross-attention, in place on the residual stream (MG_EPI_XATTN2, MG_OP_ROWGEMM's form 3 and the
    GEGLU form's prologue): out = P VO^T + bias + x with P the pair softmax of the folded LayerNorm's scores, rounded to an operand.
    x carries the row ladder and a mean of +-8 gains per row (the residual is what crosses the limit), VO^T entries are +-12000 for the first five heads and zero for the others (the attention term alone stays regular)."""
    from marigold_amd import weights as Wm
    g = _gen(110)
    gain = torch.exp2(13.0 * torch.arange(M, dtype=torch.float64) / M)
    sgn = torch.where(torch.rand(M, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    x = (ladder_rows(M, C, f16, 111).double() + (8.0 * sgn * gain)[:, None]).clamp(-64000.0, 64000.0).to(op16(f16))   # rows with means of their own
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    wqk = torch.zeros(64, C)
    wqk[:2 * heads] = torch.randn(2 * heads, C, generator=g) * (3.0 / math.sqrt(C))
    vot = torch.zeros(C, 64)
    vot[:, :10] = torch.where(torch.rand(C, 10, generator=g) < 0.5, -12000.0, 12000.0)   # five heads' values, bounded: |P VO^T| <= 60000
    vot = vot.to(op16(f16))
    bias = torch.randn(C, generator=g) * 50.0
    st = row_stats(x)
    wp, gv, cv = Wm.fold_layernorm(wqk, None, gamma, beta, dtype=op16(f16))
    scale = 0.125
    sc = folded_ln(x, st, wp, gv, cv)[:, :2 * heads].reshape(M, heads, 2) * scale
    P = torch.zeros(M, 64, dtype=torch.float64)
    P[:, :2 * heads] = store16(torch.softmax(sc, dim=-1).reshape(M, 2 * heads), f16)
    ref = P @ vot.double().t() + bias.double() + x.double()
    return types.SimpleNamespace(M=M, C=C, heads=heads, x=x, wp=wp, gv=gv, cv=cv, vot=vot, bias=bias, st=st, scale=scale, ref=ref)


@functools.lru_cache(maxsize=None)
def xattn_geglu_case(f16, M=416, C=320):
    """MG_OP_ROWGEMM's GEGLU form with the cross-attention prologue: the updated rows are stored (P_XOUT: ``store16`` of the
    cross-attention case's reference) and fed on as stored, normalised with the statistics of the fp32 rows BEFORE that store,
    into hidden = u * gelu(g) with O(1) weights."""
    from marigold_amd import weights as Wm
    xc = xattn_case(f16, M, C)
    g = _gen(120)
    g3, b3 = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    wg, bg = torch.randn(8 * C, C, generator=g) / math.sqrt(C), 0.1 * torch.randn(8 * C, generator=g)
    order = Wm.rowgemm_geglu_order(8 * C)
    wp, gv, cv = Wm.fold_layernorm(wg, bg, g3, b3, dtype=op16(f16))
    u, gt = folded_ln(store16(xc.ref, f16), row_stats(xc.ref), wp, gv, cv).chunk(2, dim=-1)
    return types.SimpleNamespace(xc=xc, wp=wp[order].contiguous(), gv=gv[order].contiguous(), cv=cv[order].contiguous(), ref_hidden=u * F.gelu(gt))


@functools.lru_cache(maxsize=None)
def gn_slab_case(f16, B=2, HW=240, C=320, groups=32, eps=1e-5):
    """MG_OP_GN_SLAB's normalised output: GroupNorm of O(1) values with gamma climbing the ladder over the CHANNELS (8 * 2^(13 c / C))
    and beta at 5 % of it.  ``ref`` is [B][HW][C]; it is checked transposed, each channel against its own scale."""
    g = _gen(130)
    x = (torch.randn(B, HW, C, generator=g) * 1.5 + 0.3).to(op16(f16))
    gain = (8.0 * torch.exp2(13.0 * torch.arange(C, dtype=torch.float64) / C))
    gamma = (gain * (1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64))).float()
    beta = (gain * 0.05 * torch.randn(C, generator=g, dtype=torch.float64)).float()
    ref = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1).contiguous()
    return types.SimpleNamespace(B=B, HW=HW, C=C, groups=groups, eps=eps, x=x, gamma=gamma, beta=beta, ref=ref,
                                 ref_t=ref.permute(0, 2, 1).reshape(B * C, HW).contiguous())


# --------------------------------------------------------------------------- Part B: non-finite accumulators

def plant_infs(x):
    """+inf at an interior pixel of the first image, -inf at an image-border pixel of the last ([B][C][H][W], in place), and both
    signs in one more pixel's channels, so that some outputs see inf - inf."""
    B, C, H, W = x.shape
    x[0, 5, H // 2, W // 3] = float("inf")
    x[B - 1, C - 1, 0, W - 1] = float("-inf")
    x[0, 7, H // 2 + 3, W // 3 + 4] = float("inf")
    x[0, 8, H // 2 + 3, W // 3 + 4] = float("-inf")
    return x


# --------------------------------------------------------------------------- Part C / D: the fixed-reference attention kernels

def scores_log2(q, k, scale):
    """Scores in log2 units, float64, of the operands as stored: [Tq][Tk]."""
    return (q.double() @ k.double().t()) * (scale * LOG2E)


def sdpa64(q, k, v, scale):
    s = scores_log2(q, k, scale)
    p = torch.exp2(s - s.amax(dim=1, keepdim=True))
    return (p @ v.double()) / p.sum(dim=1, keepdim=True)


def fixed_ref_row_sums(q, k, scale, f16, first=32):
    """What variants 26 / 27 compare with ``redo_thr``: sum_j 2^(s_ij - max(s_i, first 32 keys) - F4_REF_BIAS), and the largest
    single probability of each row."""
    s = scores_log2(q, k, scale)
    p = torch.exp2(s - s[:, :first].amax(dim=1, keepdim=True) - F4_REF_BIAS[f16])
    return p.sum(dim=1), p.amax(dim=1)


def excess_over_first_tile(q, k, scale, first=32):
    """Per query: max_j s_ij - max over the first key tile, log2 units (what MG_OP_FLASH_ATTN512 compares with FA5_THR)."""
    s = scores_log2(q, k, scale)
    return s.amax(dim=1) - s[:, :first].amax(dim=1)


def plant_spike(q, k, row, key, G, scale, f16, first=32):
    """Overwrite k[key] with a multiple of q[row] such that s[row][key] = max(s[row][:first]) + G log2 units (operands as stored;
    the rounding of the new key moves G by a few 1e-3).  In place on the 16-bit tensor ``k``."""
    s = scores_log2(q[row:row + 1], k[:first], scale)[0]
    want = (float(s.max()) + G) / (scale * LOG2E)
    qr = q[row].double()
    k[key] = (qr * (want / float(qr.pow(2).sum()))).to(k.dtype)


@functools.lru_cache(maxsize=None)
def flash64_window_case(f16, G, T=1024):
    """One head, T tokens of O(1) scores; for G > 0 rows 300, 301 and 470 (all in the second block of 256 queries) get their
    largest score in the last key tile, G log2 units above the maximum of their first 32 keys."""
    g = _gen(41)
    q = torch.randn(T, 64, generator=g).to(op16(f16))
    k = torch.randn(T, 64, generator=g).to(op16(f16))
    v = torch.randn(T, 64, generator=g).to(op16(f16))
    rows = (300, 301, 470)
    if G > 0:
        for i, r in enumerate(rows):
            plant_spike(q, k, r, T - 40 + 13 * i, G, 0.125, f16)
    return types.SimpleNamespace(T=T, q=q, k=k, v=v, rows=rows, ref=sdpa64(q, k, v, 0.125))


@functools.lru_cache(maxsize=None)
def flash512_window_case(f16, G, T=1000):
    """MG_OP_FLASH_ATTN512's shape of test_flash_attn512_reference_paths; rows 5, 130, 131 and 640 spike G log2 units above their
    first tile's maximum at keys past 700."""
    g = _gen(43)
    q = torch.randn(T, 512, generator=g).to(op16(f16))
    k = torch.randn(T, 512, generator=g).to(op16(f16))
    v = torch.randn(T, 512, generator=g).to(op16(f16))
    rows = (5, 130, 131, 640)
    sc = 1.0 / math.sqrt(512.0)
    for i, r in enumerate(rows):
        plant_spike(q, k, r, 700 + 3 * i, G, sc, f16)
    return types.SimpleNamespace(T=T, q=q, k=k, v=v, rows=rows, scale=sc, ref=sdpa64(q, k, v, sc))


SUBNORMAL_RUNGS = (8.0, 12.0, 16.0, 18.0, 19.0, 19.5, 20.0, 22.0, 24.0)


def subnormal_sample(T, n=512):
    """Sampled query rows: every 256-query block's first and last row, the rest spread evenly."""
    edges = sorted({r for b in range(0, T, 256) for r in (b, min(b + 255, T - 1))})
    if len(edges) >= n or T <= n:
        return torch.arange(T) if T <= n else torch.tensor(edges)
    rest = torch.linspace(0, T - 1, n - len(edges)).long().tolist()
    return torch.tensor(sorted(set(edges) | set(rest)))


@functools.lru_cache(maxsize=None)
def subnormal_case(f16, G, T):
    """Part D.  Queries of the first half of the rows: key 7 sits G log2 units above a flat background jittered within +-0.5;
    v[7] = 0 and the other values are 1 + 0.1 randn.  The second half has no dominant key (max|ref| about 1).  The reference
    (float64) is computed for ``rows`` only."""
    g = _gen(51)
    half = T // 2
    q = torch.zeros(T, 64, dtype=torch.float64)
    k = torch.zeros(T, 64, dtype=torch.float64)
    q[:half, 0] = 2.0 * G / LOG2E                    # s[i][7] = q0 * 4 * 0.125 * log2(e) = G
    k[7, 0] = 4.0
    # the jitter lives in four other channels: |q_perp| |k_perp| scale log2(e) = 0.5 bounds it, its spread is about 0.25
    qp = F.normalize(torch.randn(T, 4, generator=g, dtype=torch.float64), dim=1)
    kp = F.normalize(torch.randn(T, 4, generator=g, dtype=torch.float64), dim=1)
    q[:, 1:5] = qp * 2.0
    k[:, 1:5] = kp * (0.5 * 8.0 / (2.0 * LOG2E))
    k[7, 1:5] = 0.0
    v = 1.0 + 0.1 * torch.randn(T, 64, generator=g, dtype=torch.float64)
    v[7] = 0.0
    q, k, v = (t.to(op16(f16)) for t in (q, k, v))
    rows = subnormal_sample(T)
    return types.SimpleNamespace(T=T, q=q, k=k, v=v, rows=rows, half=half, ref=sdpa64(q[rows], k, v, 0.125))


def emulate_fixed_ref(c, f16, flush_subnormals=False):
    """Variants 26 / 27 on ``c.rows`` in float64 with the P operand rounded as the build stores it: p = 2^(s - max32 - F4_REF_BIAS)
    rounded to the operand type (fp16 keeps subnormals down to 2^-24; ``flush_subnormals``: a matrix unit that read them as 0), row
    sums and outputs from the rounded probabilities."""
    s = scores_log2(c.q[c.rows], c.k, 0.125)
    p = torch.exp2(s - s[:, :32].amax(dim=1, keepdim=True) - F4_REF_BIAS[f16])
    p = store16(p, f16)
    if flush_subnormals:
        p = torch.where(p < (2.0 ** -14 if f16 else 2.0 ** -126), torch.zeros_like(p), p)
    return (p @ c.v.double()) / p.sum(dim=1, keepdim=True)


def subnormal_ceiling(T, f16):
    """The predicted worst absolute error of a first-half row: a background sitting just under half the smallest subnormal over
    all T - 1 keys, against the dominant key's 2^-F4_REF_BIAS."""
    return (T - 1) * 2.0 ** -(25 - F4_REF_BIAS[f16]) if f16 else 0.0
