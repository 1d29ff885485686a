"""The 16-bit stores and the fixed-reference attention kernels at the edge of the operand range, on a real MI355X, in both library
builds (DESIGN.md "Operand types").  Every other GPU test feeds O(1) values; here the outputs cross +-65504.

The store model is ``tests/operand_range.py::store16`` of a float64 reference computed from the operands as stored; outputs are
pre-filled with NaN.  Each output element is in one of four classes (``operand_range.check_store``):
  saturating  |ref| >= 65520 (1 + 2^-9), fp16 build only: the output is +-65504 exactly, with the reference's sign;
  guard band  65504 (1 - 2^-9) < |ref| < 65520 (1 + 2^-9), fp16 build only: fp32 accumulation differs from float64 by about
              K 2^-24, so the output may be what the store gives for any |ref| (1 +- 2^-9) - at the limit itself 65504 or its
              neighbour 65472.  (Below the limit the band also holds 65376 ... 65440, which are exact roundings there.)  The host
              test caps the band at 2 % of the saturating elements of every case;
  regular     finite, |got - ref| <= tol * max|ref| over the regular elements of the same output ROW: the inputs span 2^13 between
              rows, and a global scale of 65504 would hide the small rows.  tol = 1.5e-2, what tests/test_gpu_kernels.py uses;
  non-finite  NaN stays NaN, +-inf is +-65504 (fp16) or +-inf (bf16), the masks equal.
No fp16 output of this module may be +-inf.  On the bf16 build the same cases pin the other half of the sentence in csrc/common.h:
"a bf16 value of 1e5 is a number".

Part C / D place attention inputs relative to each build's own constants (mirrored in operand_range.py: F4_REF_BIAS, redo_thr,
FA5_THR; the host test proves the positions in float64): the fp16 fast path with probabilities up to 2^14 in the P operand, the
fallbacks just past it, and the low end where the background probabilities are fp16 subnormals.

Measured tables, and what a library without the clamp does to this file: docs/history/operand_range.md."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import operand_range as R

pytestmark = pytest.mark.gpu

BUILDS = [False, True]   # the fp16-operand library?
BUILD_IDS = ["bf16lib", "fp16lib"]
builds = pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {False: L.init(0), True: L.init(0, True)}


def _launch(op, lib):
    """One launch, waited for.  After a GPU fault nothing more of this module is launched on the card."""
    from marigold_amd import ops
    try:
        ops.launch(op, lib=lib)
        torch.cuda.synchronize()
    except Exception as e:
        if any(w in str(e).lower() for w in ("illegal memory", "memory access fault", "hardware exception", "unspecified launch failure")):
            pytest.exit(f"GPU fault: {e}", returncode=3)
        raise


def _d(t):
    return None if t is None else t.contiguous().to("cuda")


def _nan16(f16, *shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=R.op16(f16))


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---- Part A: the 16-bit store sites on the ladder --------------------------------------------------------------------------------

@builds
@pytest.mark.parametrize("variant", [0, 23, 36, 46, 62, 72, 73])
@pytest.mark.parametrize("form", R.LINEAR_FORMS)
def test_igemm_linear_saturates(libs, f16, variant, form):
    """MG_OP_IGEMM, M = 312 (one whole and one ragged 256-row tile), K = N = 320: one tile of every kernel family with its own
    epilogue code (igemm2_body.h, the ping-pong tile, igemm2_big.hip, the hand-placed K loops)."""
    from marigold_amd import ops
    c = R.linear_case(form, f16)
    x, w, bias, rowvec, res = _d(c.x), _d(c.w), _d(c.bias), _d(c.rowvec), _d(c.res)
    out = _nan16(f16, c.M, c.N)
    _launch(ops.linear(x, w, out, M=c.M, K=c.K, N=c.N, bias=bias, rowvec=rowvec, residual=res, variant=variant), libs[f16])
    R.check_store(f"linear/{form}/v{variant}", out, c.ref, f16)


@builds
@pytest.mark.parametrize("variant,splits", [(0, 0), (36, 4)], ids=["auto", "v36_split4"])
def test_igemm_splitk_reduce_saturates(libs, f16, variant, splits):
    """splitk_reduce_kernel: the g2_auto_splitk shape of test_gpu_kernels.py (1 x 12 x 12, 1280 -> 128, 3 x 3: the automatic rule
    splits K) and one explicit split.  Only the reduced value is clamped: the fp32 partials of a regular total may themselves pass
    65504 in the upper rows, and a clamp on them would move that total."""
    from marigold_amd import ops, weights as Wm
    B, H, W, Cin, Cout = R.SPLITK_SHAPE
    c = R.conv_case(f16, B, H, W, Cin, Cout, amp=R.SPLITK_AMP)
    x, w, bias = _d(_nhwc(c.x)), _d(Wm.pack_conv3x3(c.w)), _d(c.bias)
    out = _nan16(f16, B, H, W, Cout)
    _launch(ops.igemm(x, w, out, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, N=Cout, taps=9, stride=1, pad=1, bias=bias, variant=variant,
                      splits=splits), libs[f16])
    R.check_store(f"split-K/v{variant}/splits{splits}", out.reshape(B * H * W, Cout), c.ref, f16)


def _row_stats64(rows):
    return torch.stack([rows.mean(-1), 1.0 / torch.sqrt(rows.var(-1, unbiased=False) + 1e-5)], dim=-1)


def _check_ln_out(name, stats, got, ref, f16, tol=2e-4):
    """(mean, rstd) taken by an epilogue from its fp32 values BEFORE the pack.  Every statistic is finite, the saturating rows'
    included.  Rows without a saturating element: within ``tol`` of the scale of the float64 statistics of the exact row (what
    the kernel is documented to sum), and within ``tol`` of those of the row as stored.  On the bf16 build alone the stored-row
    bound is ``tol`` plus what the store by itself moves the statistics of these rows by (``store16`` of the reference against the
    reference): rounding to 8 mantissa bits moves them by up to 3e-4 of the scale, more than 2e-4, where fp16's 11 bits move them
    by 5e-5 (tests/test_operand_range_host.py::test_row_statistics_of_the_stored_row)."""
    stats = stats.detach().double().cpu()
    assert torch.isfinite(stats).all(), f"{name}: non-finite row statistics"
    sat, guard, _, _ = R.classify(ref, True)
    rows = ~(sat | guard).any(dim=1)
    assert 4 * int(rows.sum()) >= ref.shape[0]
    exact, model = _row_stats64(ref[rows]), _row_stats64(R.store16(ref, f16)[rows])
    for which, src in (("exact", ref), ("stored", got.detach().cpu().double())):
        want = _row_stats64(src[rows])
        for j, what in enumerate(("mean", "rstd")):
            scale = float(want[:, j].abs().max())
            moved = float((exact[:, j] - model[:, j]).abs().max()) / scale if which == "stored" and not f16 else 0.0
            err = float((stats[rows][:, j] - want[:, j]).abs().max())
            print(f"[range] {name} {'fp16' if f16 else 'bf16'}: ln_out {what} of {int(rows.sum())} regular rows against the {which} row: "
                  f"max|err| {err:.3e} scale {scale:.3e} rel {err / scale:.3e} bound {tol + moved:.3e}")
            assert err <= (tol + moved) * scale, f"{name}: {what} against the {which} row {err:.4e} > {tol + moved:.3e} * {scale:.4e}"


@builds
@pytest.mark.parametrize("variant", [0, 46, 62, 72])
def test_igemm_ln_out_under_saturation(libs, f16, variant):
    """MG_OP_IGEMM ln_out on the residual form: the statistics come from the fp32 values before the pack (include/marigold_hip.h),
    so a saturating row's are those of the unclamped values - finite; the regular rows' agree with the stored row; the row-block
    tickets are back at zero."""
    from marigold_amd import ops
    c = R.linear_case("residual", f16)
    M, N = c.M, c.N
    out = _nan16(f16, M, N)
    st = torch.full((M * (N // 32 + 1), 2), float("nan"), device="cuda")
    tickets = torch.zeros(65536, dtype=torch.int32, device="cuda")
    x, w, bias, res = _d(c.x), _d(c.w), _d(c.bias), _d(c.res)
    for rep in range(2):
        _launch(ops.linear(x, w, out, M=M, K=c.K, N=N, bias=bias, residual=res, ln_out=st, ln_counters=tickets, variant=variant), libs[f16])
        assert int(tickets.abs().sum()) == 0, "tickets not back at zero"
    R.check_store(f"linear/residual+ln_out/v{variant}", out, c.ref, f16)
    _check_ln_out(f"linear/residual+ln_out/v{variant}", st[M * (N // 32):], out, c.ref, f16)


@builds
@pytest.mark.parametrize("K,waves", [(320, 4), (320, 8), (320, 12), (640, 8)])
def test_rowgemm_saturates(libs, f16, K, waves):
    """MG_OP_ROWGEMM form 0, M = 416 (13 row blocks: a ragged workgroup at 12 waves): bias + residual + row statistics, and the
    plain bias form."""
    from marigold_amd import ops, weights as Wm
    c = R.rowgemm_case(f16, K)
    pk = _d(Wm.pack_rowgemm(c.w.float(), c.bias, dtype=R.op16(f16)))
    x = _d(c.x)
    out, so = _d(c.res).clone(), torch.full((c.M, 2), float("nan"), device="cuda")     # (to_out's form: the residual in place)
    _launch(ops.rowgemm(x, pk, out, M=c.M, K=K, N=c.N, residual=out, ln_out=so, waves=waves), libs[f16])
    R.check_store(f"rowgemm/K{K}/{waves}w/bias+residual", out, c.ref, f16)
    _check_ln_out(f"rowgemm/K{K}/{waves}w/bias+residual", so, out, c.ref, f16)
    out = _nan16(f16, c.M, c.N)
    _launch(ops.rowgemm(x, pk, out, M=c.M, K=K, N=c.N, waves=waves), libs[f16])
    R.check_store(f"rowgemm/K{K}/{waves}w/bias", out, c.ref_bias, f16)


@builds
@pytest.mark.parametrize("K,waves", [(320, 4), (320, 8), (320, 12), (640, 8)])
def test_rowgemm_geglu_product_saturates(libs, f16, K, waves):
    """MG_OP_ROWGEMM form 1 (GEGLU), M = 416: the product overflows, neither factor does."""
    from marigold_amd import _lib as L, ops, weights as Wm
    c = R.geglu_case(f16, M=416, K=K)
    assert c.factor_max < 4096.0
    order = Wm.rowgemm_geglu_order(2 * c.Nh)
    pk = _d(Wm.pack_rowgemm(c.w.float()[order], c.b[order], dtype=R.op16(f16)))
    x = _d(c.x)
    out = _nan16(f16, c.M, c.Nh)
    _launch(ops.rowgemm(x, pk, out, M=c.M, K=K, N=2 * c.Nh, form=L.RG_GEGLU, waves=waves), libs[f16])
    R.check_store(f"rowgemm/K{K}/{waves}w/geglu", out, c.ref, f16)


@builds
@pytest.mark.parametrize("waves", [4, 8, 12])
def test_rowgemm_qkv_transposed_section_saturates(libs, f16, waves):
    """MG_OP_ROWGEMM form 2 (QKV), one image of 416 tokens, K = C = 320: columns >= 2C go to V^T in the attention kernel's
    permuted key order (un-permuted here for the row-wise check).  The pad columns stay zero."""
    from marigold_amd import _lib as L, ops, weights as Wm
    c = R.qkv_case(f16, 416, B=1, C=320)
    C, T, ldt = c.C, c.T, c.T + 32
    pk = _d(Wm.pack_rowgemm(c.w.float(), c.b, dtype=R.op16(f16)))
    x = _d(c.x)
    qk = _nan16(f16, c.M, 2 * C)
    vt = torch.zeros(1, C, ldt, device="cuda", dtype=R.op16(f16))
    vt[:, :, :T] = float("nan")
    _launch(ops.rowgemm(x, pk, qk, M=c.M, K=c.K, N=3 * C, form=L.RG_QKV, ldo=2 * C, vt=vt, tokens=T, ldt=ldt, trans_from=2 * C, waves=waves), libs[f16])
    assert not vt[:, :, T:].any(), "V^T pad columns were written"
    R.check_store(f"rowgemm/{waves}w/qkv/qk", qk, c.ref[:, :2 * C], f16)
    nat = ops.permute_vt_keys(vt[:, :, :T].contiguous())       # (the permutation swaps two blocks of four: its own inverse)
    R.check_store(f"rowgemm/{waves}w/qkv/vt", nat.permute(0, 2, 1).reshape(c.M, C), c.ref[:, 2 * C:], f16)


@builds
@pytest.mark.parametrize("variant,fused", [(0, False), (0, True), (6, False), (6, True), (10, False), (11, False)])
def test_conv3x3_saturates(libs, f16, variant, fused):
    """MG_OP_CONV3X3, B = 2, 12 x 20, 320 -> 320: the 12-wave tiles plain and with the fused scale / shift + SiLU (whose normalised
    operand is itself a 16-bit store on its way into LDS: the reference applies ``store16`` there), the four-wave tiles plain."""
    from marigold_amd import ops, weights as Wm
    B, H, W, Cin, Cout = R.CONV_SHAPE
    Cout = 256 if variant == 10 else Cout            # (the 16 x 16 x 256 tile takes multiples of 256 channels)
    c = R.conv_case(f16, B, H, W, Cin, Cout, fused=fused, amp=R.CONV_FUSED_AMP if fused else R.CONV_AMP)
    x, w, bias, ss = _d(_nhwc(c.x)), _d(Wm.pack_conv3x3(c.w)), _d(c.bias), _d(c.ss)
    out = _nan16(f16, B, H, W, Cout)
    _launch(ops.conv3x3(x, w, out, B=B, H=H, W=W, C0=Cin, N=Cout, ss=ss, silu=fused, bias=bias, variant=variant), libs[f16])
    R.check_store(f"conv3x3/v{variant}/{'fused' if fused else 'plain'}", out.reshape(B * H * W, Cout), c.ref, f16)


@builds
def test_gn_apply_saturates(libs, f16):
    """MG_OP_GN_APPLY: x * scale + shift crosses the limit in the ladder's upper rows."""
    from marigold_amd import ops
    c = R.gn_apply_case(f16)
    x, ss = _d(c.x), _d(c.ss)
    out = _nan16(f16, c.B, c.HW, c.C)
    _launch(ops.gn_apply(x, ss, out, B=c.B, HW=c.HW, C=c.C, silu=False), libs[f16])
    R.check_store("gn_apply", out.reshape(c.B * c.HW, c.C), c.ref, f16)


@builds
@pytest.mark.parametrize("variant", [0, 36, 62, 72, 73])
def test_igemm_geglu_product_saturates(libs, f16, variant):
    """MG_OP_IGEMM's GEGLU epilogue: u * gelu(g) overflows though neither factor comes near the limit (a few thousand each)."""
    from marigold_amd import _lib as L, ops, weights as Wm
    c = R.geglu_case(f16)
    assert c.factor_max < 4096.0
    wp, bp = Wm.pack_geglu(c.w, c.b)
    x, wp, bp = _d(c.x), _d(wp), _d(bp)
    out = _nan16(f16, c.M, c.Nh)
    _launch(ops.linear(x, wp, out, M=c.M, K=c.K, N=2 * c.Nh, bias=bp, epi=L.EPI_GEGLU, variant=variant), libs[f16])
    R.check_store(f"geglu/v{variant}", out, c.ref, f16)


@builds
@pytest.mark.parametrize("variant", [0, 23, 62])
@pytest.mark.parametrize("T", [160, 156], ids=["16-byte", "scalar-tail"])
def test_igemm_transposed_section_saturates(libs, f16, variant, T):
    """The transposed V^T section of a fused QKV launch, 2 images x T tokens: eight tokens of one channel as one 16-byte store
    (T = 160), and the scalar store of a token count that is no multiple of 8 (T = 156).  The pad columns stay zero."""
    from marigold_amd import ops
    c = R.qkv_case(f16, T)
    C, ldt = c.C, 192
    x, w, b = _d(c.x), _d(c.w), _d(c.b)
    qk = _nan16(f16, c.M, 3 * C)
    vt = torch.zeros(c.B, C, ldt, device="cuda", dtype=R.op16(f16))
    vt[:, :, :T] = float("nan")
    _launch(ops.igemm(x, w, qk, B=c.B, H=T, W=1, Cin=c.K, Ho=T, Wo=1, N=3 * C, bias=b, out2=vt, trans_from=2 * C, ldt=ldt, variant=variant),
            libs[f16])
    assert not vt[:, :, T:].any(), "V^T pad columns were written"
    R.check_store(f"qkv/T{T}/v{variant}/qk", qk[:, :2 * C], c.ref[:, :2 * C], f16)
    R.check_store(f"qkv/T{T}/v{variant}/vt", vt[:, :, :T].permute(0, 2, 1).reshape(c.M, C), c.ref[:, 2 * C:], f16)


@builds
@pytest.mark.parametrize("variant", [0, 6])
def test_conv3x3_subpixel_saturates(libs, f16, variant):
    """MG_OP_CONV3X3's sub-pixel up-sampling form, B = 2, 12 x 20 -> 24 x 40, 320 -> 320."""
    from marigold_amd import ops
    B, H, W, Cin, Cout = R.CONV_SHAPE
    c = R.subpix_case(f16, B, H, W, Cin, Cout)
    x, ws, bias = _d(_nhwc(c.x)), _d(c.ws), _d(c.bias)
    out = _nan16(f16, B, 2 * H, 2 * W, Cout)
    _launch(ops.conv3x3(x, ws, out, B=B, H=H, W=W, C0=Cin, N=Cout, subpix=True, bias=bias, wz=Cout * 4 * Cin, variant=variant), libs[f16])
    R.check_store(f"conv3x3/v{variant}/sub-pixel", out.reshape(B * 4 * H * W, Cout), c.ref, f16)


@builds
def test_im2col_small_saturates(libs, f16):
    """MG_OP_IM2COL_SMALL (misc.hip::im2col_small_kernel): fp32 latents beyond the limit, both infinities among them, to operand
    rows - a conversion only, so every element equals the store model."""
    from marigold_amd import ops
    c = R.im2col_case()
    a, b = _d(c.a), _d(c.b)
    col = _nan16(f16, c.B * c.H * c.W, c.Kp)
    _launch(ops.im2col_small(a, b, col, B=c.B, H=c.H, W=c.W, C0=c.C0, C1=c.C1, Kp=c.Kp), libs[f16])
    got, want = col.cpu().double(), R.store16(c.rows, f16)
    n_over = int((c.rows.abs() >= R.F16_OVER).sum())
    assert n_over > 1000
    print(f"[range] im2col_small {'fp16' if f16 else 'bf16'}: {n_over} of {got.numel()} elements at or beyond 65520, {int((got != want).sum())} differ from the store model")
    assert torch.equal(got, want)
    assert not f16 or not torch.isinf(got).any()


@builds
@pytest.mark.parametrize("silu", [False, True], ids=["affine", "silu"])
def test_conv3x3_head_operand_pack_saturates(libs, f16, silu):
    """MG_OP_CONV3X3_HEAD: the reference applies ``store16`` to the normalised value and then convolves in float64.  The outputs
    are fp32 and cross no limit themselves: each is held to 4e-3 (test_conv3x3_head's bound) of the largest reference of its own
    and the two neighbouring image lines (the 3 x 3 taps mix them; the ladder moves by 2^0.54 per line), and must be finite - an
    fp16 inf in the packed patch would show as inf or NaN."""
    from marigold_amd import ops, weights as Wm
    c = R.head_case(f16, silu)
    B, H, W, C, Cout, npad = c.B, c.H, c.W, c.C, c.Cout, 8
    wd = torch.zeros(npad, 9 * C, dtype=R.op16(f16))
    wd[:Cout] = Wm.pack_conv3x3(c.w)
    x, ss, wd, bias = _d(_nhwc(c.x)), _d(c.ss), _d(wd), _d(c.bias)
    out = torch.full((B * H * W, npad), float("nan"), device="cuda")
    _launch(ops.conv3x3_head(x, ss, wd, bias, out, B=B, H=H, W=W, C=C, Cout=Cout, ldo=npad, silu=silu), libs[f16])
    assert torch.isnan(out[:, Cout:]).all(), "the padding columns were written"
    got = out[:, :Cout].reshape(B, H, W, Cout).cpu().double()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} non-finite outputs"
    line = c.ref.abs().amax(dim=(2, 3))                                            # [B][H]
    pad = F.pad(line, (1, 1))
    scale = torch.stack([pad[:, :-2], pad[:, 1:-1], pad[:, 2:]]).amax(0)[:, :, None, None]
    worst = float(((got - c.ref).abs() / scale).max())
    n_over = int((c.h.abs() >= R.F16_OVER).sum())
    print(f"[range] conv3x3_head/{'silu' if silu else 'affine'} {'fp16' if f16 else 'bf16'}: {n_over} of {c.h.numel()} normalised values at or beyond 65520, "
          f"worst |err| / scale of the three lines {worst:.3e}")
    assert worst <= 4e-3


# ---- Part A, the forms behind a folded LayerNorm: the ladder runs over the output columns, each checked against its own scale ----

def _geglu_pack_order(n2):
    from marigold_amd import weights as Wm
    idx = torch.arange(n2, dtype=torch.float32)
    return Wm.pack_geglu(idx[:, None], idx)[1].long()


@builds
@pytest.mark.parametrize("variant", [0, 36, 46, 62, 72, 73])
def test_igemm_layernorm_fold_saturates(libs, f16, variant):
    """MG_OP_IGEMM with ln_in (out = rstd (x Wp^T - mean g) + c), M = 416, K = N = 320, 2e-2 as test_igemm_layernorm_fold."""
    from marigold_amd import ops
    c = R.ln_fold_case(f16, False)
    wp, gv, cv, ref = R.ln_fold_operands(c)
    x, st, wp, gv, cv = _d(c.x), _d(c.st), _d(wp), _d(gv), _d(cv)
    out = _nan16(f16, c.M, c.N)
    _launch(ops.linear(x, wp, out, M=c.M, K=c.K, N=c.N, ln_in=st, ln_g=gv, ln_c=cv, variant=variant), libs[f16])
    R.check_store(f"ln_fold/v{variant}", out.t(), ref.t(), f16, tol=2e-2)


@builds
@pytest.mark.parametrize("variant", [0, 62, 72, 73])
def test_igemm_layernorm_fold_geglu_saturates(libs, f16, variant):
    """The same in front of the GEGLU epilogue: the product of a column's pair crosses the limit, neither factor does."""
    from marigold_amd import _lib as L, ops
    c = R.ln_fold_case(f16, True)
    wp, gv, cv, ref = R.ln_fold_operands(c, _geglu_pack_order(c.N))
    x, st, wp, gv, cv = _d(c.x), _d(c.st), _d(wp), _d(gv), _d(cv)
    out = _nan16(f16, c.M, c.Nh)
    _launch(ops.linear(x, wp, out, M=c.M, K=c.K, N=c.N, epi=L.EPI_GEGLU, ln_in=st, ln_g=gv, ln_c=cv, variant=variant), libs[f16])
    R.check_store(f"ln_fold/geglu/v{variant}", out.t(), ref.t(), f16, tol=2e-2)


@builds
@pytest.mark.parametrize("K,waves", [(320, 4), (320, 8), (320, 12), (640, 8)])
def test_rowgemm_geglu_with_ln_in_saturates(libs, f16, K, waves):
    """MG_OP_ROWGEMM form 1 as the transformer runs it: GEGLU behind the folded LayerNorm, M = 416."""
    from marigold_amd import _lib as L, ops, weights as Wm
    c = R.ln_fold_case(f16, True, K=K)
    wp, gv, cv, ref = R.ln_fold_operands(c, Wm.rowgemm_geglu_order(c.N))
    pk = _d(Wm.pack_rowgemm(wp.float(), cv, gv, dtype=R.op16(f16)))
    x, st = _d(c.x), _d(c.st)
    out = _nan16(f16, c.M, c.Nh)
    _launch(ops.rowgemm(x, pk, out, M=c.M, K=K, N=c.N, form=L.RG_GEGLU, ln_in=st, waves=waves), libs[f16])
    R.check_store(f"rowgemm/K{K}/{waves}w/ln_in+geglu", out.t(), ref.t(), f16, tol=2e-2)


def _finite_stats(name, so):
    assert torch.isfinite(so).all(), f"{name}: non-finite row statistics"


@builds
def test_igemm_xattn2_epilogue_saturates(libs, f16):
    """MG_EPI_XATTN2 in place on the residual stream, M = 312, C = 320, 5 heads: P VO^T + bias + x crosses the limit where the
    rows of x are large; the probabilities are rounded to operands where the kernel packs them (``store16`` in the reference)."""
    from marigold_amd import _lib as L, ops
    c = R.xattn_case(f16, 312)
    h, st, wp, gv, cv, vot, bias = _d(c.x).clone(), _d(c.st), _d(c.wp), _d(c.gv), _d(c.cv), _d(c.vot), _d(c.bias)
    mr = torch.full((c.M, 2), float("nan"), device="cuda")
    _launch(ops.linear(h, wp, h, M=c.M, K=c.C, N=64, epi=L.EPI_XATTN2, ln_in=st, ln_g=gv, ln_c=cv, sm_scale=c.scale, sm_cols=2 * c.heads,
                       out2=vot, c2=c.C, ldo=c.C, bias=bias, residual=h, ldr=c.C, ln_out=mr), libs[f16])
    R.check_store("xattn2 epilogue", h, c.ref, f16)
    _finite_stats("xattn2 epilogue", mr)


def _pack_xattn(c, f16):
    from marigold_amd import weights as Wm
    pack = Wm.pack_rowgemm_xattn if c.C == 320 else Wm.pack_rowgemm_xattn_ksplit
    return _d(pack(c.wp.float(), c.cv, c.gv, c.vot.float(), c.bias, dtype=R.op16(f16)))


@builds
@pytest.mark.parametrize("C,heads,waves", [(320, 5, 8), (320, 5, 12), (640, 10, 0)])
def test_rowgemm_xattn_saturates(libs, f16, C, heads, waves):
    """MG_OP_ROWGEMM form 3 (RG_XATTN), in place, M = 416: the K = 320 kernel at 8 and 12 waves, and at K = 640 the K-split kernel
    (rowgemm_xattn_ksplit_kernel, a store site of its own)."""
    from marigold_amd import _lib as L, ops
    c = R.xattn_case(f16, 416, C, heads)
    pk, h, st = _pack_xattn(c, f16), _d(c.x).clone(), _d(c.st)
    so = torch.full((c.M, 2), float("nan"), device="cuda")
    _launch(ops.rowgemm(h, pk, h, M=c.M, K=c.C, N=64, form=L.RG_XATTN, ln_in=st, ln_out=so, sm_cols=2 * c.heads, sm_scale=c.scale, waves=waves),
            libs[f16])
    R.check_store(f"rowgemm/C{C}/{waves}w/xattn", h, c.ref, f16)
    _finite_stats(f"rowgemm/C{C}/{waves}w/xattn", so)


@builds
@pytest.mark.parametrize("waves", [4, 8, 12])
def test_rowgemm_xattn_prologue_of_geglu_saturates(libs, f16, waves):
    """MG_OP_ROWGEMM form 1 with the cross-attention prologue, out of place: the updated rows go to P_XOUT through a 16-bit store
    (checked like every store) and are fed on as stored - the hidden activations are those of ``store16`` of the rows, normalised
    with the statistics of the fp32 rows before that store (2e-2, the row kernel's GEGLU bound)."""
    from marigold_amd import _lib as L, ops, weights as Wm
    c = R.xattn_geglu_case(f16)
    xc = c.xc
    pkx = _pack_xattn(xc, f16)
    pkg = _d(Wm.pack_rowgemm(c.wp.float(), c.cv, c.gv, dtype=R.op16(f16)))
    x_in, st = _d(xc.x), _d(xc.st)
    rows, hid = _nan16(f16, xc.M, xc.C), _nan16(f16, xc.M, 4 * xc.C)
    _launch(ops.rowgemm(x_in, pkg, hid, M=xc.M, K=xc.C, N=8 * xc.C, form=L.RG_GEGLU, ln_in=st, waves=waves, xattn=pkx, xout=rows,
                        sm_cols=2 * xc.heads, sm_scale=xc.scale), libs[f16])
    assert torch.equal(x_in.cpu(), xc.x), "the input rows were written"
    R.check_store(f"rowgemm/{waves}w/xattn prologue/rows", rows, xc.ref, f16)
    R.check_store(f"rowgemm/{waves}w/xattn prologue/hidden", hid, c.ref_hidden, f16, tol=2e-2)


@builds
def test_gn_slab_normalised_output_saturates(libs, f16):
    """MG_OP_GN_SLAB's normalised output, B = 2, 240 pixels, 320 channels in 32 groups, gamma on the ladder over the channels."""
    from marigold_amd import ops
    c = R.gn_slab_case(f16)
    x, gamma, beta = _d(c.x), _d(c.gamma), _d(c.beta)
    out, ss = _nan16(f16, c.B, c.HW, c.C), torch.full((c.B, 2, c.C), float("nan"), device="cuda")
    _launch(ops.gn_slab(x, out, ss, B=c.B, HW=c.HW, C=c.C, groups=c.groups, gamma=gamma, beta=beta, eps=c.eps), libs[f16])
    assert torch.isfinite(ss).all()
    R.check_store("gn_slab", out.permute(0, 2, 1).reshape(c.B * c.C, c.HW), c.ref_t, f16)


@builds
@pytest.mark.parametrize("variant", [9, 1])
def test_conv3x3_gn_table_is_of_the_values_as_stored(libs, f16, variant):
    """MG_OP_CONV3X3 p[8], documented as the GroupNorm sums "of the values as stored": 320 -> 256 on the tiles that produce the
    table, reduced by MG_OP_GN_FINALIZE with gamma = 1, beta = 0 to (rstd, -mean rstd) per channel, against the float64 statistics
    of the output tensor as read back (saturated where the fp16 build saturates), 2e-4 of the scale as
    test_conv3x3_patch_output_groupnorm_statistics."""
    from marigold_amd import ops, weights as Wm
    B, H, W, Cin = R.CONV_SHAPE[:4]
    N, cpg, HW = 256, 8, H * W
    c = R.conv_case(f16, B, H, W, Cin, N, amp=R.CONV_AMP)
    x, w, bias = _d(_nhwc(c.x)), _d(Wm.pack_conv3x3(c.w)), _d(c.bias)
    out = _nan16(f16, B, H, W, N)
    kw = dict(B=B, H=H, W=W, C0=Cin, N=N, bias=bias, variant=variant)
    slots = ops.conv3x3_gn_slots(ops.conv3x3(x, w, out, **kw), f16)
    assert slots > 0
    part = torch.full((B, slots, 32, 2), float("nan"), device="cuda")
    _launch(ops.conv3x3(x, w, out, gn_part=part, gn_cpg=cpg, gn_slots=slots, **kw), libs[f16])
    R.check_store(f"conv3x3/v{variant}/with the table", out.reshape(B * HW, N), c.ref, f16)
    ss = torch.full((B, 2, N), float("nan"), device="cuda")
    one, zero = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    _launch(ops.gn_finalize(part, one, zero, ss, B=B, C=N, groups=32, slots=slots, HW=HW, eps=1e-6), libs[f16])
    o = out.cpu().double().reshape(B, HW, 32, cpg)
    assert torch.isfinite(o).all()
    mean, var = o.mean(dim=(1, 3)), o.var(dim=(1, 3), unbiased=False)
    rstd = (var + 1e-6).rsqrt()
    for what, got, want in (("rstd", ss[:, 0], rstd.repeat_interleave(cpg, 1)), ("-mean rstd", ss[:, 1], (-mean * rstd).repeat_interleave(cpg, 1))):
        got = got.cpu().double()
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"[range] conv3x3/v{variant} GroupNorm table {'fp16' if f16 else 'bf16'}: {what} against the output as read back: max|err| {err:.3e} scale {scale:.3e} rel {err / scale:.3e}")
        assert torch.isfinite(got).all() and err <= 2e-4 * scale, (what, err, scale)


# ---- Part B: non-finite accumulators ---------------------------------------------------------------------------------------------

def _conv_inputs(f16, B, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = R.plant_infs(torch.randn(B, Cin, H, W, generator=g).to(R.op16(f16)))
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(R.op16(f16))
    bias = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x.float(), w.float(), bias, padding=1)          # fp32 torch on the CPU: inf - inf and inf * 0 are NaN there too
    ref = ref.permute(0, 2, 3, 1).reshape(B * H * W, Cout).double()
    assert torch.isnan(ref).any() and (ref == float("inf")).any() and (ref == float("-inf")).any()
    return x, w, bias, ref


@builds
@pytest.mark.parametrize("B,H,W,Cin,Cout,variant", [(2, 16, 24, 128, 192, 36), (1, 12, 12, 1280, 128, 0)], ids=["v36", "auto_splitk"])
def test_nonfinite_accumulator_igemm_conv(libs, f16, B, H, W, Cin, Cout, variant):
    """+inf at an interior pixel, -inf at an image-border pixel, both in one more: an infinite accumulator is stored as +-65504 by
    the fp16 build and as +-inf by the bf16 build, inf - inf as NaN, everything else within the regular bound."""
    from marigold_amd import ops, weights as Wm
    x, w, bias, ref = _conv_inputs(f16, B, H, W, Cin, Cout, 300 + variant)
    out = _nan16(f16, B, H, W, Cout)
    xd, wd, bd = _d(_nhwc(x)), _d(Wm.pack_conv3x3(w)), _d(bias)
    _launch(ops.igemm(xd, wd, out, B=B, H=H, W=W, Cin=Cin, Ho=H, Wo=W, N=Cout, taps=9, stride=1, pad=1, bias=bd, variant=variant), libs[f16])
    st = R.check_store(f"non-finite/igemm conv/v{variant}", out.reshape(B * H * W, Cout), ref, f16)
    assert st["nonfinite"] > 0


@builds
@pytest.mark.parametrize("variant", [0, 6])
def test_nonfinite_accumulator_conv3x3(libs, f16, variant):
    from marigold_amd import ops, weights as Wm
    B, H, W, Cin, Cout = 2, 12, 20, 320, 320
    x, w, bias, ref = _conv_inputs(f16, B, H, W, Cin, Cout, 310 + variant)
    out = _nan16(f16, B, H, W, Cout)
    xd, wd, bd = _d(_nhwc(x)), _d(Wm.pack_conv3x3(w)), _d(bias)
    _launch(ops.conv3x3(xd, wd, out, B=B, H=H, W=W, C0=Cin, N=Cout, bias=bd, variant=variant), libs[f16])
    st = R.check_store(f"non-finite/conv3x3/v{variant}", out.reshape(B * H * W, Cout), ref, f16)
    assert st["nonfinite"] > 0


@builds
def test_nonfinite_accumulator_rowgemm(libs, f16):
    from marigold_amd import ops, weights as Wm
    M, C = 416, 320
    g = torch.Generator().manual_seed(320)
    x = torch.randn(M, C, generator=g).to(R.op16(f16))
    x[77, 11], x[M - 1, 0] = float("inf"), float("-inf")
    x[200, 3], x[200, 300] = float("inf"), float("-inf")
    w, b = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(R.op16(f16)), 0.1 * torch.randn(C, generator=g)
    ref = (x.float() @ w.float().t() + b).double()
    assert torch.isnan(ref).any() and (ref == float("inf")).any() and (ref == float("-inf")).any()
    out = _nan16(f16, M, C)
    xd, pk = _d(x), _d(Wm.pack_rowgemm(w.float(), b, dtype=R.op16(f16)))
    _launch(ops.rowgemm(xd, pk, out, M=M, K=C, N=C), libs[f16])
    st = R.check_store("non-finite/rowgemm bias", out, ref, f16)
    assert st["nonfinite"] > 0


# ---- Part C: the fp16 window of the fixed-reference attention kernels ------------------------------------------------------------

def _flash64(lib, c, f16, variant, split=2, rows=None):
    """One head of ``c`` through MG_OP_FLASH_ATTN64 -> the output rows asked for (CPU); variant 21 reads the natural V^T, the
    others the permuted one; ``split`` = 1: with the workspace, pieces along the keys (tickets checked)."""
    from marigold_amd import ops
    T = c.T
    qk = _d(torch.cat([c.q, c.k], dim=-1)[None])
    vt = _d(c.v.t()[None])
    perm = variant != 21
    if perm:
        vt = ops.permute_vt_keys(vt)
    ws = torch.zeros(ops.FLASH_WS_BYTES, dtype=torch.uint8, device="cuda") if split == 1 else None
    out = _nan16(f16, 1, T, 64)
    _launch(ops.flash_attn64(qk, qk[:, :, 64:], vt, out, B=1, heads=1, Ntok=T, ldq=128, ldo=64, ldvt=T, sq=0, sk=0, svt=0, so=0, scale=0.125,
                             variant=variant, vt_perm=perm, ws=ws, ws_bytes=ops.FLASH_WS_BYTES if split == 1 else 0, split=split), lib)
    if split == 1:
        assert int(ws[:4096].view(torch.int32).abs().sum()) == 0, "tickets not back at zero"
    out = out[0] if rows is None else out[0][rows.to("cuda")]
    return out.cpu().double()


def _attn_close(name, got, ref, f16):
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"[range] {name} {'fp16' if f16 else 'bf16'}: max|err| {err:.3e} scale {scale:.3e} rel {err / scale:.3e}")
    assert err <= 1.5e-2 * scale, f"{name}: max|err| {err:.4e} > 1.5e-2 * {scale:.4e}"
    return err / scale


@builds
@pytest.mark.parametrize("variant", [26, 27], ids=["mfma32x32x16", "mfma16x16x32"])
@pytest.mark.parametrize("split", [2, 1], ids=["whole", "keysplit"])
@pytest.mark.parametrize("G", R.FLASH64_G)
def test_flash_attn64_fp16_window(libs, f16, variant, split, G):
    """Variants 26 / 27, T = 1024: rows 300, 301 and 470 have their largest score in the last key tile, G log2 units above the
    maximum of their first 32 keys.  fp16 build: up to G = 20 the row sums against max32 + 6 stay below 2^15 (2^14.0 at G = 20:
    probabilities up to 2^14 in the P operand, no fallback); at G = 22 the row sum passes 2^15, at G = 26 a single probability
    (2^20) overflows the P operand before the row sum tells - the block of 256 queries redoes with the running maximum either way,
    and its other rows move against the launch without the spike as the float64 reference does.  bf16 build: all of them fast path."""
    c, c0 = R.flash64_window_case(f16, G), R.flash64_window_case(f16, 0.0)
    got = _flash64(libs[f16], c, f16, variant, split)
    _attn_close(f"flash_attn64 window/v{variant}/split{split}/G{G}", got, c.ref, f16)
    got0 = _flash64(libs[f16], c0, f16, variant, split)
    _attn_close(f"flash_attn64 window/v{variant}/split{split}/no spike", got0, c0.ref, f16)
    other = torch.ones(256, dtype=torch.bool)
    other[[r - 256 for r in c.rows]] = False
    blk = slice(256, 512)
    moved, want = (got[blk] - got0[blk])[other], (c.ref[blk] - c0.ref[blk])[other]
    d = float((moved - want).abs().max())
    print(f"[range] flash_attn64 window/v{variant}/split{split}/G{G}: the block's other rows against the launch without the spike: {d:.3e}")
    assert d <= 1.5e-2 * float(c.ref.abs().max())


@builds
@pytest.mark.parametrize("G", R.FLASH512_G)
def test_flash_attn512_fp16_window(libs, f16, G):
    """MG_OP_FLASH_ATTN512, T = 1000: spikes of 8, 12 and 14.9 log2 units over the first tile's maximum retry on neither build;
    15.5 (a probability that still fits fp16) and 17 (one that would not) retry on the fp16 build (FA5_THR = 15), not on bf16 (60)."""
    from marigold_amd import ops
    c = R.flash512_window_case(f16, G)
    T, C = c.T, 512
    ldvt = ((T + 63) // 64) * 64
    qk = torch.zeros(T + 8, 2 * C, device="cuda", dtype=R.op16(f16))
    qk[:T] = _d(torch.cat([c.q, c.k], dim=-1))
    vt = torch.zeros(1, C, ldvt, device="cuda", dtype=R.op16(f16))
    vt[0, :, :T] = _d(c.v.t())
    out = _nan16(f16, 1, T, C)
    _launch(ops.flash_attn512(qk, qk.data_ptr() + C * 2, vt, out, B=1, Ntok=T, ldq=2 * C, ldo=C, ldvt=ldvt, sq=T * 2 * C, sk=T * 2 * C,
                              svt=C * ldvt, so=T * C, scale=c.scale), libs[f16])
    _attn_close(f"flash_attn512 window/G{G}", out[0].cpu().double(), c.ref, f16)


# ---- Part D: the low end - subnormal probabilities -------------------------------------------------------------------------------

@builds
@pytest.mark.parametrize("variant", [26, 27, 21, 25])
@pytest.mark.parametrize("T", [1024, 9216])
@pytest.mark.parametrize("G", R.SUBNORMAL_RUNGS)
def test_flash_attn64_subnormal_probabilities(libs, f16, variant, T, G):
    """Key 7 dominates the first half of the queries by G log2 units over a flat background, v[7] = 0, the other values 1 + 0.1
    randn: in the fp16 build's fixed-reference kernels the background probabilities are 2^(-G - 6 +- 0.5) - fp16 subnormals from
    G = 8, a single step of 2^-24 at G = 18, and gone by design from G = 19.5, where the lost mass is at most
    (T - 1) 2^-(25 - F4_REF_BIAS) of the dominant key's (emulated in tests/test_operand_range_host.py: 1.25e-2 at T = 9216,
    G = 19.5, against the 1.5e-2 asserted here; a matrix unit that flushed subnormal inputs would give 0.70 at G = 12).  The
    compiled kernel (21 / 25) keeps a running maximum and has no such window.  Reference: float64 for the sampled rows (every
    256-query block's first and last row among them)."""
    c = R.subnormal_case(f16, G, T)
    got = _flash64(libs[f16], c, f16, variant, rows=c.rows)
    first = c.rows < c.half
    rel_rows = float(((got - c.ref).abs().amax(1) / c.ref.abs().amax(1))[first].max())
    emu = float((R.emulate_fixed_ref(c, f16) - c.ref).abs().max()) if variant in (26, 27) else float("nan")
    print(f"[range] subnormal ladder v{variant} T={T} G={G} {'fp16' if f16 else 'bf16'}: emulated {emu:.3e}, worst per-row relative error of the first half {rel_rows:.3e}")
    _attn_close(f"flash_attn64 subnormal/v{variant}/T{T}/G{G}", got, c.ref, f16)
