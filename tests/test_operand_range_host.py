"""The helpers of tests/operand_range.py and the input conditions of tests/test_gpu_operand_range.py, on the CPU: the store model
against torch's own conversions, every Part A case's class counts from its float64 reference alone, the positions of the attention
cases relative to each build's thresholds, and the emulated subnormal ladder."""
import math

import numpy as np
import pytest
import torch

from tests import operand_range as R

BUILDS = [False, True]
BUILD_IDS = ["bf16", "fp16"]


def _sweep():
    f = np.float32
    v = [0.0, -0.0, 1.0, -1.0, 1.0 / 3.0, 5.96e-8, 2.98e-8, 2.9802322e-8, 8.9e-8, 6.1e-5, 6.0975552e-5, 1e-40, 3e-39,
         2047.0, 2049.0, 2051.0, 60000.0, 65471.0, 65472.0, 65488.0, 65503.0, 65504.0, 65519.0, 65519.99, 65520.0, 65521.0, 65536.0,
         1e5, 1e30, 3.38e38, 3.3895314e38, 3.3961775e38, 3.4e38, float("inf"), float("nan")]
    v = np.array(v + [-x for x in v], dtype=f)
    g = np.random.default_rng(0)
    rnd = (g.standard_normal(20000) * np.exp2(g.uniform(-30, 18, 20000))).astype(f)
    near = (65504.0 + g.uniform(-64, 64, 4000)).astype(f) * np.where(g.uniform(size=4000) < 0.5, -1, 1).astype(f)
    tiny = (g.standard_normal(4000) * 2.0 ** -20).astype(f)      # fp16 subnormals
    huge = (g.uniform(0.9, 1.0, 2000) * 3.4028235e38).astype(f) * np.where(g.uniform(size=2000) < 0.5, -1, 1).astype(f)   # bf16's own overflow
    return torch.from_numpy(np.concatenate([v, rnd, near, tiny, huge]))


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_store16_equals_torch_conversion_plus_clamp(f16):
    """fp32 values (what a kernel holds before its store) through ``store16`` and through torch: ``.to(bfloat16)`` is the bf16
    store as it is (overflow to inf); the fp16 store is ``.to(float16)`` followed by a clamp to +-65504 that keeps NaN."""
    x = _sweep()
    got = R.store16(x.double(), f16)
    if f16:
        want = x.to(torch.float16).double()
        want = torch.where(torch.isnan(want), want, want.clamp(-65504.0, 65504.0))
    else:
        want = x.to(torch.bfloat16).double()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = torch.isnan(want) | (got == want)
    assert bool(ok.all()), [(float(a), float(b), float(c)) for a, b, c in zip(x[~ok][:8], got[~ok][:8], want[~ok][:8])]
    assert torch.equal(torch.signbit(got[~torch.isnan(got)]), torch.signbit(want[~torch.isnan(want)]))


def test_store16_named_values():
    s = lambda v, f16: float(R.store16(torch.tensor([v], dtype=torch.float64), f16)[0])   # noqa: E731
    assert s(65503.0, True) == 65504.0 and s(65504.0, True) == 65504.0 and s(65519.99, True) == 65504.0
    assert s(65520.0, True) == 65504.0 and s(-65520.0, True) == -65504.0 and s(1e5, True) == 65504.0
    assert s(float("inf"), True) == 65504.0 and s(float("-inf"), True) == -65504.0 and math.isnan(s(float("nan"), True))
    assert s(65488.0, True) == 65472.0 and s(65488.1, True) == 65504.0        # the tie goes to the even mantissa (65472)
    assert s(2.0 ** -25, True) == 0.0 and s(2.0 ** -25 * 1.01, True) == 2.0 ** -24 and s(2.0 ** -24, True) == 2.0 ** -24
    assert s(1e5, False) == 99840.0 and s(65520.0, False) == 65536.0
    assert s(3.3962e38, False) == float("inf") and s(-3.4e38, False) == float("-inf") and s(3.3895314e38, False) == 3.3895313892515355e38
    assert s(float("inf"), False) == float("inf") and math.isnan(s(float("nan"), False))


def test_classes_partition_and_check_store_bites():
    """Every element is in exactly one class; ``check_store`` accepts the model's own output and refuses an inf where 65504
    belongs, a clamped NaN, a value one step off in the saturating class and a regular error above the row's bound."""
    ref = R.linear_case("residual", True).ref.clone()
    ref[3, 5], ref[4, 6], ref[5, 7] = float("nan"), float("inf"), float("-inf")
    for f16 in BUILDS:
        sat, guard, reg, nonfin = R.classify(ref, f16)
        assert bool((sat.int() + guard.int() + reg.int() + nonfin.int() == 1).all())
        assert (int(sat.sum()) > 0) == f16 and int(nonfin.sum()) == 3
        good = R.store16(ref, f16).to(R.op16(f16))
        st = R.check_store("model", good, ref, f16)
        assert st["exact"] == st["sat"] and st["worst"] < (2.0 ** -11 if f16 else 2.0 ** -8)
    good = R.store16(ref, True).to(torch.float16)
    sat, _, reg, _ = R.classify(ref, True)
    r, c = [int(t[0]) for t in torch.nonzero(sat, as_tuple=True)]
    for name, val, where in (("inf", float("inf") * float(torch.sign(ref[r, c])), (r, c)), ("one step off", 65472.0 * float(torch.sign(ref[r, c])), (r, c)),
                             ("clamped NaN", -65504.0, (3, 5)), ("lost inf", 0.0, (4, 6))):
        bad = good.clone()
        bad[where] = val
        with pytest.raises(AssertionError):
            R.check_store(name, bad, ref, True)
    bad = good.clone()
    bad[0] = (ref[0] * 1.04).to(torch.float16)       # a small-gain row: 4 % of its own scale, nothing against 65504
    with pytest.raises(AssertionError):
        R.check_store("row scale", bad, ref, True)


def _part_a_cases(f16):
    for form in R.LINEAR_FORMS:
        yield f"linear/{form}", R.linear_case(form, f16).ref
    yield "conv 2x12x20 320->320", R.conv_case(f16, *R.CONV_SHAPE, amp=R.CONV_AMP).ref
    yield "conv 2x12x20 320->256", R.conv_case(f16, *R.CONV_SHAPE[:4], 256, amp=R.CONV_AMP).ref
    yield "conv 2x12x20 320->320 fused norm", R.conv_case(f16, *R.CONV_SHAPE, fused=True, amp=R.CONV_FUSED_AMP).ref
    yield "split-K 1x12x12 1280->128", R.conv_case(f16, *R.SPLITK_SHAPE, amp=R.SPLITK_AMP).ref
    for K in (320, 640):
        c = R.rowgemm_case(f16, K)
        yield f"rowgemm K{K} bias+residual", c.ref
        yield f"rowgemm K{K} bias", c.ref_bias
    yield "gn_apply", R.gn_apply_case(f16).ref
    yield "GEGLU", R.geglu_case(f16).ref
    for T in (160, 156):
        c = R.qkv_case(f16, T)
        yield f"QKV T{T} columns below the transposed section", c.ref[:, :2 * c.C]
        yield f"QKV T{T} transposed section", c.ref[:, 2 * c.C:]
    for K in (320, 640):
        yield f"rowgemm GEGLU K{K}", R.geglu_case(f16, M=416, K=K).ref
    c = R.qkv_case(f16, 416, B=1, C=320)
    yield "rowgemm QKV columns below the transposed section", c.ref[:, :2 * c.C]
    yield "rowgemm QKV transposed section", c.ref[:, 2 * c.C:]
    yield "head convolution's normalised patch", R.head_case(f16, False).h
    for M in (312, 416):
        yield f"cross-attention on the residual stream M{M}", R.xattn_case(f16, M).ref
    yield "cross-attention on the residual stream M416 C640", R.xattn_case(f16, 416, 640, 10).ref
    yield "conv sub-pixel", R.subpix_case(f16, *R.CONV_SHAPE).ref


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_part_a_input_conditions(f16):
    """Each case's float64 reference alone: at least 100 saturating elements of each sign, 100 eight-wide packs that hold both
    saturating and regular values, a quarter of the rows entirely regular, and a guard band of at most 2 % of the saturating
    elements."""
    for name, ref in _part_a_cases(f16):
        c = R.assert_case_conditions(name, ref)
        print(f"[range] {name} {BUILD_IDS[f16]}: {c}")
    # the column ladders (a folded LayerNorm takes every row to O(1); GroupNorm's gamma is per channel): checked transposed, the
    # kernels' eight-wide packs run down the columns of that layout
    cols = [(f"folded LayerNorm K{K}{' + GEGLU' if ge else ''}", R.ln_fold_operands(R.ln_fold_case(f16, ge, K=K))[3].t().contiguous())
            for ge, K in ((False, 320), (True, 320), (True, 640))]
    cols.append(("gn_slab", R.gn_slab_case(f16).ref_t))
    for name, ref in cols:
        c = R.assert_case_conditions(name, ref, packs_along_rows=True)
        print(f"[range] {name} {BUILD_IDS[f16]} (transposed): {c}")
    for K in (320, 640):      # neither factor of the GEGLU product comes near the limit
        c = R.ln_fold_case(f16, True, K=K)
        wp, gv, cv, _ = R.ln_fold_operands(c)
        assert float(R.folded_ln(c.x, c.st, wp, gv, cv).abs().max()) < 4096.0
    xc = R.xattn_case(f16, 416)
    assert float((xc.ref - xc.x.double()).abs().max()) < R.SAT_LO and float(xc.x.double().abs().max()) <= 64000.0, "only the add crosses the limit"
    assert float(R.xattn_geglu_case(f16).ref_hidden.abs().max()) < 64.0
    assert max(R.geglu_case(f16).factor_max, R.geglu_case(f16, M=416, K=320).factor_max, R.geglu_case(f16, M=416, K=640).factor_max) < 4096.0, \
        "neither GEGLU factor comes near the limit"
    assert R.case_conditions(R.head_case(f16, True).h)["pos"] >= 100      # (SiLU leaves nothing below -0.28)
    c = R.qkv_case(f16, 160)     # the 16-byte store packs eight TOKENS of one channel: mixed packs in that layout too
    vt = c.ref[:, 2 * c.C:].reshape(c.B, c.T, c.C).permute(0, 2, 1).reshape(c.B * c.C, c.T)
    assert R.case_conditions(vt)["mixed_packs"] >= 100


def test_row_statistics_of_the_stored_row():
    """ln_out is taken from the fp32 values before the pack.  How far does the store alone move a regular row's (mean, rstd)?
    fp16: under 1e-4 of the scale, so the GPU test holds ln_out to 2e-4 against the stored row as it stands.  bf16: more than 2e-4
    for the mean of the Linear case - no kernel could meet 2e-4 against the stored row there, so on that build the GPU test adds
    this movement, computed from the reference, to the bound."""
    moved = {}
    for f16 in BUILDS:
        for name, ref in [("linear/residual", R.linear_case("residual", f16).ref)] + [(f"rowgemm K{K}", R.rowgemm_case(f16, K).ref) for K in (320, 640)]:
            sat, guard, _, _ = R.classify(ref, True)
            rows = ~(sat | guard).any(dim=1)
            stat = lambda t: torch.stack([t.mean(-1), 1.0 / torch.sqrt(t.var(-1, unbiased=False) + 1e-5)], -1)   # noqa: E731
            exact, stored = stat(ref[rows]), stat(R.store16(ref, f16)[rows])
            for j in range(2):
                moved[f16, name, j] = float((exact[:, j] - stored[:, j]).abs().max() / stored[:, j].abs().max())
                print(f"[range] {name} {BUILD_IDS[f16]}: statistic {j} moved by the store: {moved[f16, name, j]:.3e} of the scale")
    assert max(v for (f16, _, _), v in moved.items() if f16) < 1e-4
    assert moved[False, "linear/residual", 0] > 2e-4


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("splits", [4, 8])
def test_splitk_partials_pass_the_limit_where_the_total_does_not(f16, splits):
    """The split-K case per K slice, in float64: the slices add up to the reference, and at least 100 regular totals have a partial
    sum at or beyond 65520 - a reduce kernel (or a GEMM) that clamped its fp32 partials would move those totals by more than the
    regular bound allows."""
    c = R.conv_case(f16, *R.SPLITK_SHAPE, amp=R.SPLITK_AMP)
    p = R.splitk_partials(c, splits)
    assert float((p.sum(0) + c.bias.double() - c.ref).abs().max()) < 1e-6
    reg = R.classify(c.ref, True)[2]
    clamped = p.clamp(-R.F16_MAX, R.F16_MAX).sum(0) + c.bias.double()
    scale = torch.where(reg, c.ref.abs(), torch.zeros_like(c.ref)).amax(dim=1, keepdim=True)
    caught = reg & ((clamped - c.ref).abs() > 1.5e-2 * scale)
    n = int((reg & (p.abs() >= R.F16_OVER).any(0)).sum())
    print(f"[range] split-K {BUILD_IDS[f16]} {splits} slices: {n} regular totals with a partial beyond the limit, {int(caught.sum())} of them past the bound if clamped")
    assert n >= 100 and int(caught.sum()) >= 100


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_residual_add_is_what_saturates(f16):
    c = R.linear_case("residual", f16)
    planted = (c.res.double().abs() > 59000.0).any(dim=1)
    assert int(planted.sum()) == 4
    prod = c.ref - c.res.double()
    sat = R.classify(c.ref, True)[0]
    assert R.classify(prod[planted], True)[2].all(), "the planted rows' products are regular"
    assert int(sat[planted].sum()) >= 50 and bool(R.classify(c.ref[planted], True)[2].any(dim=1).all())


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_part_c_positions(f16):
    """Variants 26 / 27: the planted rows' sums against max32 + F4_REF_BIAS lie on the stated side of the build's ``redo_thr``,
    every probability of a no-fallback case fits the P operand, and no other row comes near.  MG_OP_FLASH_ATTN512: the planted
    rows' excess over the first tile's maximum against FA5_THR."""
    thr = R.F4_REDO_THR[f16]
    for G in R.FLASH64_G:
        c = R.flash64_window_case(f16, G)
        l, pmax = R.fixed_ref_row_sums(c.q, c.k, 0.125, f16)
        other = torch.ones(c.T, dtype=torch.bool)
        other[list(c.rows)] = False
        assert float(l[other].max()) < thr / 1024.0, G
        fast = G <= 20 or not f16
        for r in c.rows:
            assert r // 256 == 1 and int(torch.argmax(R.scores_log2(c.q[r:r + 1], c.k, 0.125)[0])) >= c.T - 64
            assert (float(l[r]) < 0.75 * thr) == fast and (float(l[r]) >= 1.9 * thr) == (not fast), (G, float(l[r]))
        if fast:
            assert float(pmax.max()) < (65504.0 if f16 else 2.0 ** 127)
        if f16 and G == 20:
            assert abs(math.log2(float(l[list(c.rows)].max())) - 14.0) < 0.05
        if f16 and G == 26:
            assert float(pmax.max()) > 2.0 ** 19.9           # overflows the fp16 P operand before the row sum tells
    for G in R.FLASH512_G:
        c = R.flash512_window_case(f16, G)
        e = R.excess_over_first_tile(c.q, c.k, c.scale)
        other = torch.ones(c.T, dtype=torch.bool)
        other[list(c.rows)] = False
        assert float(e[other].max()) < 8.0
        for r in c.rows:
            assert abs(float(e[r]) - G) < 0.02 and (float(e[r]) > R.FA5_THR[f16]) == (f16 and G > 15.0), (G, float(e[r]))
    assert float(2.0 ** 15.5) < 65504.0 < float(2.0 ** 17)      # 15.5 still fits an fp16 probability, 17 would not


@pytest.mark.parametrize("T", [1024, 9216])
def test_part_d_emulated_ladder(T):
    """p = 2^(s - max32 - 6) rounded to fp16 (subnormals kept) in float64: under the suite's 1.5e-2 at every rung, the peak at
    G = 19.5 where the background rounds to 0 or 2^-24; a matrix unit that flushed subnormal inputs would miss the bound at the low
    rungs.  The bf16 build's probabilities have the exponent range and lose nothing."""
    worst = {}
    for G in R.SUBNORMAL_RUNGS:
        c = R.subnormal_case(True, G, T)
        scale = float(c.ref.abs().max())
        assert 0.9 < scale < 1.2
        first = c.rows < c.half
        assert len(c.rows) <= 1024 and int(first.sum()) >= 200
        if T > 1024:
            assert set(range(0, T, 256)) <= set(c.rows.tolist()) and set(range(255, T, 256)) <= set(c.rows.tolist())
        s = R.scores_log2(c.q[c.rows][first], c.k, 0.125)
        bg = torch.cat([s[:, :7], s[:, 8:]], dim=1)
        assert abs(float((s[:, 7:8] - bg).mean()) - G) < 0.05 and float(bg.amax(1).max() - bg.amin(1).min()) <= 1.01
        worst[G] = float((R.emulate_fixed_ref(c, True) - c.ref).abs().max())
        flushed = float((R.emulate_fixed_ref(c, True, flush_subnormals=True) - c.ref).abs().max())
        print(f"[range] subnormal ladder T={T} G={G}: emulated |err| {worst[G]:.3e}, with flushed subnormal inputs {flushed:.3e}")
        assert worst[G] <= 1.5e-2 * scale, (G, worst[G])
        if T == 9216 and G in (12.0, 16.0, 18.0):
            assert flushed > 2.0 * 1.5e-2 * scale
        cb = R.subnormal_case(False, G, T)
        assert float((R.emulate_fixed_ref(cb, False) - cb.ref).abs().max()) < 1e-3
    assert max(worst, key=worst.get) == 19.5
    if T == 9216:
        assert 1.0e-2 < worst[19.5] < 1.5e-2 < R.subnormal_ceiling(T, True) < 1.8e-2
    else:
        assert worst[19.5] < 2e-3
