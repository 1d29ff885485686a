"""Algorithmic work of one ``mg_op`` (FLOPs = 2 x MACs of the contraction; bytes = one read of
every input + one write of every output, weights counted once per launch) and the kernel class
it runs on.  bench.py turns per-op HIP-event timings into per-class achieved TFLOP/s / GB/s
against the gfx950 rooflines; DESIGN.md quotes the same formulas.
"""
from . import _lib as L, ops as O

MFMA_PEAK_TFLOPS = 2500.0   # bf16 dense, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0       # HBM3E spec (6.29 TB/s measured streaming)

CLASS = {
    L.OP_IGEMM: "igemm_mfma", L.OP_ROWGEMM: "rowgemm_mfma", L.OP_CONV3X3: "conv3x3_patch", L.OP_FLASH_ATTN64: "flash_attn64", L.OP_FLASH_ATTN512: "flash_attn512", L.OP_GN_STATS: "groupnorm",
    L.OP_GN_FINALIZE: "groupnorm", L.OP_GN_APPLY: "groupnorm", L.OP_GN_SLAB: "groupnorm",
    L.OP_SOFTMAX_ROWS: "softmax",
    L.OP_SCHED_STEP: "scheduler_step", L.OP_LINEAR_SMALL_M: "time_embedding",
    L.OP_LATENT_1X1: "boundary_conv", L.OP_POST_NCHW: "boundary_conv", L.OP_CONV3X3_HEAD: "boundary_conv", L.OP_IM2COL_SMALL: "boundary_conv", L.OP_ENS_DEPTH_STATS: "ensemble", L.OP_ENS_DEPTH_MEDIAN: "ensemble",
    L.OP_ENS_DEPTH_NORM: "ensemble", L.OP_ENS_NORMALS: "ensemble", L.OP_ENS_IID: "ensemble", L.OP_RESIZE: "resize", L.OP_COLORIZE: "resize", L.OP_IID_VIS: "resize", L.OP_RGB_PREP: "resize", L.OP_NORMALS_VIS: "resize", L.OP_RANDN: "noise", L.OP_MEMSET: "memops", L.OP_COPY: "memops",
}
BOUND = {"igemm_mfma": "mfma", "rowgemm_mfma": "mfma", "conv3x3_patch": "mfma", "flash_attn64": "mfma", "flash_attn512": "mfma"}   # everything else is HBM-bound streaming


def op_cost(op):
    """-> (class name, algorithmic FLOPs, algorithmic HBM bytes) of one launch."""
    k = op.kind
    cls = CLASS.get(k, "other")
    flops = byts = 0
    r = O.Raw(op) if k in L.FIELDS else None   # the fields as stored, by name
    if k == L.OP_IGEMM:
        v = O.igemm_view(op)
        B, H, W, Cin, N, taps, M, K, bz, cx, n_out = v.b, v.h, v.w, v.cin, v.n, v.taps, v.M, v.K, v.batch_z, v.cx, v.n_out
        flops = 2 * M * (v.n_alg or N) * (v.k_alg or K) * bz   # n_alg / k_alg: un-padded N / K of the boundary convs
        flops += 2 * M * N * cx                                # a folded 1x1 convolution: extra K, its input and weights read once
        osz = 4 if v.epi == L.EPI_F32 else 2   # bf16 for the plain, GEGLU and pair-softmax epilogues
        if taps == 4:   # sub-pixel up-sampling conv: the 4 parities share one input, each writes its own output pixels
            byts = B * H * W * Cin * 2 + bz * (N * K * 2 + M * n_out * osz)
        else:
            byts = bz * (B * H * W * Cin * 2 + N * K * 2 + M * n_out * osz)
        if v.epi == L.EPI_XATTN2:   # second stage: P [M][N] x W2 [c2][N] -> out [M][c2] (+ residual)
            c2 = v.c2
            flops += 2 * M * c2 * N
            byts = B * H * W * Cin * 2 + N * K * 2 + c2 * N * 2 + M * c2 * 2 + (M * c2 * 2 if v.has_residual else 0)
        elif v.has_residual:
            byts += bz * M * n_out * 2   # fused residual read
        byts += (M + N) * cx * 2
    elif k == L.OP_ROWGEMM:
        v = O.rowgemm_view(op)
        M, K, N, form = v.m, v.k, v.n, v.form
        flops = 2 * M * N * K
        byts = M * K * 2 + N * K * 2 + M * (N // 2 if form == L.RG_GEGLU else N) * 2 + (M * N * 2 if v.has_residual else 0)
        if form == L.RG_XATTN:   # + P [M][64] x VO^T [K][64]; x read once, out [M][K] written once
            flops += 2 * M * K * N
            byts = 2 * M * K * 2 + 2 * N * K * 2
        if v.has_xattn:   # the cross-attention prologue: scores + blend GEMMs, the updated rows written once
            flops += 2 * 2 * M * K * 64
            byts += M * K * 2 + 2 * 64 * K * 2
    elif k == L.OP_CONV3X3:
        v = O.conv3x3_view(op)
        B, H, W, N, Cin, par, T = v.b, v.h, v.w, v.n, v.cin, v.par, v.taps
        flops = 2 * B * H * W * N * T * Cin * par
        byts = B * H * W * Cin * 2 + par * (N * T * Cin * 2 + B * H * W * N * 2)
        if v.has_residual:
            byts += B * H * W * N * 2
    elif k == L.OP_CONV3X3_HEAD:
        flops = 2 * r.b * r.h * r.w * r.cout * 9 * r.c
        byts = r.b * r.h * r.w * (r.c * 2 + r.cout * 4)
    elif k == L.OP_FLASH_ATTN64:
        v = O.flash_attn64_view(op)
        B, heads, T = v.b, v.heads, v.ntok
        flops = 4 * B * heads * T * T * 64
        byts = 4 * B * heads * T * 64 * 2
    elif k == L.OP_FLASH_ATTN512:
        flops = 4 * r.b * r.ntok * r.ntok * 512
        byts = 4 * r.b * r.ntok * 512 * 2
    elif k == L.OP_GN_STATS:
        byts = r.b * r.hw * (r.c + (r.c1 if r.x1 else 0)) * 2
    elif k == L.OP_GN_APPLY:
        byts = 2 * r.b * r.hw * r.c * 2
    elif k == L.OP_GN_SLAB:
        byts = (2 if r.out else 1) * r.b * r.hw * r.c * 2
    elif k == L.OP_SOFTMAX_ROWS:
        byts = r.r * r.ncols * 4 + r.r * r.ldp * 2
    elif k == L.OP_SCHED_STEP:
        byts = (4 if r.noise else 3) * r.n * 4
    elif k == L.OP_LINEAR_SMALL_M:
        flops = 2 * r.m * r.n * r.k
        byts = r.n * r.k * 4
    elif k == L.OP_LATENT_1X1:
        byts = r.b * (r.ci + r.co) * r.hw * 4
    elif k == L.OP_IM2COL_SMALL:
        byts = r.b * r.h * r.w * ((r.c0 + r.c1) * 4 + r.kp * 2)
    elif k == L.OP_POST_NCHW:
        byts = r.b * r.hw * (r.ldi + (1 if r.post == L.POST_DEPTH else r.cout)) * 4
        if r.post == L.POST_SCHED:   # reads x_t (and the LCM noise) as well
            byts += r.b * r.hw * r.cout * 4 * (2 if r.noise else 1)
    elif k in (L.OP_ENS_DEPTH_STATS, L.OP_ENS_DEPTH_MEDIAN):
        byts = r.e * r.hw * 4
    elif k == L.OP_ENS_DEPTH_NORM:
        byts = 2 * r.hw * 4
    elif k == L.OP_ENS_NORMALS:
        byts = (r.e + 1) * 3 * r.hw * 4
    elif k == L.OP_ENS_IID:   # every member read once, the prediction (and the uncertainty) written once
        byts = (r.e + (2 if r.unc else 1)) * r.n * 4
    elif k == L.OP_IID_VIS:   # the fp32 planes read once (twice by the targets that take a maximum first), one byte written per element
        n3 = 3 * r.h * r.w
        byts = n3 * (5 * r.n + 4 * bin(r.linear_bits & r.up_to_scale_bits).count("1"))
    elif k == L.OP_RGB_PREP:   # one byte read per source element, one fp32 / 16-bit value written; two passes: the fp32 temporary once each way
        byts = 3 * (r.hin * r.win + r.hout * r.wout * (2 if r.out16 else 4))
        if r.mode != 2 and r.hin != r.hout and r.win != r.wout:
            byts += 2 * 3 * r.hin * r.wout * 4
    elif k == L.OP_NORMALS_VIS:
        byts = 3 * r.h * r.w * 5
    elif k == L.OP_RANDN:   # written once, nothing read
        byts = r.n * (2 if r.out16 else 4)
    elif k in (L.OP_MEMSET, L.OP_COPY):
        byts = r.bytes
    return cls, flops, byts


def summarize(ops, ms):
    """Aggregate per-op (cost, time) into {class: {launches, ms, flops, bytes, tflops, gbs}}."""
    out = {}
    for op, t in zip(ops, ms):
        cls, f, b = op_cost(op)
        d = out.setdefault(cls, dict(launches=0, ms=0.0, flops=0, bytes=0))
        d["launches"] += 1
        d["ms"] += float(t)
        d["flops"] += f
        d["bytes"] += b
    for d in out.values():
        s = max(d["ms"], 1e-9) * 1e-3
        d["tflops"] = d["flops"] / s / 1e12
        d["gbs"] = d["bytes"] / s / 1e9
    return out


def program_flops(ops):
    return sum(op_cost(op)[1] for op in ops)
