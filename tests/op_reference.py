"""Float64 reference of single ``mg_op`` launches (the op ABI of include/marigold_hip.h), for replaying a production program
op by op against the kernels.  A plain helper module for the tests.

Two stages:
  ``decode(op, resolve, label)``  field decoding only (runs on a CPU): the regions the op reads and writes (pointer, dtype,
                                  shape, strides) and its row sample.  ``resolve(ptr)`` -> (tensor, byte offset) | None.  A
                                  pointer the op reads that resolves to nothing is an error; a kind or flag combination this
                                  module has no reference for raises ``Unsupported(label, field)`` - never a silent pass.
  ``expected(spec, inputs)``      the arithmetic in float64 from the 16-bit operands as stored, on the inputs' device; returns
                                  {output name: (reference, index of the checked elements)}.

Forms covered: the launch forms of the AutoencoderKL encoder program - im2col_small; igemm with 1 / 9 taps, stride 1 / 2,
BF16 / F32 epilogues, bias, row vector, residual, the folded 1x1 shortcut, batching over z, the transposed section, explicit / automatic split-K;
gn_stats with the fused finalize; gn_finalize; gn_apply; conv3x3 with fused GroupNorm scale / shift + SiLU, residual and the
p[8] GroupNorm partial table; softmax_rows; post_nchw (POST_NONE).  Everything else raises Unsupported.

Sampling: GEMM-like ops check a sample of output rows, every column of each (``row_sample``): the first and last row of every
image, both sides of a strided subset of the 256-row tile boundaries, the last (ragged) tile, image-border pixels of 3x3 forms
and a seeded random remainder.  Reductions (GroupNorm scale / shift, the p[8] table) are checked in full.

Metrics (``metrics``): max|err| / max|ref| (bound 1.5e-2, the kernel suite's) and rmse / rms of the checked elements, bounded
per kind by ``RMS_BOUND``: 2x the worst value one MI355X run of tests/test_gpu_program_shadow.py measured (VAE encode 768^2,
bf16 operands): see the table there.
"""
import math
from dataclasses import dataclass, field

import torch

from marigold_amd import _lib as L, ops as O

MAX_REL_BOUND = 1.5e-2
# rmse / rms per kind: 2x the worst value measured on the MI355X (VAE encode 768^2, bf16 operands; measured value in brackets)
RMS_BOUND = {
    "im2col_small": 0.0,          # exact: a copy with one rounding to the operand type  [0]
    "igemm": 3.3e-3,              # [1.67e-3]
    "conv3x3": 3.3e-3,            # [1.67e-3]
    "conv3x3.gn_table": 2.7e-8,   # [1.37e-8]
    "gn_stats": 1.0e-6,           # [5.0e-7]
    "gn_finalize": 7.8e-8,        # [3.9e-8]
    "gn_apply": 3.3e-3,           # [1.68e-3]
    "softmax_rows": 3.3e-3,       # [1.66e-3]
    "post_nchw": 5.0e-8,          # [2.5e-8]
}
TILE = 256


class Unsupported(Exception):
    def __init__(self, label, what):
        super().__init__(f"{label}: no float64 reference for {what}")
        self.label, self.what = label, what


@dataclass
class Region:
    ptr: int
    dtype: torch.dtype
    shape: tuple
    strides: tuple

    def nbytes(self):
        esz = torch.empty((), dtype=self.dtype).element_size()
        return (sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + 1) * esz


@dataclass
class Spec:
    kind: int
    name: str
    label: str
    op: object
    reads: dict = field(default_factory=dict)
    writes: dict = field(default_factory=dict)
    rows: object = None     # output rows to check (torch.long), for GEMM-like ops


def view(resolve, r: Region):
    """The tensor of region ``r`` as the device holds it (a view, no copy)."""
    hit = resolve(r.ptr)
    if hit is None:
        raise KeyError(f"pointer {r.ptr:#x} resolves to no held tensor")
    base, off = hit
    esz = torch.empty((), dtype=r.dtype).element_size()
    flat = base.reshape(-1).view(torch.uint8)
    n = r.nbytes()
    assert off % esz == 0 and off + n <= flat.numel(), (hex(r.ptr), off, n, flat.numel())
    return flat[off:off + n].view(r.dtype).as_strided(r.shape, r.strides)


def make_resolver(tensors):
    """resolve(ptr) over a list of tensors (the program's held tensors, weight cache, pool)."""
    spans = []
    seen = set()

    def add(t):
        if isinstance(t, torch.Tensor):
            if t.numel() and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), t))
        elif isinstance(t, (list, tuple)):
            for u in t:
                add(u)
        elif isinstance(t, dict):
            for u in t.values():
                add(u)
    add(tensors)
    spans.sort(key=lambda s: s[0])

    def resolve(ptr):
        best = None
        for lo, hi, t in spans:
            if lo <= ptr < hi and (best is None or hi - lo > best[1] - best[0]):
                best = (lo, hi, t)
        return None if best is None else (best[2], ptr - best[0])
    return resolve


def row_sample(M, rows_per_img, *, Wimg=0, Himg=0, n_random=384, seed=0):
    """Rows of an [M] output to check (see the module docstring)."""
    s = set()
    n_img = max(1, M // max(1, rows_per_img))
    for b in range(n_img):
        s.update((b * rows_per_img, min(M, (b + 1) * rows_per_img) - 1))
        if Wimg and Himg:   # image-border pixels of a 3x3 form: strided along each edge
            base = b * rows_per_img
            for x in range(0, Wimg, max(1, Wimg // 24)):
                s.update((base + x, base + (Himg - 1) * Wimg + x))
            for y in range(0, Himg, max(1, Himg // 24)):
                s.update((base + y * Wimg, base + y * Wimg + Wimg - 1))
    nt = (M + TILE - 1) // TILE
    for t in range(1, nt, max(1, nt // 16)):
        s.update((t * TILE - 1, t * TILE))
    s.update(range((nt - 1) * TILE, M))
    g = torch.Generator().manual_seed(seed)
    s.update(torch.randint(0, M, (min(n_random, M),), generator=g).tolist())
    return torch.tensor(sorted(r for r in s if 0 <= r < M), dtype=torch.long)


def _op16(f16):
    return torch.float16 if f16 else torch.bfloat16


def decode(op, resolve, label="", f16=False):
    """One mg_op -> Spec (regions read / written, sample).  Raises Unsupported for forms without a reference."""
    k, r = op.kind, O.Raw(op)
    o16 = _op16(f16)
    name = L.OP_NAMES.get(k, str(k))
    sp = Spec(k, name, label, op)
    R = lambda ptr, dt, shape, strides: Region(ptr, dt, tuple(shape), tuple(strides))
    if k == L.OP_IM2COL_SMALL:
        B, H, W, C0, Kp = r.b, r.h, r.w, r.c0, r.kp
        if r.c1 or r.src1 or r.src0_broadcast:
            raise Unsupported(label, "im2col_small with a second source / broadcast")
        sp.reads["src0"] = R(r.src0, torch.float32, (B, C0, H, W), (C0 * H * W, H * W, W, 1))
        sp.writes["out"] = R(r.out, o16, (B * H * W, Kp), (Kp, 1))
        sp.rows = row_sample(B * H * W, H * W, Wimg=W, Himg=H)
    elif k == L.OP_IGEMM:
        v = O.igemm_view(op)
        for has, what in ((v.has_a1, "a second channel source"), (v.has_ln_out, "row statistics"), (v.has_ln_in, "folded LayerNorm")):
            if has:
                raise Unsupported(label, what)
        epi = v.epi
        if epi not in (L.EPI_BF16, L.EPI_F32):
            raise Unsupported(label, f"igemm epilogue {epi}")
        if v.hu or v.wu:
            raise Unsupported(label, "igemm on a virtual up-sampled input")
        if v.trans_perm:
            raise Unsupported(label, "igemm permuted transposed section")
        B, H, W, Cin, Ho, Wo, N, taps, stride, pad = v.b, v.h, v.w, v.cin, v.ho, v.wo, v.n, v.taps, v.stride, v.pad
        if taps not in (1, 9):
            raise Unsupported(label, f"igemm taps {taps}")
        bz, Cx, Cx0, tf, M = v.batch_z, v.cx, v.cx0, v.trans_from, v.M
        if v.has_fold and (taps != 9 or stride != 1 or pad != 1 or bz != 1):
            raise Unsupported(label, "a folded shortcut outside the 3x3 / stride 1 form")
        ncols = tf if v.has_trans else N
        odt = torch.float32 if epi == L.EPI_F32 else o16
        sp.reads["A"] = R(v.a, o16, (bz, B * H * W, Cin), (v.sa, v.lda, 1))
        sp.reads["Wt"] = R(v.wt, o16, (bz, N, v.Kx), (v.sw, v.ldw, 1))
        if v.has_fold:   # the 1x1 shortcut of a second tensor as extra K: X0 channels [0, Cx0), X1 [Cx0, Cx)
            sp.reads["X0"] = R(v.x0, o16, (B * H * W, Cx0), (v.ldx0, 1))
            if v.has_x1:
                sp.reads["X1"] = R(v.x1, o16, (B * H * W, Cx - Cx0), (v.ldx1, 1))
            elif Cx != v.raw.cx0:
                raise Unsupported(label, "a folded shortcut without its second source")
        if v.bias:
            sp.reads["bias"] = R(v.bias, torch.float32, (N,), (1,))
        if v.has_rowvec:
            sp.reads["rowvec"] = R(v.rowvec, torch.float32, (B, N), (0 if v.rowvec_bcast else N, 1))
        if v.has_residual:
            sp.reads["residual"] = R(v.residual, o16, (bz, M, ncols), (v.sr, v.ldr, 1))
        sp.writes["out"] = R(v.out, odt, (bz, M, ncols), (v.so, v.ldo, 1))
        if v.has_trans:
            sp.writes["out2"] = R(v.out2, o16, (B, N - tf, v.ldt), ((N - tf) * v.ldt, v.ldt, 1))
            if bz != 1:
                raise Unsupported(label, "igemm transposed section with batching")
        sp.rows = row_sample(M, Ho * Wo, Wimg=Wo if taps == 9 else 0, Himg=Ho if taps == 9 else 0)
        sp.n_check = v.n_alg or N
    elif k == L.OP_GN_STATS:
        B, HW, C = r.b, r.hw, r.c
        if not r.ss:
            raise Unsupported(label, "gn_stats without the fused finalize")
        if (r.ctot and r.ctot != C) or r.coff or r.x1 or r.c1:
            raise Unsupported(label, "gn_stats of a channel window / second source")
        sp.reads["x"] = R(r.x, o16, (B, HW, C), (HW * C, C, 1))
        sp.reads["gamma"] = R(r.gamma, torch.float32, (C,), (1,))
        sp.reads["beta"] = R(r.beta, torch.float32, (C,), (1,))
        sp.writes["ss"] = R(r.ss, torch.float32, (B, 2, C), (2 * C, C, 1))
    elif k == L.OP_GN_FINALIZE:
        B, C, groups, slots = r.b, r.c, r.groups, r.slots
        sp.reads["partials"] = R(r.partials, torch.float32, (B, slots, groups, 2), (slots * groups * 2, groups * 2, 2, 1))
        sp.reads["gamma"] = R(r.gamma, torch.float32, (C,), (1,))
        sp.reads["beta"] = R(r.beta, torch.float32, (C,), (1,))
        sp.writes["ss"] = R(r.ss, torch.float32, (B, 2, C), (2 * C, C, 1))
    elif k == L.OP_GN_APPLY:
        B, HW, C = r.b, r.hw, r.c
        if r.x1:
            raise Unsupported(label, "gn_apply with a second source")
        sp.reads["x"] = R(r.x, o16, (B, HW, C), (HW * C, C, 1))
        sp.reads["ss"] = R(r.ss, torch.float32, (B, 2, C), (2 * C, C, 1))
        sp.writes["out"] = R(r.out, o16, (B, HW, C), (HW * C, C, 1))
    elif k == L.OP_CONV3X3:
        v = O.conv3x3_view(op)
        B, H, W, C0, N = v.b, v.h, v.w, v.c0, v.n
        if v.subpix or v.c1 or v.has_a1:
            raise Unsupported(label, "conv3x3 sub-pixel / second source")
        M = B * H * W
        sp.reads["A"] = R(v.a0, o16, (M, C0), (v.lda0, 1))
        sp.reads["Wt"] = R(v.wt, o16, (N, 9 * C0), (v.ldw, 1))
        if v.bias:
            sp.reads["bias"] = R(v.bias, torch.float32, (N,), (1,))
        if v.has_rowvec:
            sp.reads["rowvec"] = R(v.rowvec, torch.float32, (B, N), (0 if v.rowvec_bcast else N, 1))
        if v.has_residual:
            sp.reads["residual"] = R(v.residual, o16, (M, N), (v.ldr, 1))
        if v.has_ss:
            sp.reads["ss"] = R(v.ss, torch.float32, (B, 2, C0), (2 * C0, C0, 1))
        sp.writes["out"] = R(v.out, o16, (M, N), (v.ldo, 1))
        if v.has_gn_part:
            ng = N // v.gn_cpg
            sp.writes["gn_table"] = R(v.gn_part, torch.float32, (B, v.gn_slots, ng, 2), (v.gn_slots * ng * 2, ng * 2, 2, 1))
        sp.rows = row_sample(M, H * W, Wimg=W, Himg=H)
    elif k == L.OP_SOFTMAX_ROWS:
        Rn, ncols, lds, ldp = r.r, r.ncols, r.lds, r.ldp
        sp.reads["S"] = R(r.scores, torch.float32, (Rn, ncols), (lds, 1))
        sp.writes["P"] = R(r.probs, o16, (Rn, ldp), (ldp, 1))
        sp.rows = row_sample(Rn, Rn)
    elif k == L.OP_POST_NCHW:
        B, HW, Cout, ldi = r.b, r.hw, r.cout, r.ldi
        if r.post != L.POST_NONE:
            raise Unsupported(label, f"post_nchw mode {r.post}")
        sp.reads["in"] = R(r.x, torch.float32, (B, HW, Cout), (HW * ldi, ldi, 1))
        sp.writes["out"] = R(r.out, torch.float32, (B, Cout, HW), (Cout * HW, HW, 1))
    else:
        raise Unsupported(label, f"op kind {name}")
    for nm, reg in sp.reads.items():   # every pointer the op reads must resolve
        if resolve(reg.ptr) is None:
            raise KeyError(f"{label}: {nm} pointer {reg.ptr:#x} resolves to no held tensor")
    return sp


def load_inputs(spec, resolve):
    """Clones (on the device) of every region the op reads - taken BEFORE the op runs (some write in place)."""
    return {nm: view(resolve, r).clone() for nm, r in spec.reads.items()}


def read_outputs(spec, resolve):
    return {nm: view(resolve, r) for nm, r in spec.writes.items()}


def _taps_gather(A, rows, B, H, W, Ho, Wo, stride, pad, taps):
    """[len(rows)][taps * C] float64 operand rows of an implicit GEMM (zero outside the image)."""
    C = A.shape[-1]
    A3 = A.reshape(B, H, W, C)
    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    yo, xo = rem // Wo, rem % Wo
    if taps == 1:
        return A3[b, yo * stride, xo * stride].double()
    cols = []
    for ky in range(3):
        for kx in range(3):
            y, x = yo * stride - pad + ky, xo * stride - pad + kx
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            v = A3[b, y.clamp(0, H - 1), x.clamp(0, W - 1)].double()
            cols.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    return torch.cat(cols, dim=1)


def expected(spec, inputs, f16=False):
    """{output: (float64 reference, index)}: index = rows (GEMM-like) or None (whole region)."""
    op, k, r = spec.op, spec.kind, O.Raw(spec.op)
    o16 = _op16(f16)
    dev = next(iter(inputs.values())).device
    if k == L.OP_IM2COL_SMALL:
        B, H, W, C0, Kp = r.b, r.h, r.w, r.c0, r.kp
        x = inputs["src0"].double().permute(0, 2, 3, 1).reshape(B * H * W, C0)
        rows = spec.rows.to(dev)
        g = _taps_gather(x, rows, B, H, W, H, W, 1, 1, 9)
        ref = torch.zeros(len(rows), Kp, dtype=torch.float64, device=dev)
        ref[:, :9 * C0] = g.to(o16).double()
        return {"out": (ref, rows)}
    if k == L.OP_IGEMM:
        v = O.igemm_view(op)
        B, H, W, Ho, Wo, N, taps, stride, pad, tf = v.b, v.h, v.w, v.ho, v.wo, v.n, v.taps, v.stride, v.pad, v.trans_from
        rows = spec.rows.to(dev)
        scale = v.scale or 1.0
        res = {}
        bz = inputs["A"].shape[0]
        refs = []
        for z in range(bz):
            a = _taps_gather(inputs["A"][z], rows, B, H, W, Ho, Wo, stride, pad, taps)
            if "X0" in inputs:
                a = torch.cat([a, inputs["X0"][rows].double()] + ([inputs["X1"][rows].double()] if "X1" in inputs else []), 1)
            acc = a @ inputs["Wt"][z].double().t() * scale
            if "bias" in inputs:
                acc = acc + inputs["bias"].double()
            if "rowvec" in inputs:
                acc = acc + inputs["rowvec"].double()[rows // (Ho * Wo)]
            if "residual" in inputs:
                acc = acc + torch.cat([inputs["residual"][z][rows].double(),
                                       torch.zeros(len(rows), acc.shape[1] - inputs["residual"].shape[-1], dtype=torch.float64,
                                                   device=dev)], 1)
            refs.append(acc)
        acc = torch.stack(refs)                        # [bz][rows][N]
        ncheck = getattr(spec, "n_check", N)
        if tf >= 0:
            res["out"] = (acc[:, :, :min(tf, ncheck)], rows)
            b, t = rows // (Ho * Wo), rows % (Ho * Wo)
            res["out2"] = (acc[0, :, tf:], (b, t))     # out2[b][n - tf][t]
        else:
            res["out"] = (acc[:, :, :ncheck], rows)
        return res
    if k == L.OP_GN_STATS or k == L.OP_GN_FINALIZE:
        eps = r.eps
        gamma, beta = inputs["gamma"].double(), inputs["beta"].double()
        if k == L.OP_GN_STATS:
            B, HW, C, groups = r.b, r.hw, r.c, r.groups
            x = inputs["x"].double().reshape(B, HW, groups, C // groups)
            mean = x.mean(dim=(1, 3))
            var = x.var(dim=(1, 3), unbiased=False)
        else:
            B, C, groups, HW = r.b, r.c, r.groups, r.hw
            part = inputs["partials"].double().sum(1)     # [B][groups][2] = (sum, sum of squares)
            n = HW * (C // groups)
            mean = part[..., 0] / n
            var = (part[..., 1] / n - mean ** 2).clamp_min(0)
        rstd = (var + eps).rsqrt()
        cpg = C // groups
        sc = rstd.repeat_interleave(cpg, 1) * gamma
        sh = beta - mean.repeat_interleave(cpg, 1) * sc
        return {"ss": (torch.stack([sc, sh], 1), None)}
    if k == L.OP_GN_APPLY:
        x, ss = inputs["x"].double(), inputs["ss"].double()
        y = x * ss[:, 0:1, :] + ss[:, 1:2, :]
        if r.silu:
            y = y * torch.sigmoid(y)
        return {"out": (y, None)}
    if k == L.OP_CONV3X3:
        v = O.conv3x3_view(op)
        B, H, W, silu = v.b, v.h, v.w, v.silu
        rows = spec.rows.to(dev)
        A = inputs["A"]
        if "ss" in inputs:   # the fused norm: silu?(x * scale + shift), rounded to the operand type as staged; padding stays 0
            ss = inputs["ss"].double()
            img = torch.arange(B * H * W, device=dev) // (H * W)
            y = A.double() * ss[img, 0] + ss[img, 1]
            if silu:
                y = y * torch.sigmoid(y)
            A = y.to(o16)
        a = _taps_gather(A, rows, B, H, W, H, W, 1, 1, 9)
        acc = a @ inputs["Wt"].double().t()
        if "bias" in inputs:
            acc = acc + inputs["bias"].double()
        if "rowvec" in inputs:
            acc = acc + inputs["rowvec"].double()[rows // (H * W)]
        if "residual" in inputs:
            acc = acc + inputs["residual"][rows].double()
        return {"out": (acc, rows)}
    if k == L.OP_SOFTMAX_ROWS:
        rows = spec.rows.to(dev)
        ldp = r.ldp
        s = inputs["S"][rows].double()
        ref = torch.zeros(len(rows), ldp, dtype=torch.float64, device=dev)
        ref[:, :s.shape[1]] = torch.softmax(s, dim=-1)
        return {"P": (ref, rows)}
    if k == L.OP_POST_NCHW:
        return {"out": (inputs["in"].double().permute(0, 2, 1) * r.scale, None)}
    raise Unsupported(spec.label, f"op kind {spec.name}")


def gn_table_reference(spec, out):
    """The conv3x3 ``gn_part`` table summed over its slots, from the output as stored: [B][groups][2] (sum, sum of squares)."""
    v = O.conv3x3_view(spec.op)
    B, H, W, N, cpg = v.b, v.h, v.w, v.n, v.gn_cpg
    y = out.double().reshape(B, H * W, N // cpg, cpg)
    return torch.stack([y.sum(dim=(1, 3)), (y * y).sum(dim=(1, 3))], -1)


def pick(got, index):
    """The checked elements of an output region."""
    if index is None:
        return got
    if isinstance(index, tuple):        # transposed section: out2[b][:, t]
        b, t = index
        return got[b, :, t]
    if got.dim() == 3:                  # [bz][M][N]
        return got[:, index]
    return got[index]


def metrics(got, ref):
    """(max|err| / max|ref|, rmse / rms) of the checked elements, in float64."""
    got, ref = got.double(), ref.double().to(got.device)
    if got.shape != ref.shape:
        got = got[..., :ref.shape[-1]]
    err = got - ref
    scale = max(float(ref.abs().max()), 1e-30)
    rms = max(float(ref.pow(2).mean().sqrt()), 1e-30)
    mx = float(err.abs().max())
    rm = float(err.pow(2).mean().sqrt())
    if not (math.isfinite(mx) and math.isfinite(rm)):
        return float("inf"), float("inf")
    return mx / scale, rm / rms


def check_op(spec, inputs, outputs, f16=False):
    """[(name, kind key, max_rel, rms_rel)] of one op; the caller asserts the bounds."""
    res = []
    for nm, (ref, idx) in expected(spec, inputs, f16).items():
        got = pick(outputs[nm], idx)     # (out2: [rows][N - tf], like its reference)
        res.append((nm, spec.name, *metrics(got, ref)))
    if "gn_table" in outputs:
        ref = gn_table_reference(spec, outputs["out"])
        got = outputs["gn_table"].double().sum(1)
        res.append(("gn_table", "conv3x3.gn_table", *metrics(got, ref)))
    return res
