"""Op descriptors for libmarigold_hip (one ``mg_op`` per kernel launch) and ``OpSeq``, the
host-side container that turns a list of them into a native program (``mg_program_*``).

torch is used only as the owner of device memory and the source of the HIP stream handle.
Field layout of every op is documented in include/marigold_hip.h.  Every kind is built and read by field NAME (the header's
enumerators, mirrored in _lib.FIELDS): ``build_op`` makes an op from its fields, ``Raw`` is an op's fields as stored.  For the four
kinds with many launch forms (MG_OP_IGEMM, MG_OP_CONV3X3, MG_OP_ROWGEMM, MG_OP_FLASH_ATTN64) ``igemm_view`` / ``conv3x3_view`` /
``rowgemm_view`` / ``flash_attn64_view`` are the op decoded the way its launcher decodes it.  The launchers' defaulting rules are
restated in those views and nowhere else in Python.
"""
import ctypes

import torch

from . import _lib as L
from ._lib import MgOp


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    return int(x)


# --------------------------------------------------------------------------- named fields

_TO_SLOT = dict(i=int, f=float, p=_ptr, l=int)
_WHERE = {kind: {name: (arr, k) for arr, names in tab.items() for k, name in enumerate(names)} for kind, (_, tab) in L.FIELDS.items()}
assert all(len(w) == sum(len(names) for names in L.FIELDS[kind][1].values()) for kind, w in _WHERE.items()), "a field name is used twice"


class Raw:
    """The fields of an op by name, as stored: ``Raw(op).ldw`` reads and writes an MG_OP_IGEMM's MG_IGEMM_I_LDW slot."""

    def __init__(self, op):
        object.__setattr__(self, "op", op)
        object.__setattr__(self, "_where", _WHERE[op.kind])

    def __getattr__(self, name):
        if name not in self._where:
            raise AttributeError(f"{L.OP_NAMES[self.op.kind]} has no field {name!r}")
        arr, k = self._where[name]
        return getattr(self.op, arr)[k] or 0   # (a NULL pointer reads as 0, not None)

    def __setattr__(self, name, value):
        arr, k = self._where[name]
        getattr(self.op, arr)[k] = _TO_SLOT[arr](value)


def build_op(kind, **fields):
    """An op from its fields by name; what is not named stays zero / NULL."""
    op = MgOp()
    op.kind = kind
    raw = Raw(op)
    for name, value in fields.items():
        setattr(raw, name, value)
    return op


class View:
    """An op decoded once.  ``raw``: its fields as stored (writable).  The attributes set by the ``*_view`` function: what the
    launcher works with after its defaulting rules; every other field name reads through to ``raw``."""

    def __init__(self, op):
        self.op, self.raw = op, Raw(op)

    def __getattr__(self, name):
        return getattr(self.raw, name)


def igemm_view(op):
    """MG_OP_IGEMM as csrc/igemm2.hip::mg_launch_igemm2 decodes it.  ``M`` rows; ``K`` = taps * Cin, ``Kx`` = K + the folded
    shortcut's ``cx`` channels (``cx0`` of them in X0); ``c0`` = the channels A holds; row strides with their defaults (``ldo`` has
    none in the launcher: ``igemm()`` fills it in); ``n_out`` = columns stored (GEGLU: N / 2); ``fits_31bit``: the operands are
    within the hand-placed tiles' (72 / 73) 31-bit byte offsets."""
    v = View(op)
    r = v.raw
    v.has_residual, v.has_ln_out, v.has_ln_in, v.has_a1, v.has_rowvec, v.has_fold, v.has_x1 = (
        bool(x) for x in (r.residual, r.ln_out, r.ln_in, r.a1, r.rowvec, r.x0, r.x1))
    v.has_trans = r.trans_from >= 0
    v.M = r.b * r.ho * r.wo
    v.batch_z = max(1, r.batch_z)
    v.cx = r.cx if v.has_fold else 0
    v.cx0 = r.cx0 if v.has_x1 else v.cx
    v.K = r.taps * r.cin
    v.Kx = v.K + v.cx
    v.c0 = r.c0 if v.has_a1 else r.cin
    v.lda = r.lda if r.lda > 0 else v.c0
    v.lda1 = (r.lda1 if r.lda1 > 0 else r.cin - v.c0) if v.has_a1 else 0
    v.ldw = r.ldw if r.ldw > 0 else v.Kx
    v.ldr = r.ldr if r.ldr > 0 else r.n
    v.ldx0 = r.ldx0 if r.ldx0 > 0 else v.cx0
    v.ldx1 = (r.ldx1 if r.ldx1 > 0 else v.cx - v.cx0) if v.has_x1 else 0
    v.n_out = r.n // 2 if r.epi == L.EPI_GEGLU else r.n
    v.fits_31bit = r.b * r.h * r.w * max(v.lda, v.lda1, v.ldx0, v.ldx1) < (1 << 30) and r.n * v.ldw < (1 << 30)
    return v


def conv3x3_view(op):
    """MG_OP_CONV3X3 as csrc/conv_patch.hip::conv3x3_decode decodes it: ``cin`` = C0 + C1, ``taps`` (4 in sub-pixel mode: ``par`` = 4
    output parities; else 9), dense row strides where the op leaves them 0."""
    v = View(op)
    r = v.raw
    v.has_residual, v.has_a1, v.has_ss, v.has_rowvec, v.has_gn_part = (bool(x) for x in (r.residual, r.a1, r.ss, r.rowvec, r.gn_part))
    v.cin = r.c0 + r.c1
    v.taps, v.par = (4, 4) if r.subpix else (9, 1)
    v.lda0 = r.lda0 if r.lda0 > 0 else r.c0
    v.lda1 = r.lda1 if r.lda1 > 0 else r.c1
    v.ldo = r.ldo if r.ldo > 0 else r.n
    v.ldr = r.ldr if r.ldr > 0 else r.n
    v.ldw = r.ldw if r.ldw > 0 else v.taps * v.cin
    return v


def rowgemm_view(op):
    """MG_OP_ROWGEMM as csrc/rowgemm.hip::mg_launch_rowgemm decodes it: ``n_out`` = columns stored (GEGLU: N / 2; the
    cross-attention form writes K), dense row strides where the op leaves them 0, ``has_xattn``: the cross-attention prologue."""
    v = View(op)
    r = v.raw
    v.has_residual, v.has_ln_in, v.has_ln_out, v.has_gn_ss = (bool(x) for x in (r.residual, r.ln_in, r.ln_out, r.gn_ss))
    v.has_xattn = r.form == L.RG_GEGLU and bool(r.xattn)
    v.n_out = {L.RG_GEGLU: r.n // 2, L.RG_XATTN: r.k}.get(r.form, r.n)
    v.ldx = r.ldx if r.ldx > 0 else r.k
    v.ldo = r.ldo if r.ldo > 0 else v.n_out
    v.ldr = r.ldr if r.ldr > 0 else r.n
    v.waves = r.waves if r.waves > 0 else (8 if r.k == 640 else 12)
    return v


def flash_attn64_view(op):
    """MG_OP_FLASH_ATTN64: no defaulting rules - every field as stored; ``ws_bytes`` of the workspace."""
    v = View(op)
    v.ws_bytes = v.raw.ws_kb * 1024
    return v


def igemm_tickets(op):
    """Device address of the caller's row-block tickets of an MG_OP_IGEMM (its ``tickets_lo`` / ``tickets_hi`` halves); 0 = the library's."""
    r = Raw(op)
    return (r.tickets_lo & 0xffffffff) | ((r.tickets_hi & 0xffffffff) << 32)


def set_igemm_tickets(op, addr):
    """Store the ticket buffer's address (tensor / int; None or 0 clears it) as two int32 halves."""
    addr = _ptr(addr) or 0
    r = Raw(op)
    r.tickets_lo, r.tickets_hi = (h - (1 << 32) if h >= 1 << 31 else h for h in (addr & 0xffffffff, (addr >> 32) & 0xffffffff))


def current_stream_handle():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------- builders

def igemm(a, w, out, *, B, H, W, Cin, Ho, Wo, N, taps=1, stride=1, pad=0, up=None, bias=None,
          rowvec=None, residual=None, epi=L.EPI_BF16, ldo=None, out2=None, trans_from=-1, ldt=0,
          batch_z=1, ldr=0, lda=0, ldw=0, zstrides=(0, 0, 0, 0), scale=1.0, variant=0,
          rowvec_bcast=False, n_alg=0, k_alg=0, a1=None, C0=0, lda1=0, ln_out=None, ln_in=None, ln_g=None, ln_c=None,
          ln_eps=1e-5, sm_scale=0.0, sm_cols=0, c2=0, trans_perm=False, ln_counters=None, splits=0, fold=None):
    """``fold`` = (x0, x1 | None, Cx0, Cx[, ldx0, ldx1]): a 1x1 convolution of a second tensor (the ResNet block's conv_shortcut)
    as extra K of this 3x3 convolution; ``w`` rows are then [conv weights | shortcut weights]."""
    hu, wu = up if up else (0, 0)
    if ldo is None:
        ldo = N // 2 if epi == L.EPI_GEGLU else N
    op = build_op(L.OP_IGEMM, b=B, h=H, w=W, cin=Cin, ho=Ho, wo=Wo, n=N, taps=taps, stride=stride, pad=pad, hu=hu, wu=wu, epi=epi, ldo=ldo,
                  trans_from=trans_from, batch_z=batch_z, ldr=ldr, lda=lda, ldt=ldt, variant=variant, ldw=ldw, rowvec_bcast=rowvec_bcast,
                  n_alg=n_alg, k_alg=k_alg, c0=C0, lda1=lda1, trans_perm=trans_perm, sm_cols=sm_cols, c2=c2, splits=splits,
                  scale=scale, ln_eps=ln_eps, sm_scale=sm_scale, a=a, wt=w, out=out, bias=bias, rowvec=rowvec, residual=residual,
                  out2=out2, a1=a1, ln_out=ln_out, ln_in=ln_in, ln_g=ln_g, ln_c=ln_c, **dict(zip(("sa", "sw", "so", "sr"), zstrides)))
    set_igemm_tickets(op, ln_counters)   # the program's own row-block tickets
    if fold:
        r = Raw(op)
        r.x0, r.x1, r.cx0, r.cx = fold[:4]
        r.ldx0, r.ldx1 = (tuple(fold[4:6]) + (0, 0))[:2]
    return op


def conv3x3(a0, w, out, *, B, H, W, C0, N, a1=None, C1=0, subpix=False, ss=None, silu=False, bias=None, rowvec=None,
            residual=None, lda0=0, lda1=0, ldo=0, ldr=0, ldw=0, rowvec_bcast=False, variant=0, wz=0, gn_part=None, gn_cpg=0,
            gn_slots=0):
    """Patch-resident conv3x3 / pad 1 (MG_OP_CONV3X3): fused GroupNorm scale/shift (+SiLU) on the input, second
    channel source, sub-pixel 2x up-sampling; ``gn_part``: the output's GroupNorm partial sums as a by-product
    (``conv3x3_gn_slots`` tells whether / how many slots per image)."""
    return build_op(L.OP_CONV3X3, b=B, h=H, w=W, c0=C0, c1=C1, n=N, subpix=subpix, silu=silu, lda0=lda0, lda1=lda1, ldo=ldo, ldr=ldr,
                    ldw=ldw, rowvec_bcast=rowvec_bcast, variant=variant, gn_cpg=gn_cpg, gn_slots=gn_slots, a0=a0, wt=w, out=out, bias=bias,
                    rowvec=rowvec, residual=residual, a1=a1, ss=ss, gn_part=gn_part, sw=wz)


def conv3x3_gn_slots(op, f16=False):
    """Partial-table slots per image this MG_OP_CONV3X3 fills with its output's GroupNorm statistics (0: its tile does not);
    ``f16``: asked of the fp16-operand build (its tile choice differs where a kernel is bf16-only)."""
    return int(L.load(f16).mg_conv3x3_gn_slots(ctypes.byref(op)))


def rowgemm(x, wp, out, *, M, K, N, form=L.RG_BF16, ldx=0, ldo=0, ldr=0, residual=None, ln_in=None, ln_out=None, vt=None,
            gn_ss=None, tokens=0, ldt=0, trans_from=0, waves=0, ln_eps=1e-5, sm_cols=0, sm_scale=0.0, dbg=None, nsplit=0,
            xattn=None, xout=None):
    """Row-resident GEMM (MG_OP_ROWGEMM): ``wp`` from weights.pack_rowgemm (form RG_XATTN: pack_rowgemm_xattn).  ``xattn`` (GEGLU
    form, K = 320, no column split): a pack_rowgemm_xattn image - the collapsed cross-attention runs on the rows in registers before
    the projection (``ln_in`` = the statistics of the rows as loaded, ``xout`` = where the updated rows go, ``sm_cols`` / ``sm_scale``)."""
    return build_op(L.OP_ROWGEMM, m=M, k=K, n=N, ldx=ldx, ldo=ldo, ldr=ldr, form=form, tokens=tokens, ldt=ldt, trans_from=trans_from,
                    waves=waves, sm_cols=sm_cols, nsplit=nsplit, ln_eps=ln_eps, sm_scale=sm_scale, x=x, wp=wp, out=out, residual=residual,
                    ln_in=ln_in, ln_out=ln_out, vt=vt, gn_ss=gn_ss, dbg=dbg, xattn=xattn, xout=xout if xattn is not None else None)


def linear(x, w, out, *, M, K, N, **kw):
    """out[M][N] = x[M][K] @ w[N][K]^T (+ fused epilogue)."""
    return igemm(x, w, out, B=1, H=M, W=1, Cin=K, Ho=M, Wo=1, N=N, taps=1, **kw)


def gn_stats(x, partials, *, B, HW, C, chunks, groups, Ctot=0, coff=0, slot0=0, slots=0, gamma=None, beta=None, ss=None,
             counters=None, eps=0.0, x1=None, C1=0):
    """Partials [B][slots][groups][2]; with ``ss`` the image's last-arriving block also finalizes (MG_OP_GN_STATS).  ``x1``
    ([B][HW][C1]): the concat's second source in the same launch (slots slot0 + chunks ...)."""
    return build_op(L.OP_GN_STATS, b=B, hw=HW, c=C, chunks=chunks, ctot=Ctot, coff=coff, groups=groups, slot0=slot0, slots=slots, c1=C1, eps=eps,
                    x=x, partials=partials, gamma=gamma, beta=beta, ss=ss, counters=counters, x1=x1)


def gn_finalize(partials, gamma, beta, ss, *, B, C, groups, slots, HW, eps):
    return build_op(L.OP_GN_FINALIZE, b=B, c=C, groups=groups, slots=slots, hw=HW, eps=eps, partials=partials, gamma=gamma, beta=beta, ss=ss)


def gn_apply(x, ss, out, *, B, HW, C, silu, x1=None, C0=0):
    return build_op(L.OP_GN_APPLY, b=B, hw=HW, c=C, silu=silu, c0=C0, x=x, ss=ss, out=out, x1=x1)


def gn_slab(x0, out, ss, *, B, HW, C, groups, gamma, beta, eps, silu=False, x1=None, C0=0):
    """GroupNorm in one launch (MG_OP_GN_SLAB): scale / shift into ``ss`` and, with ``out``, the normalised tensor."""
    return build_op(L.OP_GN_SLAB, b=B, hw=HW, c=C, c0=C0, groups=groups, silu=silu, eps=eps, x0=x0, x1=x1, out=out, gamma=gamma, beta=beta, ss=ss)


SPLITK_WS_BYTES = 64 << 20   # MG_SPLITK_WS_BYTES (csrc/common.h): what MG_OP_IGEMM's splitk_ws must hold
FLASH_WS_BYTES = 4096 + 255 * 4 * 4 * (16384 + 1024)   # tickets + four partial results for up to 255 split blocks of queries (tests: split = 1)
# What the engine allocates per program: the automatic rule (split = 0) only splits a left-over of at most CUs / 8 blocks (32 on
# MI355X; 40 leaves room for a larger part) - 11 MB instead of 71 MB zeroed per Builder.  A smaller workspace than a launch could
# use is safe: the plan then does not split (flash4w.hip::mg_flash4w_plan).
FLASH_WS_BYTES_AUTO = 4096 + 40 * 4 * 4 * (16384 + 1024)


def flash_attn64(q, k, vt, o, *, B, heads, Ntok, ldq, ldo, ldvt, sq, sk, svt, so, scale, variant=0, vt_perm=False, dbg=None,
                 redo_thr=0.0, ws=None, ws_bytes=0, split=0):
    """``vt_perm``: V^T holds its keys in the order [0-3, 8-11, 4-7, 12-15] inside every group of 16 (what MG_OP_IGEMM's
    transposed section writes with ``trans_perm``) - generation 3 consumes that order without a lane exchange.
    ``redo_thr`` (tests only; 0 = 2^100): the row-sum bound above which the hand-placed kernel (variant 26) redoes a block of
    queries with the running-maximum loop.  ``ws`` (optional, ZEROED once, then owned by the launches of one stream): workspace of
    the hand-placed kernel's key-split blocks - the blocks of 256 queries beyond the last multiple of the CU count are split
    along the keys over the chip (``FLASH_WS_BYTES`` covers every case); ``split``: 0 = when it pays, 1 = always (tests), 2 = never."""
    return build_op(L.OP_FLASH_ATTN64, b=B, heads=heads, ntok=Ntok, ldq=ldq, ldo=ldo, ldvt=ldvt, variant=variant, vt_perm=vt_perm,
                    ws_kb=ws_bytes // 1024, split=split, scale=scale, redo_thr=redo_thr, q=q, k=k, vt=vt, o=o, dbg=dbg, ws=ws,
                    sq=sq, sk=sk, svt=svt, so=so)


def flash_attn512(q, k, vt, o, *, B, Ntok, ldq, ldo, ldvt, sq, sk, svt, so, scale):
    """One head of width 512 (the VAE mid-block attention), flash form: no score matrix in memory (MG_OP_FLASH_ATTN512)."""
    return build_op(L.OP_FLASH_ATTN512, b=B, ntok=Ntok, ldq=ldq, ldo=ldo, ldvt=ldvt, scale=scale, q=q, k=k, vt=vt, o=o, sq=sq, sk=sk, svt=svt, so=so)


VT_PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def permute_vt_keys(vt):
    """Natural V^T [..., keys] (keys a multiple of 16) -> the ``vt_perm`` order (host helper for tests / tools)."""
    sh = vt.shape
    return vt.reshape(*sh[:-1], sh[-1] // 16, 16)[..., list(VT_PERM16)].reshape(sh).contiguous()


def softmax_rows(s, p, *, R, ncols, lds, ldp):
    return build_op(L.OP_SOFTMAX_ROWS, r=R, ncols=ncols, lds=lds, ldp=ldp, scores=s, probs=p)


def sched_step(x, model_out, noise, out, *, n, cx, cm, cn=0.0):
    return build_op(L.OP_SCHED_STEP, cx=cx, cm=cm, cn=cn, x=x, model_out=model_out, noise=noise, out=out, n=n)


def linear_small_m(x, w, b, out, *, M, N, K, act_in=0, act_out=0, ldo=0):
    return build_op(L.OP_LINEAR_SMALL_M, m=M, n=N, k=K, act_in=act_in, act_out=act_out, ldo=ldo, x=x, w=w, bias=b, out=out)


def latent_1x1(x, w, b, out, *, B, Ci, Co, HW, scale=1.0):
    return build_op(L.OP_LATENT_1X1, b=B, ci=Ci, co=Co, hw=HW, scale=scale, x=x, w=w, bias=b, out=out)


def im2col_small(src0, src1, out, *, B, H, W, C0, C1, Kp, bcast0=False, members_per_src0=0):
    """``members_per_src0`` = m > 0: row b reads src0 row b // m (src0 [B / m, C0, H, W]); 0 = ``bcast0`` decides."""
    return build_op(L.OP_IM2COL_SMALL, b=B, h=H, w=W, c0=C0, c1=C1, kp=Kp, src0_broadcast=bcast0, members_per_src0=members_per_src0,
                    src0=src0, src1=src1, out=out)


def conv3x3_head(x, ss, w, bias, out, *, B, H, W, C, Cout, ldo=0, silu=True):
    """GroupNorm apply (``ss`` = scale / shift [B][2][C], or None) [+ SiLU] + conv3x3 pad 1 to <= 4 fp32 channels, one launch
    (MG_OP_CONV3X3_HEAD); ``w`` bf16 [>= Cout][9 C] as weights.pack_conv3x3 lays it out."""
    return build_op(L.OP_CONV3X3_HEAD, b=B, h=H, w=W, c=C, cout=Cout, ldo=ldo, silu=silu, x=x, ss=ss, wt=w, bias=bias, out=out)


def post_nchw(x, out, *, B, HW, Cout, ldi, post=L.POST_NONE, scale=1.0, noise=None, cx=0.0, cm=0.0, cn=0.0):
    return build_op(L.OP_POST_NCHW, b=B, hw=HW, cout=Cout, ldi=ldi, post=post, scale=scale, cx=cx, cm=cm, cn=cn, x=x, out=out, noise=noise)


def ens_depth_stats(d, scratch, out, *, E, HW):
    return build_op(L.OP_ENS_DEPTH_STATS, e=E, d=d, scratch=scratch, out=out, hw=HW)


def ens_depth_median(d, st, med, mad, minmax, scratch, *, E, HW, reduction=0, has_shift=True):
    return build_op(L.OP_ENS_DEPTH_MEDIAN, e=E, reduction=reduction, has_shift=has_shift, d=d, st=st, med=med, mad=mad, minmax=minmax,
                    scratch=scratch, hw=HW)


def ens_depth_norm(med, unc, minmax, *, HW, shift_invariant=True):
    return build_op(L.OP_ENS_DEPTH_NORM, shift_invariant=shift_invariant, med=med, mad=unc, minmax=minmax, hw=HW)


def ens_normals(n, out, unc, *, E, HW, reduction=0):
    return build_op(L.OP_ENS_NORMALS, e=E, reduction=reduction, normals=n, out=out, unc=unc, hw=HW)


def ens_iid(preds, pred, unc, *, E, n, reduction=0):
    """The intrinsic-image ensemble (MG_OP_ENS_IID): fp32 ``preds`` [E, n] -> ``pred`` [n] and, unless ``unc`` is None, ``unc`` [n]:
    per element the median (+ median absolute deviation; ``reduction`` 0) or the mean (+ unbiased std; 1) over the members."""
    return build_op(L.OP_ENS_IID, e=E, reduction=reduction, preds=preds, pred=pred, unc=unc, n=n)


def resize(src, dst, tmp, *, planes, Hin, Win, Hout, Wout, mode, u8):
    return build_op(L.OP_RESIZE, planes=planes, hin=Hin, win=Win, hout=Hout, wout=Wout, mode=mode, u8=u8, src=src, dst=dst, tmp=tmp)


def colorize(depth, lut, out, *, n, lo=0.0, hi=1.0, clipped=None, u16=None):
    """The depth picture (MG_OP_COLORIZE): fp32 ``depth`` [n] -> uint8 ``out`` [n, 3] through the 256 x 3 uint8 table ``lut``.
    ``clipped`` (fp32 [n], may be ``depth``) / ``u16`` (uint16 [n]): the same launch also stores ``clip(depth, 0, 1)`` and
    ``uint16(clip(depth, 0, 1) * 65535)`` - the range (0, 1) only; ``out`` (and ``lut``) may then be None."""
    return build_op(L.OP_COLORIZE, min_depth=lo, max_depth=hi, depth=depth, lut=lut, out=out, clipped=clipped, u16=u16, n=n)


def iid_vis(pred, out, ws, *, n, H, W, linear, up_to_scale):
    """The IID output stage for the ``n`` targets of one image (MG_OP_IID_VIS): fp32 [n,3,H,W] -> uint8 [n,H,W,3]; ``linear`` /
    ``up_to_scale``: one bool per target; ``ws``: fp32 [n, L.IID_VIS_PARTS], needed when a target is both."""
    linear, up_to_scale = [bool(v) for v in linear], [bool(v) for v in up_to_scale]
    if len(linear) != n or len(up_to_scale) != n:
        raise ValueError(f"iid_vis: {n} targets, {len(linear)} linear and {len(up_to_scale)} up_to_scale flags")
    linear_bits, scale_bits = (sum(1 << t for t, v in enumerate(flags) if v) for flags in (linear, up_to_scale))
    return build_op(L.OP_IID_VIS, n=n, h=H, w=W, linear_bits=linear_bits, up_to_scale_bits=scale_bits, pred=pred, out=out, ws=ws)


RESIZE_MODES = {"bilinear": 0, "bicubic": 1, "nearest-exact": 2}   # MG_OP_RESIZE's and MG_OP_RGB_PREP's `mode`


def rgb_prep(src, dst, tmp=None, *, Hin, Win, Hout=None, Wout=None, mode=0, hwc=True, out16=False, reciprocal=False):
    """The pipelines' input stage (MG_OP_RGB_PREP): uint8 ``src`` [Hin,Win,3] (``hwc``) or [3,Hin,Win] -> ``dst`` [3,Hout,Wout] =
    ``src / 255.0 * 2.0 - 1.0`` in fp32 or (``out16``) the library's 16-bit operand type, resampled first when the sizes differ
    (``mode``: a key of RESIZE_MODES or its number; ``tmp``: fp32 [3,Hin,Wout] when bilinear / bicubic change both sizes).
    ``reciprocal``: multiply by fp32(1 / 255) as torch's device kernel does, in place of the host kernel's IEEE division."""
    return build_op(L.OP_RGB_PREP, hin=Hin, win=Win, hout=Hin if Hout is None else Hout, wout=Win if Wout is None else Wout,
                    mode=RESIZE_MODES.get(mode, mode), hwc=bool(hwc), out16=bool(out16), reciprocal=bool(reciprocal), src=src, dst=dst, tmp=tmp)


def normals_vis(pred, out, *, H, W):
    """The normals picture (MG_OP_NORMALS_VIS): fp32 ``pred`` [3,H,W] -> uint8 ``out`` [H,W,3]."""
    return build_op(L.OP_NORMALS_VIS, h=H, w=W, pred=pred, out=out)


def randn(dst, *, n, seed, stream=0, offset=0, words=False, out16=False):
    """Native Gaussian noise (MG_OP_RANDN): elements [offset, offset + n) of stream ``stream`` of the 64-bit ``seed`` -> ``dst``, fp32 or
    (``out16``) the library's 16-bit operand type; ``words``: the raw Philox4x32-10 words instead (``dst`` uint32 / int32)."""
    seed, stream = int(seed), int(stream)
    if not (0 <= seed < 1 << 64 and 0 <= stream < 1 << 64):
        raise ValueError(f"randn: seed {seed} / stream {stream} outside 64 bits")
    as_i64 = lambda v: v - (1 << 64) if v >= 1 << 63 else v   # the bits of a uint64 in the op's int64 slot
    return build_op(L.OP_RANDN, mode=int(bool(words)), out16=bool(out16), dst=dst, n=n, offset=offset, seed=as_i64(seed), stream=as_i64(stream))


def eval_fit_width(H, W, max_res):
    """(sub-sampled width, fp32(1 / factor)) of the least-squares fit under ``alignment_max_res`` - evaluation/alignment.py:
    factor = min(max_res / (H, W)), only the width shrinks; (0, 0.0) = fit on every pixel."""
    if max_res is None:
        return 0, 0.0
    factor = min(max_res / H, max_res / W)
    if factor >= 1:
        return 0, 0.0
    import numpy as np
    return int(np.floor(W * factor)), float(np.float32(1.0 / factor))


def eval_depth_ls(pred, gt, mask, out5, scratch, *, H, W, disparity=False, max_res=None):
    """The five fp64 sums of the least-squares fit (MG_OP_EVAL_DEPTH_LS); ``scratch``: 512 x 5 doubles."""
    ow, inv = eval_fit_width(H, W, max_res)
    return build_op(L.OP_EVAL_DEPTH_LS, h=H, w=W, disparity=disparity, fit_w=ow, inv_factor=inv, pred=pred, gt=gt, mask=mask, out=out5, scratch=scratch)


def eval_depth_metrics(pred, gt, mask, sums5, out13, scratch, *, H, W, disparity=False, min_depth=None, max_depth=None):
    """Align (``sums5`` from eval_depth_ls, None = as is), clip and score (MG_OP_EVAL_DEPTH_METRICS); ``scratch``: 512 x 11 doubles."""
    return build_op(L.OP_EVAL_DEPTH_METRICS, h=H, w=W, disparity=disparity, clip_min=min_depth is not None, clip_max=max_depth is not None,
                    min_depth=min_depth or 0.0, max_depth=max_depth or 0.0, pred=pred, gt=gt, mask=mask, sums=sums5, out=out13, scratch=scratch)


def eval_normals(pred, gt, out9, err, ws, *, HW, masked=True):
    """Angular error and its statistics incl. the exact median (MG_OP_EVAL_NORMALS); ``ws``: L.EVAL_WS_BYTES."""
    return build_op(L.OP_EVAL_NORMALS, masked=masked, pred=pred, gt=gt, out=out9, err=err, ws=ws, hw=HW)


def iidscore_prep(pred, gt, mask, out8, ws, *, H, W, gamma=None):
    """Alignment scale, exact 0.9 brightness quantile and its scale for an up-to-scale IID target (MG_OP_IIDSCORE_PREP);
    ``mask`` uint8 [3,H,W] or None; ``ws``: L.EVAL_WS_BYTES, shared with the score ops of the same target."""
    return build_op(L.OP_IIDSCORE_PREP, h=H, w=W, gamma=L.iid_gamma_mode(gamma), pred=pred, gt=gt, mask=mask, out=out8, ws=ws)


def iidscore_psnr(pred, gt, mask, out8, ws, *, H, W, gamma=None, up_to_scale=False, write_psnr=True):
    """PSNR over the valid elements and their count (MG_OP_IIDSCORE_PSNR); ``up_to_scale``: map with what iidscore_prep left in ``ws``."""
    return build_op(L.OP_IIDSCORE_PSNR, h=H, w=W, gamma=L.iid_gamma_mode(gamma), up_to_scale=up_to_scale, write_psnr=write_psnr,
                    pred=pred, gt=gt, mask=mask, out=out8, ws=ws)


def iidscore_ssim(pred, gt, mask, out8, ws, *, H, W, gamma=None, up_to_scale=False):
    """Mean SSIM with the invalid elements zeroed (MG_OP_IIDSCORE_SSIM); H, W >= 11."""
    return build_op(L.OP_IIDSCORE_SSIM, h=H, w=W, gamma=L.iid_gamma_mode(gamma), up_to_scale=up_to_scale, pred=pred, gt=gt, mask=mask, out=out8, ws=ws)


def memset(dst, nbytes, value=0):
    return build_op(L.OP_MEMSET, value=value, dst=dst, bytes=nbytes)


def copy(src, dst, nbytes):
    return build_op(L.OP_COPY, src=src, dst=dst, bytes=nbytes)


# --------------------------------------------------------------------------- containers

def launch(op, stream=None, lib=None):
    """Launch one op on torch's current stream (or the given raw handle); ``lib``: the library build (default: bf16 operands)."""
    lib = lib or L.load()
    L.check(lib.mg_launch(ctypes.byref(op), stream if stream is not None else current_stream_handle()),
            f"mg_launch({L.OP_NAMES.get(op.kind, op.kind)})", lib)


class OpSeq:
    """An ordered list of ops + the tensors they reference (kept alive), compiled on demand to
    a native ``mg_program`` so that a whole UNet forward / denoising loop / VAE pass is ONE
    C call (and optionally one hipGraph launch)."""

    def __init__(self, name="", f16=False):
        self.name = name
        self.f16 = bool(f16)   # the library build this program belongs to: fp16 operands (libmarigold_hip_f16.so) or bf16
        self.ops = []
        self.labels = []
        self.keep = []
        self.zero_state = set()   # data_ptr()s of the held tensors that are zero-initialised kernel state (tickets, workspaces, pad columns)
        self._prog = None
        self._captured = False

    def add(self, op, label=""):
        self.ops.append(op)
        self.labels.append(label)
        self._prog = None
        return op

    def hold(self, *tensors):
        self.keep.extend(tensors)
        return tensors[0] if len(tensors) == 1 else tensors

    def extend(self, other):
        self.ops.extend(other.ops)
        self.labels.extend(other.labels)
        self.keep.extend(other.keep)
        self.zero_state |= other.zero_state
        self._prog = None

    def __len__(self):
        return len(self.ops)

    def compile(self):
        if self._prog is None:
            lib = L.load(self.f16)
            arr = (MgOp * len(self.ops))(*self.ops)
            prog = lib.mg_program_create(arr, len(self.ops))
            if not prog:
                L.check(1, "mg_program_create", lib)
            self._prog = prog
            self._captured = False
        return self._prog

    def run(self, stream=None):
        lib = L.load(self.f16)
        prog = self.compile()
        L.check(lib.mg_program_run(prog, stream if stream is not None else current_stream_handle()),
                f"mg_program_run({self.name})", lib)

    def run_range(self, first, count, stream=None):
        """Replay ops [first, first+count) only (step-wise inspection of a denoising program in the parity tests)."""
        lib = L.load(self.f16)
        L.check(lib.mg_program_run_range(self.compile(), int(first), int(count),
                                         stream if stream is not None else current_stream_handle()),
                f"mg_program_run_range({self.name})", lib)

    def validate(self):
        """Dry-run every op through its launcher's contract checks (works without a GPU)."""
        lib = L.load(self.f16)
        L.check(lib.mg_program_validate(self.compile()), f"mg_program_validate({self.name})", lib)

    def run_eager(self, stream=None):
        for op in self.ops:
            launch(op, stream, L.load(self.f16))

    def capture(self, stream=None):
        """Capture into a hipGraph (the stream must not be the legacy default stream)."""
        lib = L.load(self.f16)
        prog = self.compile()
        L.check(lib.mg_program_capture(prog, stream if stream is not None else current_stream_handle()),
                f"mg_program_capture({self.name})", lib)
        self._captured = True

    def profile(self, stream=None):
        """Per-op milliseconds (HIP events on the launch stream)."""
        lib = L.load(self.f16)
        prog = self.compile()
        ms = (ctypes.c_float * len(self.ops))()
        L.check(lib.mg_program_profile(prog, stream if stream is not None else current_stream_handle(), ms),
                f"mg_program_profile({self.name})", lib)
        return list(ms)

    def __del__(self):
        try:
            if self._prog is not None:
                L.load(self.f16).mg_program_destroy(self._prog)
        except Exception:
            pass
