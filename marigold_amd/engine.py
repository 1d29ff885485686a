"""Program builders: walk the SD-v2 UNet / AutoencoderKL structure (``arch.py``) and emit the
flat op programs that libmarigold_hip replays.  This is the host-side mirror of the module
seams the reference calls (marigold_depth_pipeline.py:461-463 ``unet(...)``, :491-492
``vae.encoder``/``quant_conv``, :512-513 ``post_quant_conv``/``vae.decoder``); all arithmetic
happens in the HIP kernels, torch only owns the device buffers.

Data layout: activations bf16 NHWC; latents / decoded maps fp32 NCHW (the reference's layout at
the pipeline boundary).  Buffers come from a size-keyed pool that is recycled along the static
program order, so the working set of a forward stays small and cache-friendly.
"""
import math
import threading
from collections import defaultdict

import torch

from . import _lib as L
from . import ops as O
from . import routes as R
from . import tuning
from . import weights as Wm
from .arch import UNetConfig, VAEConfig, unet_up_resnet_channels

LATENT_SCALE = 0.18215  # marigold_depth_pipeline.py:118


class Act:
    """A bf16 NHWC activation [B][H][W][C] living in a pooled buffer."""
    __slots__ = ("t", "B", "H", "W", "C", "gn")

    def __init__(self, t, B, H, W, C):
        self.t, self.B, self.H, self.W, self.C = t, B, H, W, C
        self.gn = None   # (partial table, slots per image): its GroupNorm partial sums, left by the convolution that wrote it

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def HW(self):
        return self.H * self.W


class Pool:
    def __init__(self, device):
        self.device = device
        self.free_lists = defaultdict(list)
        self.all = []
        self.bytes = 0

    def get(self, nbytes):
        nbytes = (int(nbytes) + 255) // 256 * 256
        fl = self.free_lists[nbytes]
        if fl:
            return fl.pop()
        t = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.all.append(t)
        self.bytes += nbytes
        return t

    def put(self, t):
        self.free_lists[t.numel()].append(t)


class WeightStore:
    """Device-resident, kernel-ready weights derived from a diffusers-layout state dict."""

    def __init__(self, sd, device, dtype=torch.bfloat16):
        self.sd = sd
        self.device = device
        self.dtype = dtype   # the 16-bit operand type of the library build these weights feed (bf16, or fp16: libmarigold_hip_f16.so)
        self.cache = {}
        self._lock = threading.RLock()   # engine replicas (modules._EngineModule.replica) build their programs from one store

    def _memo(self, key, fn):
        with self._lock:
            if key not in self.cache:
                self.cache[key] = fn()
            return self.cache[key]

    def has(self, name):
        return f"{name}.weight" in self.sd

    def conv3x3(self, name):
        return self._memo(("c3", name), lambda: Wm.bf16(Wm.pack_conv3x3(self.sd[f"{name}.weight"].float()), self.device, self.dtype))

    def conv3x3_fold(self, name, shortcut):
        """conv3x3 ``name`` with the 1x1 convolution ``shortcut`` of another tensor folded in as extra K (MG_OP_IGEMM p[12]):
        rows [Cout][9 Cin | Cx] bf16 and the two biases' sum."""
        def f():
            ws_ = self.sd[f"{shortcut}.weight"].float()
            w = torch.cat([Wm.pack_conv3x3(self.sd[f"{name}.weight"].float()), ws_.reshape(ws_.shape[0], -1)], dim=1)
            b = self.sd[f"{name}.bias"].float() + self.sd[f"{shortcut}.bias"].float()
            return Wm.bf16(w, self.device, self.dtype), Wm.f32(b, self.device)
        return self._memo(("c3f", name), f)

    def conv3x3_subpix(self, name):
        return self._memo(("c3s", name), lambda: Wm.bf16(Wm.pack_conv3x3_subpix(self.sd[f"{name}.weight"].float()), self.device, self.dtype))

    def mat(self, name):  # Linear or 1x1 conv -> [N][K]
        def f():
            w = self.sd[f"{name}.weight"].float()
            return Wm.bf16(w.reshape(w.shape[0], -1), self.device, self.dtype)
        return self._memo(("m", name), f)

    def vec(self, key):
        return self._memo(("v", key), lambda: Wm.f32(self.sd[key], self.device))

    def bias(self, name):
        return self.vec(f"{name}.bias") if f"{name}.bias" in self.sd else None

    def time_emb_proj_all(self, names):
        """The ResNet blocks' time_emb_proj layers stacked along N: fp32 [sum cout][temb_dim], bias [sum cout]."""
        def f():
            w = torch.cat([self.sd[f"{n}.time_emb_proj.weight"].float() for n in names], dim=0)
            b = torch.cat([self.sd[f"{n}.time_emb_proj.bias"].float() for n in names], dim=0)
            return Wm.f32(w, self.device), Wm.f32(b, self.device)
        return self._memo(("tep", tuple(names)), f)

    def f32mat(self, name):
        return self._memo(("fm", name), lambda: Wm.f32(self.sd[f"{name}.weight"].reshape(self.sd[f"{name}.weight"].shape[0], -1), self.device))

    def small_conv_mfma(self, key, w4, bias):
        """Cout <= 16 conv3x3 as an MFMA GEMM: weights [Cout,Cin,3,3] -> bf16 [8|16][9*Cin] (rows >= Cout
        zero), bias fp32 [8|16]."""
        def f():
            co = w4.shape[0]
            npad = 8 if co <= 8 else 16
            w = torch.zeros(npad, 9 * w4.shape[1])
            w[:co] = Wm.pack_conv3x3(w4.float())
            b = torch.zeros(npad)
            b[:co] = bias.float()
            return Wm.bf16(w, self.device, self.dtype), Wm.f32(b, self.device)
        return self._memo(("scm", key), f)

    def conv_in_mfma(self, name):
        """conv3x3 from <= 8 channels as a GEMM over an im2col buffer: [Cout,Cin,3,3] -> bf16
        [Cout][Kp] with k = tap*Cin + c, zero-padded to Kp (64 or 128)."""
        def f():
            w = self.sd[f"{name}.weight"].float()
            k = 9 * w.shape[1]
            kp = (k + 63) // 64 * 64
            wp = torch.zeros(w.shape[0], kp)
            wp[:, :k] = Wm.pack_conv3x3(w)
            return Wm.bf16(wp, self.device, self.dtype), kp
        return self._memo(("cim", name), f)

    def qkv(self, prefix, with_bias):
        def f():
            w = Wm.pack_qkv(*(self.sd[f"{prefix}.{q}.weight"].float() for q in ("to_q", "to_k", "to_v")))
            b = None
            if with_bias:
                b = Wm.f32(torch.cat([self.sd[f"{prefix}.{q}.bias"].float() for q in ("to_q", "to_k", "to_v")]), self.device)
            return Wm.bf16(w, self.device, self.dtype), b
        return self._memo(("qkv", prefix), f)

    # ---- Linear layers with the preceding LayerNorm folded in (weights.fold_layernorm) ----
    def _ln(self, norm):
        return self.sd[f"{norm}.weight"].float(), self.sd[f"{norm}.bias"].float()

    def qkv_ln(self, prefix, norm):
        def f():
            w = Wm.pack_qkv(*(self.sd[f"{prefix}.{q}.weight"].float() for q in ("to_q", "to_k", "to_v")))
            wp, g, c = Wm.fold_layernorm(w, None, *self._ln(norm), dtype=self.dtype)
            return wp.to(self.device), Wm.f32(g, self.device), Wm.f32(c, self.device)
        return self._memo(("qkv_ln", prefix), f)

    def geglu_ln(self, name, norm):
        def f():
            w, b = Wm.pack_geglu(self.sd[f"{name}.weight"].float(), self.sd[f"{name}.bias"].float())
            wp, g, c = Wm.fold_layernorm(w, b, *self._ln(norm), dtype=self.dtype)
            return wp.to(self.device), Wm.f32(g, self.device), Wm.f32(c, self.device)
        return self._memo(("gg_ln", name), f)

    # ---- MG_OP_ROWGEMM forms: weights in fragment order + per-stage constants (weights.pack_rowgemm) ----
    def rg_mat(self, name):
        def f():
            w = self.sd[f"{name}.weight"].float()
            w = w.reshape(w.shape[0], -1)
            b = self.sd[f"{name}.bias"].float() if f"{name}.bias" in self.sd else torch.zeros(w.shape[0])
            return Wm.pack_rowgemm(w, b, dtype=self.dtype).to(self.device)
        return self._memo(("rg_m", name), f)

    def rg_qkv_ln(self, prefix, norm):
        def f():
            w = Wm.pack_qkv(*(self.sd[f"{prefix}.{q}.weight"].float() for q in ("to_q", "to_k", "to_v")))
            wp, g, c = Wm.fold_layernorm(w, None, *self._ln(norm), dtype=self.dtype)
            return Wm.pack_rowgemm(wp.float(), c, g, dtype=self.dtype).to(self.device)
        return self._memo(("rg_qkv_ln", prefix), f)

    def rg_geglu_ln(self, name, norm):
        def f():
            w, b = self.sd[f"{name}.weight"].float(), self.sd[f"{name}.bias"].float()
            order = Wm.rowgemm_geglu_order(w.shape[0])
            wp, g, c = Wm.fold_layernorm(w[order], b[order], *self._ln(norm), dtype=self.dtype)
            return Wm.pack_rowgemm(wp.float(), c, g, dtype=self.dtype).to(self.device)
        return self._memo(("rg_gg_ln", name), f)

    def rg_cross_ln(self, prefix, ctx, heads, norm):
        def f():
            wqk, vot, npad = Wm.cross_attention_tables(
                self.sd[f"{prefix}.to_q.weight"], self.sd[f"{prefix}.to_k.weight"],
                self.sd[f"{prefix}.to_v.weight"], self.sd[f"{prefix}.to_out.0.weight"], ctx, heads)
            assert npad == 64
            wp, g, c = Wm.fold_layernorm(wqk, None, *self._ln(norm), dtype=self.dtype)
            pack = Wm.pack_rowgemm_xattn if wqk.shape[1] == 320 else Wm.pack_rowgemm_xattn_ksplit
            return pack(wp.float(), c, g, vot, self.sd[f"{prefix}.to_out.0.bias"].float(), dtype=self.dtype).to(self.device)
        return self._memo(("rg_x_ln", prefix), f)

    def cross_ln(self, prefix, ctx, heads, norm):
        def f():
            wqk, vot, npad = Wm.cross_attention_tables(
                self.sd[f"{prefix}.to_q.weight"], self.sd[f"{prefix}.to_k.weight"],
                self.sd[f"{prefix}.to_v.weight"], self.sd[f"{prefix}.to_out.0.weight"], ctx, heads)
            wp, g, c = Wm.fold_layernorm(wqk, None, *self._ln(norm), dtype=self.dtype)
            return wp.to(self.device), Wm.f32(g, self.device), Wm.f32(c, self.device), Wm.bf16(vot, self.device, self.dtype), npad
        return self._memo(("x_ln", prefix), f)


class Builder:
    """Emits ops into an OpSeq, allocating/recycling activation buffers from a Pool."""

    def __init__(self, seq, pool, ws, groups=32):
        self.seq, self.pool, self.ws, self.groups = seq, pool, ws, groups
        self.dev = pool.device
        self.persist = {}

    # ---- buffers -------------------------------------------------------------------------
    def new(self, B, H, W, C):
        return Act(self.pool.get(B * H * W * C * 2), B, H, W, C)

    def raw(self, nbytes):
        return self.pool.get(nbytes)

    def ln_table(self, M, C):
        """Row-statistics buffer of a tensor [M][C] that feeds a folded LayerNorm: C/32 (sum, sum of squares) slots per
        row written by the producing GEMM's tiles, then [M] (mean, rstd) written by its last column tile per row block
        (MG_OP_IGEMM ln_out)."""
        return self.raw(M * (C // 32 + 1) * 8)

    @staticmethod
    def ln_mean_rstd(table, M, C):
        """Address of the (mean, rstd) rows inside ``ln_table(M, C)`` - the ln_in of the consuming Linear layers."""
        return table.data_ptr() + M * (C // 32) * 8

    def free(self, *xs):
        for x in xs:
            if x is None:
                continue
            self.drop_gn(x)
            self.pool.put(x.t if isinstance(x, Act) else x)

    def drop_gn(self, x):
        """Forget (and recycle) the GroupNorm partial table cached on ``x``: every op that WRITES into an existing Act calls this,
        so that ``gn_scale_shift`` never finalizes statistics of values the tensor no longer holds."""
        if isinstance(x, Act) and x.gn is not None:
            self.pool.put(x.gn[0])
            x.gn = None

    def zeros_persistent(self, key, nbytes):
        """A dedicated zero-initialised buffer (never recycled): V^T pad columns must stay 0."""
        if key not in self.persist:
            self.persist[key] = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        return self.persist[key]

    def add(self, op, label):
        if op.kind == L.OP_IGEMM and not O.Raw(op).splitk_ws:
            # the program's own split-K workspace: programs on concurrent streams - two maps in flight - must not share the library's
            O.Raw(op).splitk_ws = self.zeros_persistent("splitk_ws", O.SPLITK_WS_BYTES)
        self.seq.add(tuning.apply(op), label)   # (MG_OP_IGEMM: the measured tile / split-K choice where the table has one)
        if op.kind in R.TWICE_KINDS:
            assert op.kind in (L.OP_GN_STATS, L.OP_GN_FINALIZE, L.OP_GN_APPLY, L.OP_GN_SLAB, L.OP_FLASH_ATTN64, L.OP_FLASH_ATTN512)
            self.seq.add(op, label + ".again")

    # ---- primitive layers ----------------------------------------------------------------
    def gn_slab(self, srcs, name, eps, silu, apply):
        """-> (scale/shift buffer, normalised Act | None) in ONE launch."""
        x = srcs[0]
        C = sum(y.C for y in srcs)
        ss = self.raw(x.B * 2 * C * 4)
        out = self.new(x.B, x.H, x.W, C) if apply else None
        self.add(O.gn_slab(x.t, None if out is None else out.t, ss, B=x.B, HW=x.HW, C=C, groups=self.groups,
                           gamma=self.ws.vec(f"{name}.weight"), beta=self.ws.vec(f"{name}.bias"), eps=eps, silu=silu,
                           x1=srcs[1].t if len(srcs) > 1 else None, C0=x.C), f"{name}.slab" + ("+apply" if apply else ""))
        return ss, out

    def gn_scale_shift(self, srcs, name, eps, stats):
        """GroupNorm statistics over the channel concat of ``srcs`` (never materialised: one statistics launch per
        source into a shared partial table) -> fp32 [B][2][C] (scale, shift) buffer.  ``stats``: routes.NormRoute.stats."""
        if stats == R.STATS_SLAB:
            return self.gn_slab(srcs, name, eps, False, False)[0]
        B, HW = srcs[0].B, srcs[0].HW
        C = sum(x.C for x in srcs)
        if len(srcs) == 1 and srcs[0].gn is not None:   # the producing convolution left the partial sums: no pass over the tensor
            part, slots = srcs[0].gn
            ss = self.raw(B * 2 * C * 4)
            self.add(O.gn_finalize(part, self.ws.vec(f"{name}.weight"), self.ws.vec(f"{name}.bias"), ss, B=B, C=C,
                                   groups=self.groups, slots=slots, HW=HW, eps=eps), f"{name}.finalize")
            return ss
        chunks = R.gn_stats_chunks(B, HW)
        slots = chunks * len(srcs)
        part = self.raw(B * slots * self.groups * 2 * 4)
        ss = self.raw(B * 2 * C * 4)
        counters = self.zeros_persistent("gn_counters", 4 * max(B, 1024))   # stream-ordered reuse; left zero by every use
        # the image's last-arriving statistics block turns the partial table into scale / shift (no finalize launch); the two
        # sources of a skip concat share one launch
        coff = 0
        for k, grp in enumerate([srcs] if R.GN_STATS_ONE_LAUNCH else [[x] for x in srcs]):
            x1 = grp[1] if len(grp) > 1 else None
            self.add(O.gn_stats(grp[0].t, part, B=B, HW=HW, C=grp[0].C, chunks=chunks, groups=self.groups, Ctot=C, coff=coff,
                                slot0=k * chunks, slots=slots, gamma=self.ws.vec(f"{name}.weight"), beta=self.ws.vec(f"{name}.bias"),
                                ss=ss, counters=counters, eps=eps, x1=x1.t if x1 else None, C1=x1.C if x1 else 0),
                     f"{name}.stats" + (f"{k}" if len(srcs) > 1 and not R.GN_STATS_ONE_LAUNCH else ""))
            coff += grp[0].C
        self.free(part)
        return ss

    def gn_apply(self, srcs, ss, name, silu):
        """Materialise silu?(norm(concat(srcs))) as one NHWC tensor (the concat happens in the pass' addressing)."""
        x = srcs[0]
        C = sum(y.C for y in srcs)
        out = self.new(x.B, x.H, x.W, C)
        self.add(O.gn_apply(x.t, ss, out.t, B=x.B, HW=x.HW, C=C, silu=silu,
                            x1=srcs[1].t if len(srcs) > 1 else None, C0=x.C), f"{name}.apply")
        return out

    def norm(self, srcs, name, eps, silu, route):
        """GroupNorm of the concat of ``srcs`` as ``route`` (a routes.NormRoute) says -> (scale / shift buffer, normalised Act |
        None where the consuming launch applies them)."""
        if route.apply == R.APPLY_SLAB:
            return self.gn_slab(srcs, name, eps, silu, True)
        ss = self.gn_scale_shift(srcs, name, eps, route.stats)
        return ss, (None if route.apply == R.APPLY_CONSUMER else self.gn_apply(srcs, ss, name, silu))

    def group_norm(self, x, name, eps, silu):
        ss, out = self.norm([x], name, eps, silu, R.norm_route(x.B, x.HW, (x.C,), self.groups))
        self.free(ss)
        return out

    # ---- patch-resident conv3x3 (MG_OP_CONV3X3) ------------------------------------------------------
    def conv3x3p(self, srcs, name, cout, *, ss=None, silu=False, rowvec=None, residual=None, out=None, subpix=False):
        x = srcs[0]
        skip = srcs[1] if len(srcs) > 1 else None
        H, W = (2 * x.H, 2 * x.W) if subpix else (x.H, x.W)
        if out is None:
            out = self.new(x.B, H, W, cout)
        Cin = x.C + (skip.C if skip else 0)
        w = self.ws.conv3x3_subpix(name) if subpix else self.ws.conv3x3(name)
        kw = dict(B=x.B, H=x.H, W=x.W, C0=x.C, N=cout, a1=skip.t if skip else None, C1=skip.C if skip else 0, subpix=subpix, ss=ss,
                  silu=silu, bias=self.ws.bias(name), rowvec=rowvec, rowvec_bcast=rowvec is not None,
                  residual=None if residual is None else residual.t, wz=cout * 4 * Cin if subpix else 0)
        op = O.conv3x3(x.t, w, out.t, **kw)
        self.drop_gn(out)   # this launch rewrites `out`: a table left by an earlier producer describes other values
        if R.gn_byproduct_ok(out.HW, cout, self.groups):   # the GroupNorm statistics of the output from this launch's epilogue
            slots = O.conv3x3_gn_slots(op, getattr(self.seq, "f16", False))
            if slots > 0:
                part = self.raw(x.B * slots * self.groups * 2 * 4)
                op = O.conv3x3(x.t, w, out.t, gn_part=part, gn_cpg=cout // self.groups, gn_slots=slots, **kw)
                out.gn = (part, slots)
        self.add(op, name)
        return out

    def conv3x3(self, x, name, cout, *, stride=1, pad=1, up=None, rowvec=None, residual=None, out=None, fold=None, route=None):
        """3x3 convolution of ``x`` as ``route`` (routes.conv_route; asked here for a convolution outside a ResNet block) says.
        ``fold`` = (shortcut layer name, x0, x1 | None): that 1x1 convolution of x0 (+ x1) rides as extra K (routes.CONV_IGEMM only)."""
        if route is None:
            route = R.conv_route(x.B, x.H, x.W, x.C, cout, stride, pad, up, rowvec is not None or residual is not None)
        if route == R.CONV_PATCH:
            return self.conv3x3p([x], name, cout, rowvec=rowvec, residual=residual, out=out)
        if route == R.CONV_PATCH_SUBPIX:
            return self.conv3x3p([x], name, cout, out=out, subpix=True)
        H, W = (up if up else (x.H, x.W))
        if stride == 1:
            Ho, Wo = H, W
        elif pad == 1:
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        else:  # VAE encoder: pad (0,1,0,1) then stride 2
            Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        if out is None:
            out = self.new(x.B, Ho, Wo, cout)
        self.drop_gn(out)
        kw = dict(B=x.B, H=x.H, W=x.W, Cin=x.C, N=cout)
        if route == R.CONV_IGEMM_SUBPIX:
            self.add(O.igemm(x.t, self.ws.conv3x3_subpix(name), out.t, Ho=x.H, Wo=x.W, taps=4, stride=1, pad=1, bias=self.ws.bias(name),
                             batch_z=4, zstrides=(0, cout * 4 * x.C, 0, 0), **kw), name)
        elif fold is not None:
            sc, x0, x1 = fold
            wf, bf = self.ws.conv3x3_fold(name, sc)
            cx = x0.C + (x1.C if x1 is not None else 0)
            self.add(O.igemm(x.t, wf, out.t, Ho=Ho, Wo=Wo, taps=9, stride=1, pad=1, bias=bf, rowvec=rowvec, rowvec_bcast=rowvec is not None,
                             fold=(x0.t, None if x1 is None else x1.t, x0.C, cx), **kw), f"{name}+{sc.rsplit('.', 1)[-1]}")
        else:
            self.add(O.igemm(x.t, self.ws.conv3x3(name), out.t, Ho=Ho, Wo=Wo, taps=9, stride=stride, pad=pad, up=up, bias=self.ws.bias(name),
                             rowvec=rowvec, rowvec_bcast=rowvec is not None,
                             residual=None if residual is None else residual.t, **kw), name)
        return out

    def conv_from_nchw(self, src0, src1, name, B, H, W, C0, C1, cout, bcast0=False, members0=0):
        """conv3x3 (pad 1) from <= 8 fp32 NCHW channels (two sources = the folded torch.cat of
        marigold_depth_pipeline.py:456-458) to bf16 NHWC on the MFMA path: im2col + GEMM.  ``members0`` = m > 0: row b
        takes src0 row b // m (several images' latents, m members each)."""
        w, kp = self.ws.conv_in_mfma(name)
        col = self.raw(B * H * W * kp * 2)
        self.add(O.im2col_small(src0, src1, col, B=B, H=H, W=W, C0=C0, C1=C1, Kp=kp, bcast0=bcast0,
                                members_per_src0=members0), f"{name}.im2col")
        out = self.new(B, H, W, cout)
        self.add(O.linear(col, w, out.t, M=B * H * W, K=kp, N=cout, bias=self.ws.bias(name),
                          k_alg=9 * (C0 + C1)), name)
        self.free(col)
        return out

    def norm_conv_to_nchw(self, x, norm, eps, key, w4, bias, out, cout, **kw):
        """conv_norm_out -> SiLU -> conv_out -> the pointwise tail (diffusers' output heads of the UNet and the VAE decoder)."""
        if R.head_conv_ok(x.B, x.H, x.W, x.C, cout):
            ss, _ = self.norm([x], norm, eps, True, R.norm_route(x.B, x.HW, (x.C,), self.groups, consumer=True))
            self.conv_to_nchw(x, key, w4, bias, out, cout, head_ss=ss, **kw)
            self.free(ss)
        else:
            g = self.group_norm(x, norm, eps, True)
            self.conv_to_nchw(g, key, w4, bias, out, cout, **kw)
            self.free(g)

    def conv_to_nchw(self, x, key, w4, bias, out, cout, post=L.POST_NONE, scale=1.0, sched=None, head_ss=None):
        """conv3x3 (pad 1) bf16 NHWC -> <= 4 fp32 NCHW channels on the MFMA path: GEMM into a padded
        fp32 [M][8] buffer, then the pointwise tail (MG_OP_POST_NCHW).  ``head_ss``: x is the RAW tensor and the GroupNorm's
        scale / shift + SiLU are applied inside the convolution (MG_OP_CONV3X3_HEAD)."""
        w8, b8 = self.ws.small_conv_mfma(key, w4, bias)
        npad = w8.shape[0]
        tmp = self.raw(x.M * npad * 4)
        if head_ss is not None:
            self.add(O.conv3x3_head(x.t, head_ss, w8, b8, tmp, B=x.B, H=x.H, W=x.W, C=x.C, Cout=cout, ldo=npad, silu=True),
                     f"{key[:-len('conv_out')]}conv_norm_out+silu+conv_out" if key.endswith("conv_out") else f"norm+silu+{key}")
        else:
            self.add(O.igemm(x.t, w8, tmp, B=x.B, H=x.H, W=x.W, Cin=x.C, Ho=x.H, Wo=x.W, N=npad, taps=9, stride=1,
                             pad=1, bias=b8, epi=L.EPI_F32, ldo=npad, n_alg=cout), f"{key}")
        if sched is not None:   # (cx, cm, cn, noise): the scheduler update replaces the store of the model output
            cx, cm, cn, nz = sched
            self.add(O.post_nchw(tmp, out, B=x.B, HW=x.HW, Cout=cout, ldi=npad, post=L.POST_SCHED, scale=scale, noise=nz,
                                 cx=cx, cm=cm, cn=cn), f"{key}.post+scheduler.step")
        else:
            self.add(O.post_nchw(tmp, out, B=x.B, HW=x.HW, Cout=cout, ldi=npad, post=post, scale=scale), f"{key}.post")
        self.free(tmp)

    def dense(self, x, wt, bias, N, *, residual=None, out=None, epi=L.EPI_BF16, label="", K=None, out_dtype_bytes=2,
              skip=None, ln_out=None, ln=None):
        """x: Act viewed as [M][C]; wt: [N][K] bf16.  ``skip``: second channel source (K = x.C + skip.C).  ``ln_out``:
        buffer for the row statistics of the OUTPUT (the next LayerNorm's input); ``ln`` = (stats, g, c): the LayerNorm
        of the INPUT is folded into this layer (x holds the raw rows)."""
        M, K = x.M, (K or x.C + (skip.C if skip is not None else 0))
        n_out = N // 2 if epi == L.EPI_GEGLU else N
        # row-block tickets of the statistics hand-off: this program's own zeroed buffer (never the library-global one: two
        # programs on different streams would draw from the same slots)
        ctr = self.zeros_persistent("ln_counters", 4 * 65536) if ln_out is not None else None
        if out is None:
            out = Act(self.pool.get(M * n_out * out_dtype_bytes), x.B, x.H, x.W, n_out)
        self.drop_gn(out)
        self.add(O.linear(x.t, wt, out.t, M=M, K=K, N=N, bias=bias, epi=epi,
                          residual=None if residual is None else residual.t,
                          a1=None if skip is None else skip.t, C0=x.C if skip is not None else 0, ln_out=ln_out, ln_counters=ctr,
                          ln_in=None if ln is None else ln[0], ln_g=None if ln is None else ln[1],
                          ln_c=None if ln is None else ln[2]), label)
        return out

    # ---- composite blocks ----------------------------------------------------------------
    def resnet(self, x, name, cout, eps, temb_row=None, skip=None):
        """diffusers ResnetBlock2D on the channel concat of ``x`` and ``skip`` (the UNet's up blocks; the concat is
        never materialised on the patch path), emitted as routes.resnet_route says: norm -> SiLU inside the convolution's
        operand staging, or by one pass that also performs the concat."""
        srcs = [x] + ([skip] if skip is not None else [])
        sc = f"{name}.conv_shortcut"
        r = R.resnet_route(x.B, x.H, x.W, tuple(y.C for y in srcs), cout, self.ws.has(sc), self.groups)

        def norm_conv(inputs, norm, nr, conv, cr, rowvec=None, residual=None, out=None, fold=None):
            ss, h = self.norm(inputs, norm, eps, True, nr)
            if h is None:
                y = self.conv3x3p(inputs, conv, cout, ss=ss, silu=True, rowvec=rowvec, residual=residual, out=out)
            else:
                y = self.conv3x3(h, conv, cout, rowvec=rowvec, residual=residual, out=out, fold=fold, route=cr)
                self.free(h)
            self.free(ss)
            return y

        h1 = norm_conv(srcs, f"{name}.norm1", r.norm1, f"{name}.conv1", r.conv1, rowvec=temb_row)
        if r.shortcut == R.SHORTCUT_FOLDED:
            out = norm_conv([h1], f"{name}.norm2", r.norm2, f"{name}.conv2", r.conv2, fold=(sc, x, skip))
        elif r.shortcut == R.SHORTCUT_LAUNCH:
            res = self.dense(x, self.ws.mat(sc), self.ws.bias(sc), cout, label=sc, skip=skip)
            out = norm_conv([h1], f"{name}.norm2", r.norm2, f"{name}.conv2", r.conv2, residual=res, out=res)  # in-place residual add
        else:
            assert skip is None and x.C == cout, f"{name}: the checkpoint has no conv_shortcut for {x.C} -> {cout} channels"
            out = norm_conv([h1], f"{name}.norm2", r.norm2, f"{name}.conv2", r.conv2, residual=x)
        self.free(h1)
        return out

    def self_attention(self, h, st, prefix, norm, heads, st_out, r):
        """h += to_out(attn(LN(h))) with the LayerNorm folded into the fused QKV projection (``st`` = row statistics of
        h from its producer); the to_out epilogue writes the statistics of the new h into ``st_out``.  Head dim 64.
        ``r``: the block's routes.TransformerRoute."""
        C, B, T, M = h.C, h.B, h.HW, h.M
        ldvt = (T + 63) // 64 * 64
        qk = self.raw(M * 2 * C * 2)
        vt = self.zeros_persistent(("vt", B, C, ldvt), B * C * ldvt * 2)
        # V^T with its keys in the QK^T accumulator order inside groups of 16: the QKV epilogue skips its lane regroup and
        # the attention kernel (generation 3) its v_permlane32_swap - a format private to this producer / consumer pair
        perm = T % 16 == 0
        if r.qkv is not None:
            self.add(O.rowgemm(h.t, self.ws.rg_qkv_ln(prefix, norm), qk, M=M, K=C, N=3 * C, form=L.RG_QKV, ldo=2 * C,
                               ln_in=self.ln_mean_rstd(st, M, C), vt=vt, tokens=T, ldt=ldvt, trans_from=2 * C,
                               **r.qkv), f"{prefix}.qkv")
        else:
            wqkv, g, c = self.ws.qkv_ln(prefix, norm)
            self.add(O.igemm(h.t, wqkv, qk, B=B, H=T, W=1, Cin=C, Ho=T, Wo=1, N=3 * C, ldo=2 * C, out2=vt,
                             trans_from=2 * C, ldt=ldvt, ln_in=self.ln_mean_rstd(st, M, C), ln_g=g, ln_c=c, trans_perm=perm), f"{prefix}.qkv")
        o = self.new(h.B, h.H, h.W, C)
        ws = self.zeros_persistent(("flash_ws",), O.FLASH_WS_BYTES_AUTO)   # key-split blocks of the hand-placed kernel (tickets stay 0)
        self.add(O.flash_attn64(qk, qk.data_ptr() + C * 2, vt, o.t, B=B, heads=heads, Ntok=T, ldq=2 * C,
                                ldo=C, ldvt=ldvt, sq=T * 2 * C, sk=T * 2 * C, svt=C * ldvt, so=T * C,
                                scale=1.0 / math.sqrt(C // heads), vt_perm=perm, ws=ws, ws_bytes=O.FLASH_WS_BYTES_AUTO), f"{prefix}.flash")
        self.free(qk)
        if r.whole_rows is not None:
            self.add(O.rowgemm(o.t, self.ws.rg_mat(f"{prefix}.to_out.0"), h.t, M=M, K=C, N=C, residual=h.t,
                               ln_out=self.ln_mean_rstd(st_out, M, C), **r.whole_rows), f"{prefix}.to_out")
        else:
            self.dense(o, self.ws.mat(f"{prefix}.to_out.0"), self.ws.bias(f"{prefix}.to_out.0"), C,
                       residual=h, out=h, label=f"{prefix}.to_out", ln_out=st_out)
        self.free(o)

    def cross_attention2(self, h, st, prefix, norm, heads, ctx, st_out, r):
        """h += attn2(LN(h), ctx) with the 2-token context collapsed into two thin GEMMs and the LayerNorm folded into
        the first one (``st``: row statistics of h, ``st_out``: of the new h for the next folded LayerNorm), in the form
        ``r.xattn`` names (never routes.XATTN_IN_GEGLU_LAUNCH: that one is part of the GEGLU launch)."""
        C, M = h.C, h.M
        if r.xattn_cfg is not None:
            # a single row-resident launch (the K-split kernel at the deep levels): the residual stream is read once and written once
            self.add(O.rowgemm(h.t, self.ws.rg_cross_ln(prefix, ctx, heads, norm), h.t, M=M, K=C, N=64, form=L.RG_XATTN,
                               ln_in=self.ln_mean_rstd(st, M, C), ln_out=self.ln_mean_rstd(st_out, M, C),
                               sm_cols=2 * heads, sm_scale=1.0 / math.sqrt(C // heads), **r.xattn_cfg), f"{prefix}.scores+softmax2+blend")
            return
        # ONE launch on the tile GEMM: scores GEMM with the LayerNorm folded in, the 2-key softmax on its accumulators, the
        # probabilities as the register operand of the blend GEMM (x the context's values pushed through to_out), + bias +
        # residual, in place on the residual stream, (mean, rstd) of the new rows for the next folded LayerNorm
        wqk, g, c, vot, npad = self.ws.cross_ln(prefix, ctx, heads, norm)
        if r.xattn == R.XATTN_TILE:
            self.add(O.linear(h.t, wqk, h.t, M=M, K=C, N=npad, epi=L.EPI_XATTN2, ln_in=self.ln_mean_rstd(st, M, C),
                              ln_g=g, ln_c=c, sm_scale=1.0 / math.sqrt(C // heads), sm_cols=2 * heads, out2=vot, c2=C, ldo=C,
                              bias=self.ws.bias(f"{prefix}.to_out.0"), residual=h.t, ldr=C,
                              ln_out=self.ln_mean_rstd(st_out, M, C)),
                     f"{prefix}.scores+softmax2+blend")
            return
        # more than 32 heads (no published checkpoint): two launches - scores + pair softmax, then the blend
        p = self.raw(M * npad * 2)
        self.add(O.linear(h.t, wqk, p, M=M, K=C, N=npad, epi=L.EPI_SOFTMAX2, ln_in=self.ln_mean_rstd(st, M, C), ln_g=g, ln_c=c,
                          sm_scale=1.0 / math.sqrt(C // heads), sm_cols=2 * heads), f"{prefix}.scores+softmax2")
        self.add(O.linear(p, vot, h.t, M=M, K=npad, N=C, bias=self.ws.bias(f"{prefix}.to_out.0"),
                          residual=h.t, ln_out=st_out, ln_counters=self.zeros_persistent("ln_counters", 4 * 65536)), f"{prefix}.blend")
        self.free(p)

    def transformer(self, x, name, heads, ctx):
        """diffusers Transformer2DModel / BasicTransformerBlock.  The three LayerNorms never run as passes: each Linear
        that consumes one takes the raw residual stream and corrects in its epilogue (MG_OP_IGEMM ln_in), with the row
        statistics written by the epilogue of the GEMM that produced the stream (ln_out)."""
        C = x.C
        r = R.transformer_route(x.B, x.HW, C, heads, self.groups)
        k320 = r.rows == R.ROWS_K320
        st = [self.ln_table(x.M, C) for _ in range(3)]
        ss, g = self.norm([x], f"{name}.norm", 1e-6, False, r.norm)
        if k320:   # the GroupNorm's scale / shift are applied while proj_in loads its rows
            h = self.new(x.B, x.H, x.W, C)
            self.add(O.rowgemm(x.t, self.ws.rg_mat(f"{name}.proj_in"), h.t, M=x.M, K=C, N=C, gn_ss=ss, tokens=x.HW,
                               ln_out=self.ln_mean_rstd(st[0], x.M, C), **r.whole_rows), f"{name}.proj_in")
            self.free(ss)
        else:
            self.free(ss)
            h = self.dense(g, self.ws.mat(f"{name}.proj_in"), self.ws.bias(f"{name}.proj_in"), C,
                           label=f"{name}.proj_in", ln_out=st[0])
            self.free(g)
        b = f"{name}.transformer_blocks.0"
        self.self_attention(h, st[0], f"{b}.attn1", f"{b}.norm1", heads, st[1], r)
        fuse_x = r.xattn == R.XATTN_IN_GEGLU_LAUNCH
        if not fuse_x:
            self.cross_attention2(h, st[1], f"{b}.attn2", f"{b}.norm2", heads, ctx, st[2], r)
        if r.geglu is not None:
            ff = self.new(h.B, h.H, h.W, 4 * C)
            xkw = dict(xattn=self.ws.rg_cross_ln(f"{b}.attn2", ctx, heads, f"{b}.norm2"), xout=h.t, sm_cols=2 * heads,
                       sm_scale=1.0 / math.sqrt(C // heads)) if fuse_x else {}
            self.add(O.rowgemm(h.t, self.ws.rg_geglu_ln(f"{b}.ff.net.0.proj", f"{b}.norm3"), ff.t, M=h.M, K=C, N=8 * C,
                               form=L.RG_GEGLU, ln_in=self.ln_mean_rstd(st[1] if fuse_x else st[2], h.M, C), **r.geglu, **xkw),
                     f"{b}.attn2+ff.geglu" if fuse_x else f"{b}.ff.geglu")
        else:
            wg, gg, cg = self.ws.geglu_ln(f"{b}.ff.net.0.proj", f"{b}.norm3")
            ff = self.dense(h, wg, None, 8 * C, epi=L.EPI_GEGLU, label=f"{b}.ff.geglu",
                            ln=(self.ln_mean_rstd(st[2], h.M, C), gg, cg))
        self.free(*st)
        # (round 5, tried and NOT kept: GEGLU -> ff.out in two row chunks through a chunk-sized intermediate, so that ff.out reads
        # its 236 MB A operand out of the 256 MB memory-side cache - tools/ubench/mall_probe.py: 6.6-7.2 TB/s for working sets that
        # fit, 5.1-5.4 beyond.  ff.out gained 0.7 ms per map, the two half-size GEGLU launches lost 3.0:
        # profiles/r5_ff_row_chunks_lost.log)
        self.dense(ff, self.ws.mat(f"{b}.ff.net.2"), self.ws.bias(f"{b}.ff.net.2"), C, residual=h, out=h,
                   label=f"{b}.ff.out")
        self.free(ff)
        # NB: the GEMM input must never alias its output (other column tiles still read it)
        if k320:
            self.add(O.rowgemm(h.t, self.ws.rg_mat(f"{name}.proj_out"), x.t, M=h.M, K=C, N=C, residual=x.t,
                               **r.proj_out), f"{name}.proj_out")
            out = x
        else:
            out = self.dense(h, self.ws.mat(f"{name}.proj_out"), self.ws.bias(f"{name}.proj_out"), C,
                             residual=x, out=x, label=f"{name}.proj_out")
        self.free(h)
        return out

    def vae_attention(self, x, name):
        """Single-head d=C attention of the VAE mid block: the flash form (MG_OP_FLASH_ATTN512) for the published width of
        512 channels, the materialised fp32 scores for any other width (the tiny test architecture)."""
        C, B, T, M = x.C, x.B, x.HW, x.M
        g = self.group_norm(x, f"{name}.group_norm", 1e-6, False)
        wqkv, bqkv = self.ws.qkv(name, True)
        ldp = (T + 63) // 64 * 64
        Tn = (T + 7) // 8 * 8           # score columns in whole 8-column store groups: the K rows past the last image's
        qk = self.raw((M + 8) * 2 * C * 2)   # tokens are slack rows, their columns are never read by the softmax
        vt = self.zeros_persistent(("vvt", B, C, ldp), B * C * ldp * 2)
        self.add(O.igemm(g.t, wqkv, qk, B=B, H=T, W=1, Cin=C, Ho=T, Wo=1, N=3 * C, ldo=2 * C, bias=bqkv,
                         out2=vt, trans_from=2 * C, ldt=ldp), f"{name}.qkv")
        self.free(g)
        o = self.new(x.B, x.H, x.W, C)
        if R.vae_attention_flash(B, T, C):   # the T x T scores never leave the registers
            self.add(O.flash_attn512(qk, qk.data_ptr() + C * 2, vt, o.t, B=B, Ntok=T, ldq=2 * C, ldo=C, ldvt=ldp,
                                     sq=T * 2 * C, sk=T * 2 * C, svt=C * ldp, so=T * C, scale=1.0 / math.sqrt(C)), f"{name}.flash")
            self.free(qk)
        else:
            # scores GEMM -> row softmax -> P V, everything in one batched launch per stage
            sc = self.raw(B * T * ldp * 4)
            self.add(O.igemm(qk, qk.data_ptr() + C * 2, sc, B=1, H=T, W=1, Cin=C, Ho=T, Wo=1, N=Tn, epi=L.EPI_F32, ldo=ldp,
                             lda=2 * C, ldw=2 * C, batch_z=B, n_alg=T, zstrides=(T * 2 * C, T * 2 * C, T * ldp, 0),
                             scale=1.0 / math.sqrt(C)), f"{name}.scores")
            self.free(qk)
            p = self.raw(B * T * ldp * 2)
            self.add(O.softmax_rows(sc, p, R=B * T, ncols=T, lds=ldp, ldp=ldp), f"{name}.softmax")
            self.free(sc)   # (the fp32 scores and the bf16 probabilities never live side by side beyond this launch)
            self.add(O.igemm(p, vt, o.t, B=1, H=T, W=1, Cin=ldp, Ho=T, Wo=1, N=C, lda=ldp, ldw=ldp, batch_z=B,
                             zstrides=(T * ldp, C * ldp, T * C, 0)), f"{name}.pv")
            self.free(p)
        out = self.dense(o, self.ws.mat(f"{name}.to_out.0"), self.ws.bias(f"{name}.to_out.0"), C,
                         residual=x, label=f"{name}.to_out")
        self.free(o)
        return out


# ------------------------------------------------------------------------------------------ UNet

def sinusoid_table(timesteps, dim):
    """diffusers Timesteps(dim, flip_sin_to_cos=True, freq_shift=0): [cos | sin], fp32."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    arg = torch.as_tensor(timesteps, dtype=torch.float32)[:, None] * freqs[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)


def unet_resnet_names(cfg: UNetConfig):
    """[(state-dict prefix, cout)] of every ResNet block, in execution order."""
    boc = list(cfg.block_out_channels)
    n = len(boc)
    names = []
    for i in range(n):
        for j in range(cfg.layers_per_block):
            names.append((f"down_blocks.{i}.resnets.{j}", boc[i]))
    names += [("mid_block.resnets.0", boc[-1]), ("mid_block.resnets.1", boc[-1])]
    for (i, j, _rin, _skip, out) in unet_up_resnet_channels(cfg):
        names.append((f"up_blocks.{i}.resnets.{j}", out))
    return names


def emit_time_embeddings(bld, cfg, timesteps):
    """Ops computing, for all T steps at once, the per-ResNet time-embedding projections
    (sinusoid -> Linear -> SiLU -> Linear -> [SiLU -> Linear] per block).  Returns
    {resnet prefix: fp32 tensor [T][cout]}."""
    ws, dev = bld.ws, bld.dev
    T = len(timesteps)
    c0, td = cfg.block_out_channels[0], cfg.temb_dim
    sin = bld.seq.hold(sinusoid_table(list(timesteps), c0).to(dev))
    e1 = bld.seq.hold(torch.empty(T, td, device=dev))
    emb = bld.seq.hold(torch.empty(T, td, device=dev))
    bld.add(O.linear_small_m(sin, ws.f32mat("time_embedding.linear_1"), ws.bias("time_embedding.linear_1"), e1,
                             M=T, N=td, K=c0, act_out=1), "time_embedding.linear_1")
    bld.add(O.linear_small_m(e1, ws.f32mat("time_embedding.linear_2"), ws.bias("time_embedding.linear_2"), emb,
                             M=T, N=td, K=td), "time_embedding.linear_2")
    # every ResNet block's projection in ONE launch: their weights stacked along N (24 launches of ~20 us each otherwise);
    # a block's row for step s is table[name][s] - a view of the [T][sum of couts] result
    names = list(unet_resnet_names(cfg))
    ntot = sum(cout for _, cout in names)
    wcat, bcat = ws.time_emb_proj_all([name for name, _ in names])
    tall = bld.seq.hold(torch.empty(T, ntot, device=dev))
    bld.add(O.linear_small_m(emb, wcat, bcat, tall, M=T, N=ntot, K=td, act_in=1), "resnets.time_emb_proj")
    table, off = {}, 0
    for name, cout in names:
        table[name] = tall[:, off:off + cout]
        off += cout
    return table


def emit_unet_forward(bld, cfg, ctx, rgb_latent, x_latent, eps_out, temb_table, step, B, h, w, sched=None, rgb_members=None):
    """One UNet forward: eps_out[B,4,h,w] = unet(cat(rgb_latent, x_latent), t_step, ctx).
    rgb_latent is [1,4,h,w] (shared by all members) or [B,4,h,w]; with ``rgb_members`` = m it is [B / m,4,h,w] and
    member b takes image b // m.  With ``sched`` = (cx, cm, cn, noise) the model
    output is not stored: the scheduler update x_latent <- cx x_latent + cm out + cn noise is conv_out's tail."""
    ws = bld.ws
    boc = list(cfg.block_out_channels)
    n = len(boc)

    def trow(name, cout):
        assert temb_table[name].shape[1] == cout
        return temb_table[name][step].data_ptr()   # cout contiguous fp32 values

    c0 = boc[0]
    cin = ws.sd["conv_in.weight"].shape[1]
    c_rgb = rgb_latent.shape[1]   # 4 image-latent channels + 4 per predicted modality (IID: 8 / 12)
    x = bld.conv_from_nchw(rgb_latent, x_latent, "conv_in", B, h, w, c_rgb, cin - c_rgb, c0,
                           bcast0=not rgb_members and rgb_latent.shape[0] == 1, members0=rgb_members or 0)
    skips = [x]
    force_size = any(d % (2 ** (n - 1)) != 0 for d in (h, w))
    for i in range(n):
        for j in range(cfg.layers_per_block):
            name = f"down_blocks.{i}.resnets.{j}"
            y = bld.resnet(x, name, boc[i], 1e-5, trow(name, boc[i]))
            if i < n - 1:
                y = bld.transformer(y, f"down_blocks.{i}.attentions.{j}", cfg.heads[i], ctx)
            x = y
            skips.append(x)
        if i < n - 1:
            x = bld.conv3x3(x, f"down_blocks.{i}.downsamplers.0.conv", boc[i], stride=2, pad=1)
            skips.append(x)
    name = "mid_block.resnets.0"
    y = bld.resnet(x, name, boc[-1], 1e-5, trow(name, boc[-1]))
    y = bld.transformer(y, "mid_block.attentions.0", cfg.heads[-1], ctx)
    name = "mid_block.resnets.1"
    x2 = bld.resnet(y, name, boc[-1], 1e-5, trow(name, boc[-1]))
    bld.free(y)
    x = x2  # the pre-mid x is still referenced by skips[-1]
    rheads = list(cfg.heads)[::-1]
    for (i, j, _rin, _skip, cout) in unet_up_resnet_channels(cfg):
        skip = skips.pop()
        name = f"up_blocks.{i}.resnets.{j}"
        # torch.cat([hidden, skip], dim=1) is folded into the consumers: two statistics launches, two-source operand
        # staging in conv1 / conv_shortcut (or the normalisation pass that materialises the input where it is not fused)
        y = bld.resnet(x, name, cout, 1e-5, trow(name, cout), skip=skip)
        bld.free(x, skip)
        if i > 0:
            y = bld.transformer(y, f"up_blocks.{i}.attentions.{j}", rheads[i], ctx)
        x = y
        if j == cfg.layers_per_block and i < n - 1:
            if force_size:
                up = (skips[-1].H, skips[-1].W)
            else:
                up = (2 * x.H, 2 * x.W)
            y = bld.conv3x3(x, f"up_blocks.{i}.upsamplers.0.conv", cout, up=up)
            bld.free(x)
            x = y
    bld.norm_conv_to_nchw(x, "conv_norm_out", 1e-5, "conv_out", ws.sd["conv_out.weight"], ws.sd["conv_out.bias"],
                          x_latent if sched else eps_out, cfg.out_channels, sched=sched)
    bld.free(x)


# ------------------------------------------------------------------------------------------ VAE

def emit_vae_encode(bld, cfg: VAEConfig, rgb, lat_out, B, H, W):
    """lat_out[B,4,H/8,W/8] = 0.18215 * mean(quant_conv(encoder(rgb)))  (fp32 NCHW in/out).
    quant_conv (1x1) and the posterior-mean selection are composed into the encoder's conv_out."""
    ws = bld.ws
    boc = list(cfg.block_out_channels)
    x = bld.conv_from_nchw(rgb, None, "encoder.conv_in", B, H, W, 3, 0, boc[0])
    for i, c in enumerate(boc):
        for j in range(cfg.layers_per_block):
            y = bld.resnet(x, f"encoder.down_blocks.{i}.resnets.{j}", c, 1e-6)
            bld.free(x)
            x = y
        if i < len(boc) - 1:
            y = bld.conv3x3(x, f"encoder.down_blocks.{i}.downsamplers.0.conv", c, stride=2, pad=0)
            bld.free(x)
            x = y
    x = emit_vae_mid(bld, x, "encoder.mid_block")
    g = bld.group_norm(x, "encoder.conv_norm_out", 1e-6, True)
    bld.free(x)
    L4 = cfg.latent_channels

    def composed():
        wc = ws.sd["encoder.conv_out.weight"].double()          # [2L, C, 3, 3]
        bc = ws.sd["encoder.conv_out.bias"].double()
        wq = ws.sd["quant_conv.weight"].double().reshape(2 * L4, 2 * L4)[:L4]   # mean rows
        bq = ws.sd["quant_conv.bias"].double()[:L4]
        w = torch.einsum("om,mcyx->ocyx", wq, wc)
        b = wq @ bc + bq
        return w.float(), b.float()
    wcomp, bcomp = ws._memo(("enc_tail",), composed)
    bld.conv_to_nchw(g, "encoder.conv_out+quant_conv", wcomp, bcomp, lat_out, L4, scale=LATENT_SCALE)
    bld.free(g)
    return g.H, g.W


def emit_vae_mid(bld, x, name):
    y = bld.resnet(x, f"{name}.resnets.0", x.C, 1e-6)
    bld.free(x)
    z = bld.vae_attention(y, f"{name}.attentions.0")
    bld.free(y)
    out = bld.resnet(z, f"{name}.resnets.1", z.C, 1e-6)
    bld.free(z)
    return out


def emit_vae_decode(bld, cfg: VAEConfig, latent, out, B, h, w, post):
    """out = tail(decoder(post_quant_conv(latent / 0.18215))); ``post`` fuses the pipeline's
    pointwise tail (depth: mean/clip/shift -> [B,1,H,W]; normals: clip/normalise -> [B,3,H,W])."""
    ws = bld.ws
    rev = list(cfg.block_out_channels)[::-1]
    L4 = cfg.latent_channels
    z = bld.raw(B * L4 * h * w * 4)
    bld.add(O.latent_1x1(latent, ws.f32mat("post_quant_conv"), ws.bias("post_quant_conv"), z, B=B, Ci=L4,
                         Co=L4, HW=h * w, scale=1.0 / LATENT_SCALE), "post_quant_conv")
    x = bld.conv_from_nchw(z, None, "decoder.conv_in", B, h, w, L4, 0, rev[0])
    bld.free(z)
    x = emit_vae_mid(bld, x, "decoder.mid_block")
    for i, c in enumerate(rev):
        for j in range(cfg.layers_per_block + 1):
            y = bld.resnet(x, f"decoder.up_blocks.{i}.resnets.{j}", c, 1e-6)
            bld.free(x)
            x = y
        if i < len(rev) - 1:
            y = bld.conv3x3(x, f"decoder.up_blocks.{i}.upsamplers.0.conv", c, up=(2 * x.H, 2 * x.W))
            bld.free(x)
            x = y
    bld.norm_conv_to_nchw(x, "decoder.conv_norm_out", 1e-6, "decoder.conv_out", ws.sd["decoder.conv_out.weight"],
                          ws.sd["decoder.conv_out.bias"], out, 3, post=post)
    bld.free(x)
    return x.H, x.W
