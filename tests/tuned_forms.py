"""The launch forms of marigold_amd/tuning/gfx950.json, one per (form, tile, split-K count): a plain helper module for
tests/test_gpu_tuned_launches.py and tests/test_tuned_launches_host.py (like tests/op_reference.py; not collected).

  ``classes()``               the table's entries grouped by everything in their key except M, plus the tile and the split count.
  ``build(cls, M, device)``   the ``mg_op`` of a class at a reduced row count (``M`` = None) or at a given M, through
                              ``marigold_amd.ops.igemm`` with ``variant=`` / ``splits=`` of the entry, seeded operands generated on
                              the device (``dummy=True``: one-element host tensors, for the field checks that need no GPU).
  ``reference(built)``        the result in float64 from the operands as stored (packed / folded weights, 16-bit activations, fp32
                              bias, row vector and statistics), every row.
  ``yardstick(built)``        the same operands through torch's own bf16 path, every intermediate the unfused chain would store
                              rounded to bf16 (F.linear on the gathered taps; F.layer_norm in fp32, rounded, for the fold forms).

N and K are the table's (tile legality, K tiles per split and the N edge depend on them); only M shrinks - ``geometry``.  The
fields the key does not carry (C0 of a two-source launch, Cx0 of a folded shortcut, trans_perm, ldt, n_alg, k_alg, the
broadcast row vector, leading dimensions) are set the way engine.py sets them for the layer the entry's label names;
tests/test_tuned_launches_host.py pins them to the ops of the full-size programs.
"""
import math
import re
import zlib
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from marigold_amd import _lib as L, ops as O, tuning, weights as Wm
from marigold_amd.arch import UNetConfig, VAEConfig, unet_up_resnet_channels

LN_EPS = 1e-5
BK = 64            # K-tile width the split clamp of the class ids is worked out with (igemm2.hip: sp = min(splits, KT / 2))


@dataclass
class TunedClass:
    rest: str                  # the key without its first field (M)
    tile: int
    splits: int
    entries: list = field(default_factory=list)   # the table keys of this class
    labels: list = field(default_factory=list)    # their layer labels ("E=1 down_blocks.1.attentions.0.proj_in")

    def __post_init__(self):
        p = self.rest.split(",")
        (self.N, self.K, self.taps, self.stride, self.epi, self.trans, self.bz, self.res, self.stats, self.ln, self.src2,
         self.temb) = (int(x) for x in p[:12])
        self.Cx = int(p[12][1:]) if len(p) > 12 else 0
        self.Cin = self.K // self.taps

    @property
    def id(self):
        c = self
        flags = f"t{c.taps}" + (f"s{c.stride}" if c.stride != 1 else "") + {L.EPI_BF16: "", L.EPI_GEGLU: "+geglu", L.EPI_F32: "+f32"}[c.epi]
        flags += ("+vt" if c.trans else "") + (f"+z{c.bz}" if c.bz > 1 else "") + ("+res" if c.res else "") + ("+stats" if c.stats else "")
        flags += ("+ln" if c.ln else "") + ("+a1" if c.src2 else "") + ("+temb" if c.temb else "") + (f"+x{c.Cx}" if c.Cx else "")
        s = f"{c.N},{c.K},{flags},v{c.tile},s{c.splits}"
        kt = (c.K + c.Cx) // BK
        if c.splits > max(1, kt // 2):
            s += f",clamp{max(1, kt // 2)}"     # fewer K tiles than 2 per split at this K: the launcher takes this many
        if c.taps == 4:
            s += ",M336=8x6x7"                  # 8 images: 2 x 42 rows would not fill one 256-row tile
        return s


def classes():
    """[TunedClass] in table order: every entry belongs to exactly one."""
    out = {}
    for key, hit in tuning.load().items():
        rest = key.split(",", 1)[1]
        c = out.setdefault((rest, int(hit[0]), int(hit[1])), TunedClass(rest, int(hit[0]), int(hit[1])))
        c.entries.append(key)
        c.labels.append(str(hit[4]))
    return list(out.values())


def class_of(key):
    hit = tuning.load()[key]
    return (key.split(",", 1)[1], int(hit[0]), int(hit[1]))


# --------------------------------------------------------------------------- what the key does not carry

def _up_resnet(label):
    """(channels from below, skip channels) of a UNet up-block ResNet named in ``label``, else None (one source)."""
    m = re.search(r"(?<![.\w])up_blocks\.(\d+)\.resnets\.(\d+)\.", label.split(" ", 1)[-1])
    if not m:
        return None
    for i, j, rin, skip, _ in unet_up_resnet_channels(UNetConfig()):
        if (i, j) == (int(m.group(1)), int(m.group(2))):
            return rin, skip
    raise KeyError(label)


def layer_fields(cls):
    """C0 / Cx0 / n_alg / k_alg as engine.py sets them for the layers the class's labels name (they must all agree)."""
    got = set()
    for lab in cls.labels:
        up = _up_resnet(lab)
        f = {"C0": 0, "Cx0": cls.Cx, "two_x": False, "n_alg": 0, "k_alg": 0}
        if cls.src2:     # Builder.dense(skip=): A = the hidden tensor, A1 = the skip
            assert up is not None and sum(up) == cls.Cin, (lab, up, cls.Cin)
            f["C0"] = up[0]
        if cls.Cx and up is not None:   # Builder.conv3x3(fold=(shortcut, x, skip))
            assert sum(up) == cls.Cx, (lab, up, cls.Cx)
            f["Cx0"], f["two_x"] = up[0], True
        if cls.epi == L.EPI_F32:        # Builder.conv_to_nchw: the output head padded to 8 columns
            assert lab.endswith("conv_out") and cls.N == 8, lab
            f["n_alg"] = UNetConfig().out_channels
        if lab.endswith("conv_in"):     # Builder.conv_from_nchw: K padded up from 9 x the latent channels (VAE decoder: 4, UNet: 8)
            f["k_alg"] = 9 * (VAEConfig().latent_channels if "vae." in lab else UNetConfig().in_channels)
        got.add(tuple(sorted(f.items())))
    assert len(got) == 1, (cls.id, cls.labels, got)
    return dict(got.pop())


def geometry(cls, M=None):
    """(B, H, W, Ho, Wo): the reduced shape (M = None) - one whole 256-row tile and a ragged one, also of the 192-row tile -
    or a shape with exactly M output rows."""
    if M is not None:
        return (1, 2 * M - 1, 1, M, 1) if cls.stride == 2 else (1, M, 1, M, 1)
    if cls.taps == 9:
        return (2, 24, 26, 12, 13) if cls.stride == 2 else (2, 12, 13, 12, 13)
    if cls.taps == 4:
        return (8, 6, 7, 6, 7)
    if cls.trans:
        return (2, 144, 1, 144, 1)      # the permuted V^T section needs multiples of 16 tokens
    return (1, 312, 1, 312, 1)


# --------------------------------------------------------------------------- building

@dataclass
class Built:
    cls: TunedClass
    op: object
    geom: tuple
    lay: dict
    t: dict            # operands and outputs by name (None where the form has none)
    perm: bool = False


_DUMMY = torch.zeros(1)
_SHARED = {}


def _shared(name, device, make):
    key = (name, str(device))
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def build(cls, M_small=None, device=None, dummy=False):
    B, H, W, Ho, Wo = geom = geometry(cls, M_small)
    lay = layer_fields(cls)
    N, Cin, taps, Cx = cls.N, cls.Cin, cls.taps, cls.Cx
    M, Min = B * Ho * Wo, B * H * W
    Ktot = taps * Cin + Cx
    tf = N * 2 // 3 if cls.trans else -1
    T = H
    ldt = (T + 63) // 64 * 64
    perm = bool(cls.trans and cls.ln and T % 16 == 0)          # Builder.self_attention; the VAE's attention never permutes
    gelu = cls.epi == L.EPI_GEGLU
    ncols = tf if cls.trans else (N // 2 if gelu else N)
    odt = torch.float32 if cls.epi == L.EPI_F32 else torch.bfloat16
    t = dict.fromkeys(("a", "a1", "w", "bias", "rowvec", "res", "out", "out2", "ln_out", "ctr", "ln_in", "ln_g", "ln_c", "x0", "x1", "ws"))
    if dummy:
        mk = lambda fn: _DUMMY
    else:
        gen = torch.Generator(device=device).manual_seed(zlib.crc32(cls.id.encode()))
        mk = lambda fn: fn()
    rn = lambda *s: torch.randn(*s, generator=gen, device=device)
    b16 = lambda x: x.to(torch.bfloat16).contiguous()
    C0 = lay["C0"] or Cin
    if cls.ln:      # rows with their own means, as a residual stream has
        t["a"] = mk(lambda: b16(rn(Min, Cin) * 1.3 + 0.4 * rn(Min, 1)))
    else:
        t["a"] = mk(lambda: b16(rn(Min, C0)))
    if cls.src2:
        t["a1"] = mk(lambda: b16(rn(Min, Cin - C0)))
    if lay["k_alg"] and not dummy:
        t["a"][:, lay["k_alg"]:] = 0                            # im2col_small zero-pads its rows
    if cls.ln:
        def folded():
            gamma, beta = 1 + 0.2 * rn(Cin), 0.2 * rn(Cin)
            w = rn(N, Cin) / math.sqrt(Cin)
            b = None
            if gelu:    # WeightStore.geglu_ln
                w, b = Wm.pack_geglu(w, 0.1 * rn(N))
            wp, g, c = Wm.fold_layernorm(w, b, gamma, beta)    # WeightStore.qkv_ln: no bias
            x = t["a"].double()
            st = torch.stack([x.mean(-1), 1.0 / torch.sqrt(x.var(-1, unbiased=False) + LN_EPS)], -1).float().contiguous()
            return wp.contiguous(), g.contiguous(), c.contiguous(), st
        t["w"], t["ln_g"], t["ln_c"], t["ln_in"] = (_DUMMY,) * 4 if dummy else folded()
    elif taps == 4:
        t["w"] = mk(lambda: b16(Wm.pack_conv3x3_subpix(rn(N, Cin, 3, 3) / math.sqrt(9 * Cin))))   # [4][N][4 Cin]
    else:
        t["w"] = mk(lambda: b16(rn(N, Ktot) / math.sqrt(Ktot)))
        if not dummy:
            if lay["n_alg"]:
                t["w"][lay["n_alg"]:] = 0                       # WeightStore.small_conv_mfma: rows >= Cout are zero
            if lay["k_alg"]:
                t["w"][:, lay["k_alg"]:] = 0                    # WeightStore.conv_in_mfma
    if not cls.ln:                                              # (the folded forms carry theirs in ln_c)
        t["bias"] = mk(lambda: (0.1 * rn(N)).contiguous())
        if lay["n_alg"] and not dummy:
            t["bias"][lay["n_alg"]:] = 0
    if cls.temb:
        t["rowvec"] = mk(lambda: (0.2 * rn(N)).contiguous())    # one row of the time-embedding table, shared by every image
    if cls.res:
        t["res"] = mk(lambda: b16(rn(M, N)))
    if Cx:
        t["x0"] = mk(lambda: b16(rn(Min, lay["Cx0"])))
        if lay["two_x"]:
            t["x1"] = mk(lambda: b16(rn(Min, Cx - lay["Cx0"])))
    if cls.stats:
        t["ln_out"] = mk(lambda: torch.full((M * (N // 32 + 1), 2), float("nan"), device=device))
        t["ctr"] = mk(lambda: _shared("ctr", device, lambda: torch.zeros(65536, dtype=torch.int32, device=device)))
    orows = 4 * M if taps == 4 else M
    t["out"] = mk(lambda: torch.full((orows, ncols), float("nan"), device=device, dtype=odt))
    if cls.trans:
        t["out2"] = mk(lambda: torch.zeros(B, N - tf, ldt, device=device, dtype=torch.bfloat16))
    t["ws"] = mk(lambda: _shared("ws", device, lambda: torch.zeros(O.SPLITK_WS_BYTES, dtype=torch.uint8, device=device)))
    kw = dict(B=B, H=H, W=W, Cin=Cin, Ho=Ho, Wo=Wo, N=N, taps=taps, stride=cls.stride, pad=1 if taps in (9, 4) else 0,
              bias=t["bias"], rowvec=t["rowvec"], rowvec_bcast=t["rowvec"] is not None, residual=t["res"], epi=cls.epi,
              variant=cls.tile, splits=cls.splits, n_alg=lay["n_alg"], k_alg=lay["k_alg"], a1=t["a1"], C0=lay["C0"],
              ln_out=t["ln_out"], ln_counters=t["ctr"], ln_in=t["ln_in"], ln_g=t["ln_g"], ln_c=t["ln_c"])
    if cls.trans:
        kw.update(ldo=tf, out2=t["out2"], trans_from=tf, ldt=ldt, trans_perm=perm)
    if cls.epi == L.EPI_F32:
        kw.update(ldo=N)
    if taps == 4:
        kw.update(batch_z=4, zstrides=(0, N * 4 * Cin, 0, 0))
    else:
        assert cls.bz == 1
    if Cx:
        kw.update(fold=(t["x0"], t["x1"], lay["Cx0"], Cx))
    op = O.igemm(t["a"], t["w"], t["out"], **kw)
    O.Raw(op).splitk_ws = t["ws"]      # Builder.add: the program's own split-K workspace
    return Built(cls, op, geom, lay, t, perm)


# --------------------------------------------------------------------------- the arithmetic, twice

def _gather(A, B, H, W, Ho, Wo, stride, pad, taps):
    """[B Ho Wo][taps C] operand rows of the implicit GEMM in A's own type (zero outside the image); k = tap * C + c."""
    C = A.shape[-1]
    A4 = A.reshape(B, H, W, C)
    if taps == 1:
        return A4[:, ::stride, ::stride][:, :Ho, :Wo].reshape(B * Ho * Wo, C)
    Ap = F.pad(A4, (0, 0, pad, pad + stride, pad, pad + stride))
    cols = [Ap[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] for ky in range(3) for kx in range(3)]
    return torch.cat(cols, dim=-1).reshape(B * Ho * Wo, 9 * C)


def _subpix_rows(A, B, H, W, z):
    """Operand rows of output parity z = 2a + b of the sub-pixel form: taps (ty, tx) read source pixel (y - 1 + a + ty, x - 1 + b + tx)."""
    C = A.shape[-1]
    Ap = F.pad(A.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    a_, b_ = z // 2, z % 2
    return torch.cat([Ap[:, a_ + ty:a_ + ty + H, b_ + tx:b_ + tx + W] for ty in range(2) for tx in range(2)], dim=-1).reshape(B * H * W, 4 * C)


def _operand_rows(bt, conv):
    """[M][K] rows of the launch's A operand (second source and folded shortcut included), as ``conv`` (a cast) leaves them."""
    c, t = bt.cls, bt.t
    B, H, W, Ho, Wo = bt.geom
    A = conv(t["a"]) if t["a1"] is None else torch.cat([conv(t["a"]), conv(t["a1"])], dim=-1)
    g = _gather(A, B, H, W, Ho, Wo, c.stride, 1 if c.taps == 9 else 0, c.taps)
    if c.Cx:
        g = torch.cat([g, conv(t["x0"])] + ([conv(t["x1"])] if t["x1"] is not None else []), dim=-1)
    return g


def _split_outputs(bt, y, res):
    """Main output / transposed section of the full-width result y [M][N]."""
    c = bt.cls
    B, H, W, Ho, Wo = bt.geom
    if not c.trans:
        res["out"] = y
        return res
    tf = c.N * 2 // 3
    res["out"] = y[:, :tf]
    vt = y[:, tf:].reshape(B, H, c.N - tf).permute(0, 2, 1).contiguous()
    res["out2"] = O.permute_vt_keys(vt) if bt.perm else vt
    return res


def reference(bt):
    """{output name: float64 reference}; "out2" without its zero tail; with row statistics also "slots", "mean", "rstd"."""
    c, t = bt.cls, bt.t
    B, H, W, Ho, Wo = bt.geom
    d = lambda x: x.double()
    res = {}
    if c.taps == 4:
        out = torch.empty(B, 2 * H, 2 * W, c.N, dtype=torch.float64, device=t["a"].device)
        for z in range(4):
            y = _subpix_rows(d(t["a"]), B, H, W, z) @ d(t["w"][z]).t() + d(t["bias"])
            out[:, z // 2::2, z % 2::2] = y.reshape(B, H, W, c.N)
        res["out"] = out.reshape(-1, c.N)
        return res
    acc = _operand_rows(bt, d) @ d(t["w"]).t()
    if c.ln:
        st = d(t["ln_in"])
        acc = st[:, 1:2] * (acc - st[:, 0:1] * d(t["ln_g"])) + d(t["ln_c"])
    if t["bias"] is not None:
        acc = acc + d(t["bias"])
    if t["rowvec"] is not None:
        acc = acc + d(t["rowvec"])
    if t["res"] is not None:
        acc = acc + d(t["res"])
    if c.stats:
        s = acc.reshape(acc.shape[0], c.N // 32, 32)
        res["slots"] = torch.stack([s.sum(-1), (s * s).sum(-1)], dim=-1)
        res["mean"] = acc.mean(-1)
        res["rstd"] = 1.0 / torch.sqrt(acc.var(-1, unbiased=False) + LN_EPS)
    if c.epi == L.EPI_GEGLU:    # packed rows: 16 value columns, then their 16 gates (weights.pack_geglu)
        s = acc.reshape(acc.shape[0], c.N // 32, 2, 16)
        u, gt = s[:, :, 0], s[:, :, 1]
        acc = (u * (0.5 * gt * (1 + torch.erf(gt / math.sqrt(2))))).reshape(acc.shape[0], c.N // 2)
    return _split_outputs(bt, acc, res)


def yardstick(bt):
    """The same operands through torch's bf16 path: {"out"[, "out2"]: bf16 result}."""
    c, t = bt.cls, bt.t
    B, H, W, Ho, Wo = bt.geom
    bf = lambda x: x.to(torch.bfloat16)
    same = lambda x: x
    if c.taps == 4:
        out = torch.empty(B, 2 * H, 2 * W, c.N, dtype=torch.bfloat16, device=t["a"].device)
        for z in range(4):
            out[:, z // 2::2, z % 2::2] = F.linear(_subpix_rows(t["a"], B, H, W, z), t["w"][z], bf(t["bias"])).reshape(B, H, W, c.N)
        return {"out": out.reshape(-1, c.N)}
    if c.ln:    # normalise (fp32, then stored in bf16), project with the folded weights, add the folded constant
        xhat = bf(F.layer_norm(t["a"].float(), (c.Cin,), eps=LN_EPS))
        y = F.linear(xhat, t["w"], bf(t["ln_c"]))
    else:
        y = F.linear(_operand_rows(bt, same), t["w"], bf(t["bias"]))
    if t["rowvec"] is not None:
        y = y + bf(t["rowvec"])
    if t["res"] is not None:
        y = y + t["res"]
    if c.epi == L.EPI_GEGLU:
        s = y.reshape(y.shape[0], c.N // 32, 2, 16)
        y = (s[:, :, 0] * F.gelu(s[:, :, 1])).reshape(y.shape[0], c.N // 2)
    return _split_outputs(bt, y, {})


def outputs(bt):
    """{name: what the launch wrote}, shaped like ``reference``; "out2_tail": the zero padding of the V^T section."""
    c, t = bt.cls, bt.t
    B, H, W, Ho, Wo = bt.geom
    res = {"out": t["out"]}
    if c.taps == 4:     # the four parities are [z][B H W][N] slabs of an up-sampled [B][2H][2W][N] tensor
        res["out"] = t["out"].reshape(B, 2 * H, 2 * W, c.N).reshape(-1, c.N)
    if c.trans:
        res["out2"], res["out2_tail"] = t["out2"][:, :, :H], t["out2"][:, :, H:]
    if c.stats:
        M, ns = B * Ho * Wo, c.N // 32
        res["slots"] = t["ln_out"][:M * ns].reshape(M, ns, 2)
        res["mean"], res["rstd"] = t["ln_out"][M * ns:, 0], t["ln_out"][M * ns:, 1]
    return res
