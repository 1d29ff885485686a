"""Host checks of the float64 op reference (tests/op_reference.py), no GPU: it decodes every op of the production VAE encoder
program and resolves every pointer those ops read; its arithmetic agrees with independent torch formulations for every form it
covers; it runs over a whole (tiny) program."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import op_reference as R
from marigold_amd import _lib as L, ops, weights as Wm


def _res(*ts):
    return R.make_resolver(list(ts))


def _check(op, ts, want, tol=1e-9):
    """decode + expected of ``op`` over CPU tensors ``ts``, each output's checked elements against ``want`` (float64)."""
    resolve = _res(*ts)
    spec = R.decode(op, resolve, "unit")
    got = R.expected(spec, R.load_inputs(spec, resolve))
    for nm, (ref, idx) in got.items():
        w = R.pick(want[nm], idx)
        assert w.shape[-1] >= ref.shape[-1]
        w = w[..., :ref.shape[-1]]
        err = float((ref - w.double()).abs().max()) / max(float(w.abs().max()), 1e-30)
        assert err < tol, (nm, err)
    return spec


def _bf(x):
    return x.to(torch.bfloat16)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("stride,pad", [(1, 1), (2, 0)])
def test_igemm_conv_matches_conv2d(stride, pad):
    g = torch.Generator().manual_seed(stride)
    B, H, W, C, N = 2, 9, 11, 64, 96
    x, w = _bf(torch.randn(B, C, H, W, generator=g)), _bf(torch.randn(N, C, 3, 3, generator=g) / 24)
    bias, temb = torch.randn(N, generator=g), torch.randn(B, N, generator=g)
    xin = F.pad(x.double(), (0, 1, 0, 1)) if pad == 0 else x.double()
    ref = F.conv2d(xin, w.double(), bias.double(), stride=stride, padding=pad) + temb.double()[:, :, None, None]
    Ho, Wo = ref.shape[-2:]
    res = _bf(torch.randn(B, Ho * Wo, N, generator=g))
    ref = _nhwc(ref).reshape(B * Ho * Wo, N) + res.reshape(-1, N).double()
    xd, wd, out = _nhwc(x), Wm.pack_conv3x3(w).to(torch.bfloat16), torch.zeros(B * Ho * Wo, N, dtype=torch.bfloat16)
    op = ops.igemm(xd, wd, out, B=B, H=H, W=W, Cin=C, Ho=Ho, Wo=Wo, N=N, taps=9, stride=stride, pad=pad, bias=bias, rowvec=temb,
                   residual=res)
    _check(op, [xd, wd, out, bias, temb, res], {"out": ref[None]})


def test_igemm_dense_transposed_section_and_batched_f32():
    g = torch.Generator().manual_seed(3)
    T, C, ldt = 40, 64, 64
    x, w, b = _bf(torch.randn(T, C, generator=g)), _bf(torch.randn(3 * C, C, generator=g) / 8), torch.randn(3 * C, generator=g)
    y = F.linear(x.double(), w.double(), b.double())
    qk, vt = torch.zeros(T, 2 * C, dtype=torch.bfloat16), torch.zeros(1, C, ldt, dtype=torch.bfloat16)
    op = ops.igemm(x, w, qk, B=1, H=T, W=1, Cin=C, Ho=T, Wo=1, N=3 * C, ldo=2 * C, bias=b, out2=vt, trans_from=2 * C, ldt=ldt)
    want_vt = torch.zeros(1, C, ldt, dtype=torch.float64)
    want_vt[0, :, :T] = y[:, 2 * C:].t()
    _check(op, [x, w, b, qk, vt], {"out": y[None, :, :2 * C], "out2": want_vt})
    # scores of two images in one batched F32 launch: S_z = s * Q_z K_z^T
    Z = 2
    q, k = _bf(torch.randn(Z, T, C, generator=g)), _bf(torch.randn(Z, T, C, generator=g))
    sc = torch.zeros(Z, T, T, dtype=torch.float32)
    op = ops.igemm(q, k, sc, B=1, H=T, W=1, Cin=C, Ho=T, Wo=1, N=T, epi=L.EPI_F32, ldo=T, batch_z=Z,
                   zstrides=(T * C, T * C, T * T, 0), scale=0.125)
    _check(op, [q, k, sc], {"out": 0.125 * q.double() @ k.double().transpose(1, 2)})


def test_groupnorm_forms_match_group_norm():
    g = torch.Generator().manual_seed(4)
    B, H, W, C, G, eps = 2, 6, 10, 64, 32, 1e-6
    x = _bf(torch.randn(B, C, H, W, generator=g) * 2 + 0.5)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    ref = F.group_norm(x.double(), G, gamma.double(), beta.double(), eps)
    xd = _nhwc(x).reshape(B, H * W, C)
    ss, part, cnt = torch.zeros(B, 2, C), torch.zeros(B, 4, G, 2), torch.zeros(B, dtype=torch.int32)
    op = ops.gn_stats(xd, part, B=B, HW=H * W, C=C, chunks=4, groups=G, gamma=gamma, beta=beta, ss=ss, counters=cnt, eps=eps)
    xg = x.double().reshape(B, G, -1)
    sc = (xg.var(-1, unbiased=False) + eps).rsqrt().repeat_interleave(C // G, 1) * gamma.double()
    sh = beta.double() - xg.mean(-1).repeat_interleave(C // G, 1) * sc
    _check(op, [xd, part, gamma, beta, ss, cnt], {"ss": torch.stack([sc, sh], 1)})
    # finalize from (sum, sum of squares) partials over slots
    part = torch.stack([xg.reshape(B, G, 3, -1).sum(-1), (xg.reshape(B, G, 3, -1) ** 2).sum(-1)], -1).permute(0, 2, 1, 3).float().contiguous()
    op = ops.gn_finalize(part, gamma, beta, ss, B=B, C=C, groups=G, slots=3, HW=H * W, eps=eps)
    _check(op, [part, gamma, beta, ss], {"ss": torch.stack([sc, sh], 1)}, tol=1e-5)
    ssf = torch.stack([sc, sh], 1).float()
    out = torch.zeros_like(xd)
    op = ops.gn_apply(xd, ssf, out, B=B, HW=H * W, C=C, silu=True)
    _check(op, [xd, ssf, out], {"out": F.silu(_nhwc(ref).reshape(B, H * W, C))}, tol=1e-5)


def test_conv3x3_fused_norm_and_gn_table():
    g = torch.Generator().manual_seed(5)
    B, H, W, C, N = 2, 7, 9, 64, 128
    x, w = _bf(torch.randn(B, C, H, W, generator=g)), _bf(torch.randn(N, C, 3, 3, generator=g) / 24)
    bias = torch.randn(N, generator=g)
    ss = torch.stack([1 + 0.3 * torch.randn(B, C, generator=g), 0.3 * torch.randn(B, C, generator=g)], 1)
    h = F.silu(x.double() * ss[:, 0, :, None, None].double() + ss[:, 1, :, None, None].double()).to(torch.bfloat16).double()
    res = _bf(torch.randn(B * H * W, N, generator=g))
    ref = _nhwc(F.conv2d(h, w.double(), bias.double(), padding=1)).reshape(-1, N) + res.double()
    xd, wd, out = _nhwc(x), Wm.pack_conv3x3(w).to(torch.bfloat16), torch.zeros(B * H * W, N, dtype=torch.bfloat16)
    table = torch.zeros(B, 3, N // 4, 2)
    op = ops.conv3x3(xd, wd, out, B=B, H=H, W=W, C0=C, N=N, ss=ss, silu=True, bias=bias, residual=res, gn_part=table, gn_cpg=4,
                     gn_slots=3)
    spec = _check(op, [xd, wd, out, bias, ss, res, table], {"out": ref})
    assert "gn_table" in spec.writes
    y = torch.randn(B * H * W, N, generator=g).to(torch.bfloat16)
    t = R.gn_table_reference(spec, y)
    yg = y.double().reshape(B, H * W, N // 4, 4)
    assert torch.allclose(t[..., 0], yg.sum((1, 3))) and torch.allclose(t[..., 1], (yg ** 2).sum((1, 3)))


def test_softmax_im2col_post():
    g = torch.Generator().manual_seed(6)
    Rn, n, ld = 300, 50, 64
    s = torch.randn(Rn, ld, generator=g) * 3
    p = torch.zeros(Rn, ld, dtype=torch.bfloat16)
    want = torch.zeros(Rn, ld, dtype=torch.float64)
    want[:, :n] = torch.softmax(s[:, :n].double(), -1)
    _check(ops.softmax_rows(s, p, R=Rn, ncols=n, lds=ld, ldp=ld), [s, p], {"P": want})
    B, H, W, C, Kp = 2, 5, 7, 3, 32
    x = torch.randn(B, C, H, W, generator=g)
    col = torch.zeros(B * H * W, Kp, dtype=torch.bfloat16)
    u = F.unfold(x.double(), 3, padding=1).reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
    want = torch.zeros(B * H * W, Kp, dtype=torch.float64)
    want[:, :9 * C] = u.to(torch.bfloat16).double()
    _check(ops.im2col_small(x, None, col, B=B, H=H, W=W, C0=C, C1=0, Kp=Kp), [x, col], {"out": want})
    t = torch.randn(B * H * W, 8, generator=g)
    o = torch.zeros(B, 4, H * W)
    want = (t[:, :4].double().reshape(B, H * W, 4).permute(0, 2, 1)) * 0.18215
    _check(ops.post_nchw(t, o, B=B, HW=H * W, Cout=4, ldi=8, scale=0.18215), [t, o], {"out": want}, tol=1e-7)


def test_unknown_forms_raise():
    x = torch.zeros(64, 64, dtype=torch.bfloat16)
    for op in (ops.sched_step(x, x, None, x, n=4, cx=1.0, cm=1.0),
               ops.igemm(x, x, x, B=1, H=64, W=1, Cin=64, Ho=64, Wo=1, N=64, epi=L.EPI_GEGLU)):
        with pytest.raises(R.Unsupported):
            R.decode(op, _res(x), "unit")
    op = ops.igemm(x, x, x, B=1, H=64, W=1, Cin=64, Ho=64, Wo=1, N=64)
    with pytest.raises(KeyError):
        R.decode(op, _res(), "unit")     # an operand that resolves to nothing


def _vae_encode(cfg, H, W, sd):
    from marigold_amd.modules import AutoencoderKLHIP
    vae = AutoencoderKLHIP(sd, cfg).dry()
    seq, _, _ = vae._program("encode", 1, H, W)
    return vae, seq, R.make_resolver([seq.keep, vae.ws.cache, vae.pool.all])


def test_vae_encode_768_every_op_decodes_and_resolves():
    from marigold_amd.arch import VAEConfig, vae_param_shapes
    cfg = VAEConfig()
    vae, seq, resolve = _vae_encode(cfg, 768, 768, {k: torch.zeros(s) for k, s in vae_param_shapes(cfg).items()})
    kinds = set()
    for op, lab in zip(seq.ops, seq.labels):
        spec = R.decode(op, resolve, lab)
        for r in list(spec.reads.values()) + list(spec.writes.values()):
            R.view(resolve, r)           # in bounds of the tensor it resolves to
        kinds.add(spec.name)
    assert len(seq.ops) == 70 and kinds >= {"igemm", "conv3x3", "gn_stats", "gn_finalize", "gn_apply", "softmax_rows"}


def test_tiny_vae_encode_whole_program_on_random_buffers():
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_VAE
    vae, seq, resolve = _vae_encode(TINY_VAE, 64, 96, syn.synthetic_vae_state_dict(TINY_VAE))
    g = torch.Generator().manual_seed(0)
    for t in vae.pool.all:               # finite values whichever type a buffer is read as (bf16 halves of finite fp32)
        t.view(torch.bfloat16).copy_(torch.randn(t.numel() // 2, generator=g))
    for op, lab in zip(seq.ops, seq.labels):
        spec = R.decode(op, resolve, lab)
        for nm, (ref, _) in R.expected(spec, R.load_inputs(spec, resolve)).items():
            assert torch.isfinite(ref).all(), (lab, nm)


def test_igemm_folded_shortcut_matches_two_convs():
    g = torch.Generator().manual_seed(7)
    B, H, W, C, Cx0, Cx1, N = 1, 6, 8, 64, 64, 64, 64
    h, xs = _bf(torch.randn(B, C, H, W, generator=g)), _bf(torch.randn(B, Cx0 + Cx1, H, W, generator=g))
    w, wsc = _bf(torch.randn(N, C, 3, 3, generator=g) / 24), _bf(torch.randn(N, Cx0 + Cx1, 1, 1, generator=g) / 11)
    bias = torch.randn(N, generator=g)
    ref = F.conv2d(h.double(), w.double(), bias.double(), padding=1) + F.conv2d(xs.double(), wsc.double())
    wd = torch.cat([Wm.pack_conv3x3(w).to(torch.bfloat16), wsc.reshape(N, -1)], 1).contiguous()
    x0, x1 = _nhwc(xs[:, :Cx0]), _nhwc(xs[:, Cx0:])
    hd, out = _nhwc(h), torch.zeros(B * H * W, N, dtype=torch.bfloat16)
    op = ops.igemm(hd, wd, out, B=B, H=H, W=W, Cin=C, Ho=H, Wo=W, N=N, taps=9, stride=1, pad=1, bias=bias,
                   fold=(x0, x1, Cx0, Cx0 + Cx1))
    _check(op, [hd, wd, out, bias, x0, x1], {"out": _nhwc(ref).reshape(1, -1, N)})
