"""The bytes of one ``mg_op`` per builder call, without a GPU.  A plain helper module for tests/test_op_wire_host.py (not collected),
with a ``__main__`` that writes the fixture tests/golden/op_wire.json.

``calls()`` runs every builder of marigold_amd/ops.py at least once: pointers are small plain integers (0x1000 * k), every integer
and float argument has a value of its own, and every optional argument is given in one call and left out in another.  The fixture
holds ``bytes(op).hex()`` per call - all 360 bytes, so it also pins that the slots no field names stay zero.  tests/golden/
program_digest.json covers the kinds the engine emits, in the forms it emits them; this one covers every kind, among them the
output-stage, evaluation and I/O kinds that no program holds.

    python -m tests.op_wire --write            regenerate tests/golden/op_wire.json
"""
import json
import os
import sys

from marigold_amd import _lib as L, ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "op_wire.json")


def P(k):
    return 0x1000 * k


def calls():
    """[(label, op)]: "<builder>/all" with every argument given, "<builder>/min" with every optional one left out."""
    c = []

    def add(label, op):
        assert label not in dict(c)
        c.append((label, op))

    add("igemm/all", O.igemm(P(1), P(2), P(3), B=2, H=3, W=4, Cin=5, Ho=6, Wo=7, N=8, taps=9, stride=10, pad=11, up=(12, 13), bias=P(4),
                             rowvec=P(5), residual=P(6), epi=14, ldo=15, out2=P(7), trans_from=16, ldt=20, batch_z=17, ldr=18, lda=19, ldw=22,
                             zstrides=(41, 42, 43, 44), scale=1.5, variant=21, rowvec_bcast=True, n_alg=24, k_alg=25, a1=P(8), C0=26, lda1=27,
                             ln_out=P(9), ln_in=P(10), ln_g=P(11), ln_c=P(12), ln_eps=2.5, sm_scale=3.5, sm_cols=29, c2=30, trans_perm=True,
                             ln_counters=0x123487654321, splits=33, fold=(P(13), P(14), 35, 34, 36, 37)))
    add("igemm/min", O.igemm(P(1), P(2), P(3), B=2, H=3, W=4, Cin=5, Ho=6, Wo=7, N=8))
    add("igemm/geglu,fold4", O.igemm(P(1), P(2), P(3), B=2, H=3, W=4, Cin=5, Ho=6, Wo=7, N=8, epi=L.EPI_GEGLU, fold=(P(13), None, 35, 34)))
    add("linear/all", O.linear(P(1), P(2), P(3), M=2, K=3, N=4, bias=P(4), ldo=5))
    add("linear/min", O.linear(P(1), P(2), P(3), M=2, K=3, N=4))
    add("conv3x3/all", O.conv3x3(P(1), P(2), P(3), B=2, H=3, W=4, C0=5, N=7, a1=P(7), C1=6, subpix=True, ss=P(8), silu=True, bias=P(4), rowvec=P(5),
                                 residual=P(6), lda0=8, lda1=9, ldo=10, ldr=11, ldw=12, rowvec_bcast=True, variant=14, wz=45, gn_part=P(9), gn_cpg=15,
                                 gn_slots=16))
    add("conv3x3/min", O.conv3x3(P(1), P(2), P(3), B=2, H=3, W=4, C0=5, N=7))
    add("rowgemm/all", O.rowgemm(P(1), P(2), P(3), M=2, K=3, N=4, form=L.RG_GEGLU, ldx=5, ldo=6, ldr=7, residual=P(4), ln_in=P(5), ln_out=P(6), vt=P(7),
                                 gn_ss=P(8), tokens=8, ldt=9, trans_from=10, waves=11, ln_eps=1.25, sm_cols=12, sm_scale=2.25, dbg=P(9), nsplit=13,
                                 xattn=P(10), xout=P(11)))
    add("rowgemm/min", O.rowgemm(P(1), P(2), P(3), M=2, K=3, N=4))
    add("rowgemm/xout_without_xattn", O.rowgemm(P(1), P(2), P(3), M=2, K=3, N=4, xout=P(11)))
    add("gn_stats/all", O.gn_stats(P(1), P(2), B=2, HW=3, C=4, chunks=5, groups=6, Ctot=7, coff=8, slot0=9, slots=10, gamma=P(3), beta=P(4), ss=P(5),
                                   counters=P(6), eps=1.5, x1=P(7), C1=11))
    add("gn_stats/min", O.gn_stats(P(1), P(2), B=2, HW=3, C=4, chunks=5, groups=6))
    add("gn_finalize", O.gn_finalize(P(1), P(2), P(3), P(4), B=2, C=3, groups=4, slots=5, HW=6, eps=1.5))
    add("gn_apply/all", O.gn_apply(P(1), P(2), P(3), B=2, HW=3, C=4, silu=True, x1=P(4), C0=5))
    add("gn_apply/min", O.gn_apply(P(1), P(2), P(3), B=2, HW=3, C=4, silu=False))
    add("gn_slab/all", O.gn_slab(P(1), P(2), P(3), B=2, HW=3, C=4, groups=5, gamma=P(4), beta=P(5), eps=1.5, silu=True, x1=P(6), C0=6))
    add("gn_slab/min", O.gn_slab(P(1), None, P(3), B=2, HW=3, C=4, groups=5, gamma=P(4), beta=P(5), eps=1.5))
    add("flash_attn64/all", O.flash_attn64(P(1), P(2), P(3), P(4), B=2, heads=3, Ntok=4, ldq=5, ldo=6, ldvt=7, sq=41, sk=42, svt=43, so=44, scale=0.5,
                                           variant=8, vt_perm=True, dbg=P(5), redo_thr=0.25, ws=P(6), ws_bytes=9 * 1024, split=10))
    add("flash_attn64/min", O.flash_attn64(P(1), P(2), P(3), P(4), B=2, heads=3, Ntok=4, ldq=5, ldo=6, ldvt=7, sq=41, sk=42, svt=43, so=44, scale=0.5))
    add("flash_attn512", O.flash_attn512(P(1), P(2), P(3), P(4), B=2, Ntok=3, ldq=4, ldo=5, ldvt=6, sq=41, sk=42, svt=43, so=44, scale=0.5))
    add("softmax_rows", O.softmax_rows(P(1), P(2), R=2, ncols=3, lds=4, ldp=5))
    add("sched_step/all", O.sched_step(P(1), P(2), P(3), P(4), n=2, cx=1.5, cm=2.5, cn=3.5))
    add("sched_step/min", O.sched_step(P(1), P(2), None, P(4), n=2, cx=1.5, cm=2.5))
    add("linear_small_m/all", O.linear_small_m(P(1), P(2), P(3), P(4), M=2, N=3, K=4, act_in=5, act_out=6, ldo=7))
    add("linear_small_m/min", O.linear_small_m(P(1), P(2), None, P(4), M=2, N=3, K=4))
    add("latent_1x1/all", O.latent_1x1(P(1), P(2), P(3), P(4), B=2, Ci=3, Co=4, HW=5, scale=1.5))
    add("latent_1x1/min", O.latent_1x1(P(1), P(2), P(3), P(4), B=2, Ci=3, Co=4, HW=5))
    add("im2col_small/all", O.im2col_small(P(1), P(2), P(3), B=2, H=3, W=4, C0=5, C1=6, Kp=7, bcast0=True, members_per_src0=8))
    add("im2col_small/min", O.im2col_small(P(1), None, P(3), B=2, H=3, W=4, C0=5, C1=6, Kp=7))
    add("conv3x3_head/all", O.conv3x3_head(P(1), P(2), P(3), P(4), P(5), B=2, H=3, W=4, C=5, Cout=6, ldo=7, silu=False))
    add("conv3x3_head/min", O.conv3x3_head(P(1), None, P(3), None, P(5), B=2, H=3, W=4, C=5, Cout=6))
    add("post_nchw/all", O.post_nchw(P(1), P(2), B=2, HW=3, Cout=4, ldi=5, post=L.POST_SCHED, scale=1.5, noise=P(3), cx=2.5, cm=3.5, cn=4.5))
    add("post_nchw/min", O.post_nchw(P(1), P(2), B=2, HW=3, Cout=4, ldi=5))
    add("ens_depth_stats", O.ens_depth_stats(P(1), P(2), P(3), E=2, HW=3))
    add("ens_depth_median/all", O.ens_depth_median(P(1), P(2), P(3), P(4), P(5), P(6), E=2, HW=3, reduction=1, has_shift=False))
    add("ens_depth_median/min", O.ens_depth_median(P(1), None, None, None, P(5), P(6), E=2, HW=3))
    add("ens_depth_norm/all", O.ens_depth_norm(P(1), P(2), P(3), HW=2, shift_invariant=False))
    add("ens_depth_norm/min", O.ens_depth_norm(P(1), None, P(3), HW=2))
    add("ens_normals/all", O.ens_normals(P(1), P(2), P(3), E=2, HW=3, reduction=1))
    add("ens_normals/min", O.ens_normals(P(1), P(2), None, E=2, HW=3))
    add("ens_iid/all", O.ens_iid(P(1), P(2), P(3), E=2, n=3, reduction=1))
    add("ens_iid/min", O.ens_iid(P(1), P(2), None, E=2, n=3))
    add("resize/u8", O.resize(P(1), P(2), P(3), planes=2, Hin=3, Win=4, Hout=5, Wout=6, mode=1, u8=True))
    add("resize/f32", O.resize(P(1), P(2), None, planes=2, Hin=3, Win=4, Hout=5, Wout=6, mode=2, u8=False))
    add("colorize/all", O.colorize(P(1), P(2), P(3), n=2, lo=1.5, hi=2.5))
    add("colorize/min", O.colorize(P(1), P(2), P(3), n=2))
    add("iid_vis/all", O.iid_vis(P(1), P(2), P(3), n=3, H=4, W=5, linear=(True, True, False), up_to_scale=(True, False, True)))
    add("iid_vis/min", O.iid_vis(P(1), P(2), None, n=2, H=4, W=5, linear=(False, False), up_to_scale=(False, False)))
    add("rgb_prep/all", O.rgb_prep(P(1), P(2), P(3), Hin=2, Win=3, Hout=4, Wout=5, mode="bicubic", hwc=False, out16=True, reciprocal=True))
    add("rgb_prep/min", O.rgb_prep(P(1), P(2), Hin=2, Win=3))
    add("rgb_prep/mode_number", O.rgb_prep(P(1), P(2), P(3), Hin=2, Win=3, Hout=4, Wout=5, mode=2))
    add("normals_vis", O.normals_vis(P(1), P(2), H=2, W=3))
    add("randn/all", O.randn(P(1), n=2, seed=(1 << 64) - 3, stream=(1 << 63) + 4, offset=5, words=True, out16=True))
    add("randn/min", O.randn(P(1), n=2, seed=3))
    add("eval_depth_ls/all", O.eval_depth_ls(P(1), P(2), P(3), P(4), P(5), H=37, W=53, disparity=True, max_res=20))
    add("eval_depth_ls/min", O.eval_depth_ls(P(1), P(2), P(3), P(4), P(5), H=37, W=53))
    add("eval_depth_metrics/all", O.eval_depth_metrics(P(1), P(2), P(3), P(4), P(5), P(6), H=2, W=3, disparity=True, min_depth=0.25, max_depth=80.5))
    add("eval_depth_metrics/min", O.eval_depth_metrics(P(1), P(2), P(3), None, P(5), P(6), H=2, W=3))
    add("eval_normals/all", O.eval_normals(P(1), P(2), P(3), P(4), P(5), HW=2, masked=False))
    add("eval_normals/min", O.eval_normals(P(1), P(2), P(3), None, P(5), HW=2))
    add("iidscore_prep/all", O.iidscore_prep(P(1), P(2), P(3), P(4), P(5), H=2, W=3, gamma=2.2))
    add("iidscore_prep/min", O.iidscore_prep(P(1), P(2), None, P(4), P(5), H=2, W=3))
    add("iidscore_psnr/all", O.iidscore_psnr(P(1), P(2), P(3), P(4), P(5), H=2, W=3, gamma=1.0 / 2.2, up_to_scale=True, write_psnr=False))
    add("iidscore_psnr/min", O.iidscore_psnr(P(1), P(2), None, P(4), P(5), H=2, W=3))
    add("iidscore_ssim/all", O.iidscore_ssim(P(1), P(2), P(3), P(4), P(5), H=2, W=3, gamma=(2.2, 1.0 / 2.2), up_to_scale=True))
    add("iidscore_ssim/min", O.iidscore_ssim(P(1), P(2), None, P(4), P(5), H=2, W=3))
    add("memset/all", O.memset(P(1), 2, 3))
    add("memset/min", O.memset(P(1), 2))
    add("copy", O.copy(P(1), P(2), 3))
    return c


def built():
    """{label: hex of the op's 360 bytes}."""
    return {label: bytes(op).hex() for label, op in calls()}


def main(argv):
    if argv == ["--write"]:
        got = built()
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in got.items()) + "\n}\n")   # (a call per line)
        print(f"{FIXTURE}: {len(got)} ops of {len({op.kind for _, op in calls()})} kinds")
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
