#!/usr/bin/env python3
"""Generator of flash4w.inc: the whole key loop of flash attention at head width 64 as ONE hand-placed instruction stream
(flash4w.hip: 64 queries per wave, 64-key tiles, two waves per SIMD).

Why a generator: round 4's micro-benchmark (tools/ubench/coissue2.hip, profiles/r4_ubench_flash_like_waves.log) shows that on
gfx950 the softmax's VALU work and the MFMAs only overlap when they are interleaved instruction by instruction - three waves per
SIMD that alternate whole phases (what hipcc emits for flash_attn64_v25) reach 75 % of the interleaved stream's rate, and the
compiled kernel, with its `s_waitcnt lgkmcnt(0)` in front of every MFMA and `s_nop 10` behind every score tile, about half.
A single wave, though, is bound by its own issue (one instruction at a time: ~9 cycles per v_exp_f32 / v_cvt_pk_bf16_f32, ~5 per
v_add_f32, ~8 per MFMA: 1 600-1 680 cycles per tile against 1 024 of MFMA time, the first form of this file), so the stream is
kept to 192 VGPRs + 64 AGPRs and two workgroups share a CU.

The wave's 64 queries are two blocks q of 32; a key tile is two halves of 32 keys = four groups g of 16.  The scores live in
two register sets of 2 x 16: X = v[128:159] (half 0 of a tile), Y = v[160:191] (half 1) - physical registers, single ones are
VALU operands.  One iteration t = one tile = 32 MFMAs in eight groups SG0..SG7 of four:
    SG0-3 (half 0):  two QK^T MFMAs of tile t's half 1 into Y (q0: SG0 / SG1, q1: SG2 / SG3), two P V MFMAs of X's groups
    SG4-7 (half 1):  two QK^T MFMAs of tile t + 1's half 0 into X,                              two P V MFMAs of Y's groups
  * a QK^T chain's first k-step takes -reference as its C operand: p = exp2(s) needs no subtraction;
  * P(q, g) - eight probabilities per lane - is packed IN PLACE into the first four registers of its own eight scores, by the
    twenty VALU instructions (8 v_exp_f32, 8 v_add_f32 for the row sums, 4 v_cvt_pk_bf16_f32) placed five behind each MFMA of
    the group BEFORE the one whose P V MFMAs read it (a VALU result needs wait states before an MFMA may read it as an operand:
    nothing inserts them in an asm stream; the QK^T pair in front of every P V pair provides them);
  * the four K fragments of a half and the four V^T fragments of two groups stay in registers for both query blocks (half the
    LDS traffic per MFMA of a 32-query wave), reloaded by ds_read_b128 as soon as their last MFMA has issued, every wait a
    counted lgkmcnt;
  * ring slot t of four 16 KB slots holds what iteration t reads: K rows 64 t + 32 ... 64 t + 95 (tile t's half 1, tile t + 1's
    half 0) and V^T tile t; the LDS-DMA pieces of slot t + 3 go out behind the first MFMAs of SG1-SG4; one barrier per tile,
    behind SG6: slot t + 1 has landed for every wave and nobody reads slot t - 1 any more.

Stream = ENTRY, LOOP x cnt {FULL}, NODMA(vmcnt 4), NODMA(vmcnt 0), LAST        (cnt = nkt - 3 >= 1)
"""
import sys
from collections import namedtuple

from asmstream import MFMA_RESULT_TAIL, Stream, define, renamed

X = {0: 128, 1: 144}      # score set of a tile's half 0: query block -> first register
Y = {0: 160, 1: 176}


def vt(b, n):
    return f"v[{b}:{b + n - 1}]"


def vgroup(R, la, lb):
    """exp2, row sums and packing of the eight scores in v[R : R + 7]; P ends up in v[R : R + 3].  A transcendental's result is
    never read by the next instruction (asmstream.check_hazards)."""
    r = [f"v{R + j}" for j in range(8)]
    return [
        f"v_exp_f32 {r[0]}, {r[0]}",
        f"v_exp_f32 {r[1]}, {r[1]}",
        f"v_add_f32 {la}, {la}, {r[0]}",
        f"v_exp_f32 {r[2]}, {r[2]}",
        f"v_add_f32 {lb}, {lb}, {r[1]}",
        f"v_exp_f32 {r[3]}, {r[3]}",
        f"v_add_f32 {la}, {la}, {r[2]}",
        f"v_cvt_pk_bf16_f32 {r[0]}, {r[0]}, {r[1]}",
        f"v_exp_f32 {r[4]}, {r[4]}",
        f"v_add_f32 {lb}, {lb}, {r[3]}",
        f"v_cvt_pk_bf16_f32 {r[1]}, {r[2]}, {r[3]}",
        f"v_exp_f32 {r[5]}, {r[5]}",
        f"v_add_f32 {la}, {la}, {r[4]}",
        f"v_exp_f32 {r[6]}, {r[6]}",
        f"v_add_f32 {lb}, {lb}, {r[5]}",
        f"v_exp_f32 {r[7]}, {r[7]}",
        f"v_cvt_pk_bf16_f32 {r[2]}, {r[4]}, {r[5]}",
        f"v_add_f32 {la}, {la}, {r[6]}",
        f"v_add_f32 {lb}, {lb}, {r[7]}",
        f"v_cvt_pk_bf16_f32 {r[3]}, {r[6]}, {r[7]}",
    ]


# ---------------------------------------------------------------------------------------------------------------------------
# The same loop on v_mfma_f32_16x16x32 (round 6, FA4W16_ASM; flash4w.hip, variant 27).  Why: the chip is power-limited under
# matrix load and this kernel's operands are on the CU (registers / LDS) - the regime in which a wave-tile step on 16x16x32
# MFMAs ran 14 % faster than on 32x32x16 (tools/ubench/mfma_shape_asm.hip, profiles/r6_mfma_shape.log).
#
# The wave's 64 queries are FOUR blocks q of 16; a half (32 keys) is ONE k-step of the P V product and two key blocks kb of the
# scores.  Score sets: X16 = v[128:159], Y16 = v[160:191], eight registers per query block: [kb 0: r0-r3 | kb 1: r0-r3] - lane
# (query l15, key group kq = lane >> 4), register r of block kb = the score of MFMA row 4 kq + r, whose key the K fragment's
# row map chooses (flash4w.hip: position 8 kq + 4 kb + r of the half in the permuted V^T order), so that the eight packed
# probabilities of a lane ARE its 8 consecutive k values of the P V MFMA's B operand.  One iteration = 72 MFMAs in eight groups
# SG0..SG7 of eight (ten); SG s of a half = (query pair qp = s >> 1, pair = s & 1):
#     four QK^T MFMAs:  queries 2 qp, 2 qp + 1  x  d-steps 0, 1  of key block kb = pair          (K fragments kf[2 pair + ds])
#     four P V MFMAs:   queries 2 qp, 2 qp + 1  x  d blocks 2 pair, 2 pair + 1                    (V^T fragments vf[2 pair + j])
#   so the fragments of `pair` are used in SG `pair` and SG 2 + `pair` of a half and reloaded behind the second use, as in the
#   32x32x16 stream; order QK, PV, QK, PV ...: the two d-steps of a score block are four MFMAs apart, a query block's first P V MFMA
#   has at least one MFMA between itself and the packing of its P;
#   VALU (12 instructions per query block: 8 v_exp_f32, 4 v_cvt_pk; Bresenham over the group's MFMAs): SG0 / SG1 of a half pack P of
#   its queries 2 / 3, SG2 / SG3 P of queries 0 / 1 of the NEXT half - whose scores SG0 / SG1 have just finished;
#   the `pair` = 0 groups carry two more MFMAs: the row sums of their two query blocks (below).
X16 = {q: 128 + 8 * q for q in range(4)}
Y16 = {q: 160 + 8 * q for q in range(4)}


# Row sums on the matrix pipe: one MFMA of P against ones per (query block, half) - every row of the 16 x 16 result is the sum over
# the half's 32 keys of the lane's query - instead of eight v_add_f32 per query block.  With the adds on the VALU this stream was a tie
# with the 32x32x16 one (2 936 cycles per wave-tile at 1.74-1.84 GHz against 2 408 at 1.6: a 16-cycle MFMA costs the wave the same ~8
# issue cycles as a 32-cycle one, and the kernel is issue-bound); without them 2 589 cycles at 1.8 GHz, the matrix pipe 89 % busy
# (72 MFMAs per wave-tile): 1 201 / 1 278 TFLOP/s (whole blocks / key-split) against 1 130 / 1 193 at E = 10, 9 216 tokens
# (profiles/r6_flash_mfma16.log).  The same trade LOST in the 32x32x16 stream (a third 32-cycle MFMA per pair, round 4).
def vgroup_noadd(R):
    """exp2 and packing only (the row sums are an MFMA against ones)"""
    r = [f"v{R + j}" for j in range(8)]
    return [f"v_exp_f32 {r[0]}, {r[0]}", f"v_exp_f32 {r[1]}, {r[1]}", f"v_exp_f32 {r[2]}, {r[2]}",
            f"v_cvt_pk_bf16_f32 {r[0]}, {r[0]}, {r[1]}", f"v_exp_f32 {r[3]}, {r[3]}", f"v_exp_f32 {r[4]}, {r[4]}",
            f"v_cvt_pk_bf16_f32 {r[1]}, {r[2]}, {r[3]}", f"v_exp_f32 {r[5]}, {r[5]}", f"v_exp_f32 {r[6]}, {r[6]}",
            f"v_exp_f32 {r[7]}, {r[7]}", f"v_cvt_pk_bf16_f32 {r[2]}, {r[4]}, {r[5]}", f"v_cvt_pk_bf16_f32 {r[3]}, {r[6]}, {r[7]}"]


KOFF0, KOFF1, VOFF = 0, 4096, 8192     # inside a slot: K of this tile's half 1, K of the next tile's half 0, V^T

# What distinguishes the two forms of the loop.  An iteration is eight groups SG i = (half = i >> 2, qp = (i >> 1) & 1, pair = i & 1)
# of QK^T MFMAs (two chain steps x the group's query blocks, scores of `nxt`) interleaved with as many P V MFMAs (query blocks x two
# V^T fragments, probabilities of `cur`); both use the fragments kf / vf [2 pair], [2 pair + 1].
#   nq        query blocks per group: blocks nq qp ... nq qp + nq - 1
#   X, Y      the score sets: query block -> first register
#   qk_dst    (set, q, pair) -> the score registers a QK^T MFMA accumulates into
#   qk_step   (pair, step) -> the step of the score chain (operand q<q><step>; step 0 takes -reference, %[ng<q>], as C)
#   pv_src    (set, q, pair) -> the packed probabilities a P V MFMA reads
#   o_idx     (pair, j) -> the output block of V^T fragment vf[2 pair + j]
#   kad       address operands ad<..> of the four K fragments
#   vad       per V^T fragment: (address operand, offset) for an iteration's first half and for its second
#   bump      the address operands that move on to the next ring slot
#   valu      (i, last) -> the VALU instructions spread over group i's MFMAs;  pre: those in front of the loop
#   rowsum_mfma   the row sums ride on the matrix pipe: one more MFMA (P against ones) per query block in the pair-0 groups
Form = namedtuple("Form", "macro label mfma nq X Y qk_dst qk_step pv_src o_idx kad vad bump valu pre rowsum_mfma")


def valu32(i, last):
    """P of the group whose P V MFMAs come in the NEXT group of MFMAs"""
    j = i + 1
    if j < 8:
        jh, jq, jp = j >> 2, (j >> 1) & 1, j & 1
        return vgroup((X if jh == 0 else Y)[jq] + 8 * jp, f"%[l{jq}0]", f"%[l{jq}1]")
    return [] if last else vgroup(X[0], "%[l00]", "%[l01]")       # (q0, first group) of the next tile


def valu16(i, last):
    half, s = i >> 2, i & 3
    cur, nxt = (X16, Y16) if half == 0 else (Y16, X16)
    if s < 2:
        return vgroup_noadd(cur[2 + s])
    return [] if last and half == 1 else vgroup_noadd(nxt[s - 2])


FA32 = Form("FA4W_ASM", ".Lfa4w_loop%=", "v_mfma_f32_32x32x16_bf16", 1, X, Y,
            qk_dst=lambda S, q, pair: vt(S[q], 16), qk_step=lambda pair, step: 2 * pair + step,
            pv_src=lambda S, q, pair: vt(S[q] + 8 * pair, 4), o_idx=lambda pair, j: j,
            kad=("0", "1", "2", "3"),
            vad=([("0", VOFF), ("0", VOFF + 4096), ("1", VOFF), ("1", VOFF + 4096)],
                 [("2", VOFF), ("2", VOFF + 4096), ("3", VOFF), ("3", VOFF + 4096)]),
            bump=("0", "1", "2", "3"), valu=valu32, pre=vgroup(X[0], "%[l00]", "%[l01]"), rowsum_mfma=False)
FA16 = Form("FA4W16_ASM", ".Lfa4w16_loop%=", "v_mfma_f32_16x16x32_bf16", 2, X16, Y16,
            qk_dst=lambda S, q, pair: vt(S[q] + 4 * pair, 4), qk_step=lambda pair, step: step,
            pv_src=lambda S, q, pair: vt(S[q], 4), o_idx=lambda pair, j: 2 * pair + j,
            kad=("k0", "k1", "k2", "k3"),
            vad=([("v0", VOFF + 2048 * j) for j in range(4)], [("v1", VOFF + 2048 * j) for j in range(4)]),
            bump=("k0", "k1", "k2", "k3", "v0", "v1"), valu=valu16, pre=vgroup_noadd(X16[0]) + vgroup_noadd(X16[1]),
            rowsum_mfma=True)

# Queue tags.  LDS: the fragment buffer a ds_read_b128 fills (kf0-3, vf0-3).  VMEM: S<n> = the four LDS-DMA pieces of ring slot
# t + n.  The stream is entered with slots 0, 1, 2 in flight: flash4w.hip issues two reference pieces and then, `for (int sl = 0;
# sl < 3; ++sl)`, four pieces per slot, and its `s_waitcnt vmcnt(12)` + barrier in front of the stream leave exactly those twelve.
# An iteration is entered with slots t + 1, t + 2 in flight, issues slot t + 3 and waits for t + 1:
NEXT = {"S2": "S1", "S3": "S2"}
DMA = {1: ("vk0", "srk", "sok", 0), 2: ("vk1", "srk", "sok", 4096), 3: ("vv0", "srv", "sov", 8192), 4: ("vv1", "srv", "sov", 12288)}


def read(st, buf, ad, off):
    assert buf not in st.ldsq and len(st.ldsq) < 15, (buf, st.ldsq)      # (this generator's own bound: one wait per buffer)
    st.lds(f"ds_read_b128 %[{buf}], %[ad{ad}] offset:{off}", buf)


def entry_reads(st, F, pair):
    """The fragments SG `pair` of an iteration starts from, out of the slot the address registers point at."""
    for b in (2 * pair, 2 * pair + 1):
        read(st, f"kf{b}", F.kad[b], KOFF0)
    for b in (2 * pair, 2 * pair + 1):
        read(st, f"vf{b}", *F.vad[0][b])


def drain(st):
    if st.ldsq:
        st.wait_lds()


def block(F, kind, lds, vm):
    """kind: 'full' (LDS-DMA of slot t + 3) | 'nodma' | 'last'; lds, vm: the entry queues.  -> the resolved stream"""
    st = Stream(lds, vm)
    last = kind == "last"
    dma = DMA if kind == "full" else {}
    for i in range(8):
        half, qp, pair = i >> 2, (i >> 1) & 1, i & 1
        cur, nxt = (F.X, F.Y) if half == 0 else (F.Y, F.X)     # scores being consumed / produced (this tile's half 1, the next tile's half 0)
        qs = range(F.nq * qp, F.nq * qp + F.nq)
        tail_half = last and half == 1                         # no next tile: no QK^T MFMAs
        qk, pv = [], []
        if not tail_half:
            for step in (0, 1):
                for q in qs:
                    ks, D = F.qk_step(pair, step), F.qk_dst(nxt, q, pair)
                    C = f"%[ng{q}]" if ks == 0 else D
                    qk.append((f"{F.mfma} {D}, %[kf{2 * pair + step}], %[q{q}{ks}], {C}", f"kf{2 * pair + step}"))
        for q in qs:
            for j in (0, 1):
                o = F.o_idx(pair, j)
                pv.append((f"{F.mfma} %[o{q}{o}], %[vf{2 * pair + j}], {F.pv_src(cur, q, pair)}, %[o{q}{o}]", f"vf{2 * pair + j}"))
        # QK, PV, QK, PV ...: the steps of one score accumulator are not back to back, every P V MFMA has an MFMA and VALU
        # instructions between the packing of its P and itself
        mf = [x for pr in zip(qk, pv) for x in pr] if qk else pv
        if F.rowsum_mfma and pair == 0:     # P against ones: every row of the block = the sum
            mf += [(f"{F.mfma} %[ls{q}], %[ones], {vt(cur[q], 4)}, %[ls{q}]", None) for q in qs]
        va = F.valu(i, last)
        n = len(mf)
        for k, (text, buf) in enumerate(mf):
            first = k == 0
            if first and i in dma:
                st.op(f"s_add_u32 m0, %[mb], {dma[i][3]}")
            if tail_half and first:
                st.op("s_nop 4")      # (no QK^T MFMA in front of this P V MFMA: the wait states behind the VALU that packed its P)
            if buf is not None:
                st.wait_lds(buf, "skip")      # (a buffer's second MFMA finds it waited for already)
            st.op(text)
            if first and i in dma:
                vo, srd, so, _ = dma[i]
                st.vmem(f"buffer_load_dwordx4 %[{vo}], %[{srd}], %[{so}] offen lds", "S3")
                if i == 2:
                    st.op("s_add_u32 %[sok], %[sok], %[kst]")
                if i == 4:
                    st.op("s_add_u32 %[sov], %[sov], 128")
                    st.op("s_add_u32 %[mb], %[mb], 0x4000")
                    st.op("s_and_b32 %[mb], %[mb], 0xffff")
            for text2 in va[(len(va) * k) // n:(len(va) * (k + 1)) // n]:      # Bresenham over the group's MFMAs
                st.op(text2)
            # fragment reloads for the iteration's second half, as soon as the buffer's last MFMA has issued (SG2: pair 0, SG3: pair 1)
            if i in (2, 3):
                if qk and k == 2 * len(qk) - 2 and not last:                   # behind the group's last QK^T MFMA
                    for b in (2 * pair, 2 * pair + 1):
                        read(st, f"kf{b}", F.kad[b], KOFF1)
                if k == (2 * len(pv) - 1 if qk else len(pv) - 1):              # behind its last P V MFMA
                    for b in (2 * pair, 2 * pair + 1):
                        read(st, f"vf{b}", *F.vad[1][b])
        if i == 6 and not last:
            # slot t + 1 has landed for everybody, slot t - 1 is free; the address registers move on
            drain(st)
            st.wait_vm("S1")
            st.op("s_barrier")
            for jj in F.bump:
                st.op(f"v_add_u32 %[ad{jj}], 0x4000, %[ad{jj}]")
                st.op(f"v_and_b32 %[ad{jj}], 0xffff, %[ad{jj}]")
            entry_reads(st, F, 0)
        if i == 7 and not last:
            entry_reads(st, F, 1)
    if last:
        drain(st)
        st.lines += MFMA_RESULT_TAIL
    return st


def stream(F):
    """ENTRY, LOOP x cnt {FULL}, NODMA, NODMA, LAST -> (all lines, the lines of FULL)"""
    st = Stream(vm=["S0"] * 4 + ["S1"] * 4 + ["S2"] * 4)
    st.wait_lds()
    for t in F.pre:
        st.op(t)
    st.wait_vm("S0")
    st.op("s_barrier")
    entry_reads(st, F, 0)
    entry_reads(st, F, 1)
    lds, vm = st.ldsq, st.vmq
    full = block(F, "full", lds, vm)
    assert full.ldsq == lds and renamed(full.vmq, NEXT) == vm, (lds, full.ldsq, vm, full.vmq)      # the loop is closed
    n1 = block(F, "nodma", lds, vm)
    n2 = block(F, "nodma", n1.ldsq, renamed(n1.vmq, NEXT))
    lb = block(F, "last", n2.ldsq, renamed(n2.vmq, NEXT))
    assert lb.ldsq == [] and lb.vmq == [], (lb.ldsq, lb.vmq)
    loop = [F.label + ":"] + full.lines + ["s_sub_u32 %[cnt], %[cnt], 1", "s_cmp_lg_u32 %[cnt], 0", "s_cbranch_scc1 " + F.label]
    return st.lines + loop + n1.lines + n2.lines + lb.lines, full.lines


def main():
    with open(sys.argv[1] if len(sys.argv) > 1 else "flash4w.inc", "w") as f:
        for F, title in ((FA32, "Generated by gen_fa4w.py - do not edit."), (FA16, "The 16x16x32 form.")):
            lines, full = stream(F)
            n_mfma = sum(1 for x in full if x.startswith(F.mfma))
            n_valu = sum(1 for x in full if x.startswith("v_")) - n_mfma
            n_lds = sum(1 for x in full if x.startswith("ds_"))
            f.write("// %s  One FULL iteration: %d MFMA, %d VALU, %d ds_read_b128, %d lines.\n" % (title, n_mfma, n_valu, n_lds, len(full)))
            f.write(define(F.macro, lines, eol="\\n\\t") + "\n")


if __name__ == "__main__":
    main()
