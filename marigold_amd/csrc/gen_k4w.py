#!/usr/bin/env python3
"""Writes igemm2_k4w.inc: the hand-placed K-tile instruction streams of the 256 x 256 / four-wave implicit GEMM
(igemm2_body.h, LOOP == 3; one wave per SIMD, 128 x 128 wave tile, accumulators in AGPRs).

One K tile (64 deep) of a wave = 64 v_mfma_f32_32x32x16_bf16 (4 k-steps x 4 x 4 fragments) with every other instruction of the
tile placed BY HAND in the gaps between them - hipcc's scheduler groups the fragment reads in front of the MFMAs, which on a
one-wave-per-SIMD kernel leaves the matrix pipe idle for every LDS round trip (profiles/r3_sweep_big_wave_tile.log: 1.0 PF/s).
The stream, per K tile t (LDS buffer b = t & 1; fragment set F[ks] = 4 pixel-side + 4 weight-side fragments of k-step ks):

  gap  0.. 7   ds_read F[2], F[3] of tile t            (two per gap; F[0], F[1] were read during tile t-1)
  gap  R1      s_waitcnt lgkmcnt(0) ; s_barrier         every wave has read ALL of buffer b -> it is free
  gap  D0..    16 x { s_add m0 ; buffer_load_dwordx4 .. lds }   tile t+2 -> buffer b, one piece every other gap
  gap  R2      s_waitcnt vmcnt(16) ; s_barrier          tile t+1 (issued during tile t-1) has landed for everyone
  gap  N0..    ds_read F[0], F[1] of tile t+1           (one per gap)

so a piece has 66-96 MFMA gaps (2.1-3.1 k cycles) to land, the fragments of a k-step are in registers 16+ gaps before their
first MFMA, and a gap carries at most two non-MFMA issues (MI355X_MICROARCH.md: <= 5 hide behind a 32 x 32 x 16 MFMA).
Waits are counted by the queue model of asmstream.py from the declared entry state (vmcnt retires in order; the LDS-DMA is only
ordered against ds_read by vmcnt + barrier).

Operand names (bound in igemm2_body.h): c<ni><mi> accumulators, a<ks><mi> / b<ks><ni> fragments (pixel / weight side),
la<ks> / lb<ks> LDS byte addresses of the fragment reads, xa<ks> / xb<ks> their buffer toggles (XOR), va<i> / vb<i> per-lane byte
offsets of the DMA pieces, sa / sb buffer resources, ma / mb = LDS addresses of this wave's first pixel / weight piece in the
buffers being filled.
"""
import sys

from asmstream import ALL, MFMA_RESULT_TAIL, Slots, Stream, define, renamed


class Geo:
    """MI x NI 32 x 32 fragments per wave (2 x 2 waves): 4 x 4 = the 256 x 256 tile (prefix K4W), 3 x 5 = the 192 x 320 tile
    (prefix K4WB: full-width tiles for the N = 320 k layers).  LDS: pixel-row buffers, then weight-row buffers; a read address
    toggles between an operand's two buffers by XOR with a per-register constant (xa<ks> / xb<ks>), the DMA bases (ma / mb) are
    toggled by the caller."""

    def __init__(self, prefix, mi, ni):
        self.prefix, self.MI, self.NI = prefix, mi, ni
        self.GS = mi * ni            # MFMAs per k-step
        self.NM = 4 * self.GS        # MFMAs per K tile
        self.NF = mi + ni            # reads per fragment set
        self.ND = 2 * (mi + ni)      # LDS-DMA pieces per tile and wave

    def mfma(self, g):
        ks, ni, mi = g // self.GS, (g % self.GS) // self.MI, g % self.MI
        return f"v_mfma_f32_32x32x16_bf16 %[c{ni}{mi}], %[b{ks}{ni}], %[a{ks}{mi}], %[c{ni}{mi}]"

    def reads(self, ks):
        """the fragment reads of k-step ks, pixel side first"""
        return ([f"ds_read_b128 %[a{ks}{i}], %[la{ks}] offset:{i * 4096}" for i in range(self.MI)] +
                [f"ds_read_b128 %[b{ks}{i}], %[lb{ks}] offset:{i * 4096}" for i in range(self.NI)])

    def toggles(self, ks):
        return [f"v_xor_b32 %[la{ks}], %[xa{ks}], %[la{ks}]", f"v_xor_b32 %[lb{ks}], %[xb{ks}], %[lb{ks}]"]

    def dma(self, i):
        """piece i of the next-but-one tile: (M0 write, in front of an MFMA; LDS-DMA, behind it)"""
        if i < 2 * self.MI:
            return (f"s_add_u32 m0, %[ma], {i * 4096}", f"buffer_load_dwordx4 %[va{i}], %[sa], 0 offen lds")
        j = i - 2 * self.MI
        return (f"s_add_u32 m0, %[mb], {j * 4096}", f"buffer_load_dwordx4 %[vb{j}], %[sb], 0 offen lds")

    def entry_lds(self):
        return ["F0"] * self.NF + ["F1"] * self.NF

    def entry_vm(self, mode):
        return [] if mode == "last" else ["T1"] * self.ND


# Queue tags.  LDS: F<ks> = fragment set ks of this tile, F<ks>n = of the next tile.  VMEM: T1 / T2 = the pieces of tile t + 1 /
# t + 2.  A tile is entered with F[0] then F[1] of this tile in the LDS queue and the pieces of tile t + 1 in the VMEM queue
# (none in front of the last tile).  In C that state is set up by igemm2_body.h: two stage_tile() calls, then
# `wait_vmcnt<A_IT + B_IT>` (one tile's pieces stay in flight) and the barrier in front of K4W_ASM_PROLOGUE, which reads F[0]
# and F[1] of tile 0.  What a tile issues for "the next tile" is the next stream's "this tile":
NEXT = {"F0n": "F0", "F1n": "F1", "T2": "T1"}


def tile(G, mode, rd_per_gap, r1, r2, n0, dma=(), fill=None, drain_lds_at_r2=False):
    """One K tile (also the skeleton of gen_cp4w.py).  mode: 'full' (tiles t + 1 and t + 2 exist), 'nodma' (t + 1 exists),
    'last'.  dma: (gap, M0 write, LDS-DMA, tag) per piece; fill(slots, first gap behind the fragment reads) places what a
    kernel adds between the two barriers.  -> the resolved stream; .late: tags of the F[2] / F[3] reads placed at or behind r1"""
    sl = Slots(G.NM)
    sl.pre(0, None, "wait_lds", "F0")
    # --- F[2], F[3] of this tile
    cur = [(t, "lds", f"F{ks}") for ks in (2, 3) for t in G.reads(ks)]
    late = []
    g = 0
    while cur:
        for it in cur[:rd_per_gap]:
            sl.post(g, *it)
            if g >= r1:
                late.append(it[2])
        del cur[:rd_per_gap]
        g += 1
    for ks in (2, 3):
        for t in G.toggles(ks):
            sl.post(g + ks - 2, t)
    sl.pre(r1, None, "wait_lds", ALL)          # every wave has read all of this tile's buffer ...
    if mode != "last":
        sl.pre(r1, "s_barrier")                # ... it is free
        for gg, m0_write, load, tag in dma:    # (an SALU write of M0 needs one instruction before the LDS-DMA that reads it)
            sl.pre(gg, m0_write)
            sl.post(gg, load, "vm", tag)
        if fill:
            fill(sl, g)
        sl.pre(r2, None, "wait_vm", "T1")      # tile t + 1 has landed ...
        if drain_lds_at_r2:
            sl.pre(r2, None, "wait_lds", ALL)
        sl.pre(r2, "s_barrier")                # ... for everyone: its first two fragment sets
        nxt = [(t, "lds", f"F{ks}n") for ks in (0, 1) for t in G.reads(ks)]
        assert n0 + len(nxt) <= G.NM, n0
        for k, it in enumerate(nxt):
            sl.post(n0 + k, *it)
        for t in G.toggles(0) + G.toggles(1):
            sl.tail(t)
    st = sl.play(Stream(G.entry_lds(), G.entry_vm(mode)), G.mfma)
    if mode == "last":
        st.lines += MFMA_RESULT_TAIL
    st.late = late
    return st


def prologue(G):
    """fragment sets F[0], F[1] of tile 0 (buffer 0), then la0 / la1 -> buffer 1"""
    st = Stream()
    for ks in (0, 1):
        for t in G.reads(ks):
            st.lds(t, f"F{ks}")
    for t in G.toggles(0) + G.toggles(1):
        st.op(t)
    return st


def assert_closed(G, pro, fulls, nodma, last):
    """The chain PROLOGUE, FULL x n, [NODMA], LAST is closed: every stream leaves in flight what the next one is entered with,
    the last one nothing.  fulls: (stream, older LDS items, older VMEM items); `older`: what a stream issues in front of the
    next tile's items and does not wait for (both counters retire in order: the next stream's first wait covers it).
    st.late: reads of F[2] / F[3] that a schedule places behind r1 stay in flight to the end of their tile - rd_per_gap=1 does,
    no wait covers them in front of their MFMAs; the default schedules have none - named so that everything else is compared
    exactly."""
    assert pro.ldsq == G.entry_lds(), pro.ldsq
    for st, older_lds, older_vm in fulls + [(nodma, [], [])]:
        assert renamed(st.ldsq, NEXT) == st.late + older_lds + G.entry_lds(), (st.ldsq, st.late)
        assert renamed(st.vmq, NEXT) == older_vm + (G.entry_vm("full") if st is not nodma else []), st.vmq
    assert last.ldsq == last.late and last.vmq == [], (last.ldsq, last.vmq)


def main():
    # schedule parameters: reads per gap in the first segment, gap of the buffer-release barrier, first DMA gap and DMA stride,
    # gap of the landed barrier, first gap of the next tile's fragment reads
    p = dict(rd_per_gap=2, r1=12, d0=13, dstep=2, r2=46, n0=47)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        p[k] = int(v)
    assert p["d0"] > p["r1"] and p["n0"] >= p["r2"] and p["n0"] + 16 <= 64 + 0
    txt = ["// GENERATED by gen_k4w.py " + " ".join(f"{k}={v}" for k, v in p.items()) + " - do not edit; see the generator for the schedule."]
    for G in (Geo("K4W", 4, 4), Geo("K4WB", 3, 5)):
        r2, n0 = (p["r2"], p["n0"]) if G.NM == 64 else (G.NM - 2 * G.NF - 2, G.NM - 2 * G.NF - 1)
        dma = [(p["d0"] + i * p["dstep"],) + G.dma(i) + ("T2",) for i in range(G.ND)]
        full, nodma, last = (tile(G, mode, p["rd_per_gap"], p["r1"], r2, n0, dma if mode == "full" else ())
                             for mode in ("full", "nodma", "last"))
        pro = prologue(G)
        assert_closed(G, pro, [(full, [], [])], nodma, last)
        for name, st in (("FULL", full), ("NODMA", nodma), ("LAST", last), ("PROLOGUE", pro)):
            txt += [define(f"{G.prefix}_ASM_{name}", st.lines), ""]
    print("\n".join(txt))


if __name__ == "__main__":
    main()
