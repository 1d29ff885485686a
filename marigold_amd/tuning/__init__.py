"""Measured launch choices for MG_OP_IGEMM ("find-db"): for a layer shape the library's heuristic (csrc/igemm2.hip::
mg_igemm_auto_variant + the automatic split-K rule) is not the fastest tile on, ``gfx950.json`` names the tile variant and
split-K count that measured fastest on an MI355X - written by ``tools/sweep_program.py --emit-db`` from timings of the REAL
launches of the denoising / VAE programs (real buffers and epilogues) at the ensemble sizes one GPU sees (E = 10 on one GPU;
5 / 3 / 2 / 1 members per GPU when a map's ten members are sharded over 2 / 4 / 8 GPUs), committed with its sweep logs under
``profiles/``.  A shape absent from the table runs the heuristic.  Every entry is covered as form x tile x split count:
tests/test_gpu_tuned_launches.py takes its parameter list from this table - every (key without M, tile, split-K count) runs once at
the entry's own N and K on a reduced M against float64 - and tests/test_tuned_launches_host.py pins the fields the key does not
carry to the ops of the full-size programs (results: docs/history/tuned_launch_parity.md).  The table is gfx950's: the library
itself refuses any other device (mg_init), so no second gate is needed here.  The choice is a pure function of the op - deterministic, the same on every rank.

Key = (M, N, K, taps, stride, epilogue, transposed section?, batch_z, residual?, row statistics out?, folded LayerNorm in?,
second source?, time-embedding row?): what the tile's time depends on; B / H / W enter through M only.
"""
import json
import os

from .. import _lib as L, ops as O

_DB = None
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gfx950.json")
ENABLED = not (os.environ.get("MARIGOLD_TUNING") == "1" and os.environ.get("MARIGOLD_TUNING_DB") == "0")   # A/B: heuristics only


def key_of(op):
    v = O.igemm_view(op)
    key = (f"{v.M},{v.n},{v.K},{v.taps},{v.stride},{v.epi},{int(v.has_trans)},{v.batch_z},"
           f"{int(v.has_residual)},{int(v.has_ln_out)},{int(v.has_ln_in)},{int(v.has_a1)},{int(v.has_rowvec)}")
    key += f",x{v.cx}" if v.has_fold else ""   # (a folded 1x1 convolution: its channel count)
    # (round 6) what else decides whether a tile is legal or fast - appended only where it differs from the plain form the table
    # was swept on, so that existing entries keep their keys and an odd launch can never collide with them: a virtual up-sampled
    # input, a padding other than the tap window's own, operand row strides wider than the channel count
    if v.hu or v.wu:
        key += f",u{v.hu}x{v.wu}"
    if v.pad != (1 if v.taps in (9, 4) else 0):
        key += f",p{v.pad}"
    if v.lda != v.c0 or v.lda1 != v.cin - v.c0 or v.ldw != v.Kx:
        key += f",ld{v.raw.lda}.{v.raw.lda1}.{v.raw.ldw}"
    return key


def load():
    global _DB
    if _DB is None:
        try:
            with open(_PATH) as f:
                _DB = json.load(f)["igemm"]
        except FileNotFoundError:
            _DB = {}
    return _DB


def apply(op):
    """Set the measured (tile variant, split-K count) on an MG_OP_IGEMM op that leaves both to the library (``variant`` == 0 and
    ``splits`` == 0).  Returns the op.  The hand-placed tiles (72 / 73) address their operands with 31-bit byte offsets
    (csrc/igemm2.hip::dispatch_tile); the library's own choice falls back to 62 / 46 beyond that - a table entry must not take
    that fallback away."""
    if not ENABLED or op.kind != L.OP_IGEMM:
        return op
    v = O.igemm_view(op)
    if v.variant != 0 or v.splits != 0:
        return op
    hit = load().get(key_of(op))
    if hit is not None and not (int(hit[0]) in (72, 73) and not v.fits_31bit):
        v.raw.variant, v.raw.splits = int(hit[0]), int(hit[1])
    return op
