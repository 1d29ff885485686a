"""Which kernel a layer runs on: the engine's switches and every routing rule, as free functions of plain integers.

``engine.Builder`` asks once per layer - ``conv_route`` for a lone convolution, ``resnet_route`` for a ResNet block,
``transformer_route`` for a transformer block, ``norm_route`` for a lone GroupNorm - and emits the ops the answer names; nothing
here needs a buffer, a weight, the library or a GPU:

    >>> from marigold_amd import routes
    >>> routes.resnet_route(10, 48, 48, (1280, 640), 640, True, 32)     # up_blocks.2.resnets.0 at ten members

The measurement comments are the record of why each threshold has its value.  This module imports ``math`` and ``os`` only.
"""
import math
import os
from collections import namedtuple


def _tune(name, default):
    """Tuning switch ``name`` (an environment variable): honoured ONLY under MARIGOLD_TUNING=1 (same-box A/B runs, sweeps);
    without it the engine builds the product configuration whatever else the environment holds.  The library's switches sit
    behind the same gate (csrc/runtime.hip::mg_tuning_int)."""
    if os.environ.get("MARIGOLD_TUNING") != "1":
        return default
    v = os.environ.get(name)
    if v is None:
        return default
    return v if isinstance(default, str) else type(default)(int(v))


USE_PATCH = _tune("MARIGOLD_PATCH_CONV", True)          # patch-resident conv3x3 kernel where eligible
FUSE_GN = _tune("MARIGOLD_FUSE_GN", "auto")             # auto | all | none: GroupNorm apply inside the conv
GN_BYPRODUCT = _tune("MARIGOLD_GN_BYPRODUCT", True)     # GroupNorm partial sums from the producing convolution's epilogue
VAE_FLASH_SMALL_MIN_BLOCKS = _tune("MARIGOLD_VAE_FLASH_MIN_BLOCKS", 100)   # flash512 for launches of at least this many 128-query blocks
IGEMM73_CONV = _tune("MARIGOLD_IGEMM73_CONV", True)     # plain N = 320 k convolutions on the hand-placed 192 x 320 GEMM tile
IGEMM73_CONV_MIN_TILES = _tune("MARIGOLD_IGEMM73_CONV_MIN_TILES", 120)
IGEMM72_VAE = _tune("MARIGOLD_IGEMM72_VAE", True)       # plain 512-channel convolutions on the hand-placed implicit-GEMM tile
GN_STATS_ONE_LAUNCH = _tune("MARIGOLD_GN_STATS_ONE_LAUNCH", True)   # the two sources of a skip concat in one statistics launch
HEAD_CONV = _tune("MARIGOLD_HEAD_CONV", True)   # conv_norm_out + SiLU + conv_out (<= 4 channels) as one MG_OP_CONV3X3_HEAD launch
HEAD_CONV_MIN_PIXELS = _tune("MARIGOLD_HEAD_CONV_MIN_PIXELS", 1 << 18)
FOLD_SHORTCUT = _tune("MARIGOLD_FOLD_SHORTCUT", True)   # conv_shortcut as extra K of conv2 where conv2 runs on the implicit GEMM
GN_SLAB = _tune("MARIGOLD_GN_SLAB", True)               # GroupNorm as one launch per norm (MG_OP_GN_SLAB) where it applies
GN_SLAB_MIN_WG = _tune("MARIGOLD_GN_SLAB_MIN_WG", 64)   # ... from this many (image, channel window) workgroups,
GN_SLAB_SMALL_KB = _tune("MARIGOLD_GN_SLAB_SMALL_KB", 48)   # or fewer when a workgroup's share of the tensor is at most this (small ensembles)
ROWGEMM = _tune("MARIGOLD_ROWGEMM", True)               # row-resident GEMM (MG_OP_ROWGEMM) for the K = 320 token-local layers
XATTN_KSPLIT = _tune("MARIGOLD_XATTN_KSPLIT", True)     # deep-level collapsed cross-attention as the K-split kernel
ROWGEMM_WIDE = _tune("MARIGOLD_ROWGEMM_WIDE", True)     # ... and its K = 640 form for the 640-channel level's QKV / GEGLU
XATTN_IN_GEGLU = _tune("MARIGOLD_XATTN_IN_GEGLU", True)   # the collapsed cross-attention as the prologue of the row-resident GEGLU launch
ROWGEMM_MIN_M = _tune("MARIGOLD_ROWGEMM_MIN_M", 9216)   # below: the tile GEMM (one 96 x 96 member is 72 128-row workgroups)
# Measurement probe (never the product path): every launch of these op kinds is issued TWICE (idempotent kinds only: GroupNorm
# 2,3,4,9 / flash attention 6,11 write outputs they do not read) - the map's extra time is what that class costs with the
# other lanes running beside it, i.e. the most a faster kernel of that class could return (tools: scripts/gpu_ab_env.sh)
TWICE_KINDS = tuple(int(k) for k in _tune("MARIGOLD_TWICE_KINDS", "").split(",") if k)

# ---- the values a route is made of --------------------------------------------------------------------------------------
CONV_PATCH, CONV_PATCH_SUBPIX = "patch", "patch sub-pixel"            # MG_OP_CONV3X3
CONV_IGEMM, CONV_IGEMM_SUBPIX = "igemm", "igemm sub-pixel"            # MG_OP_IGEMM
STATS_SLAB, STATS_CHUNKED = "slab", "chunked"      # a norm's scale / shift: MG_OP_GN_SLAB | the producer's by-product, else MG_OP_GN_STATS
APPLY_SLAB, APPLY_PASS, APPLY_CONSUMER = "slab", "pass", "consumer"   # the same slab launch | MG_OP_GN_APPLY | inside the consuming launch
SHORTCUT_FOLDED, SHORTCUT_LAUNCH, SHORTCUT_IDENTITY = "folded into conv2", "own launch", "identity"
ROWS_K320, ROWS_K640, ROWS_TILE = "rowgemm K=320", "rowgemm K=640", "tile GEMM"
XATTN_IN_GEGLU_LAUNCH, XATTN_KSPLIT_ROWS, XATTN_ROWS, XATTN_TILE, XATTN_TWO_LAUNCHES = "geglu prologue", "k-split", "rows", "tile", "two launches"

NormRoute = namedtuple("NormRoute", "stats apply")
ResnetRoute = namedtuple("ResnetRoute", "norm1 conv1 norm2 conv2 shortcut")
# ``rows``: the kernel family of the token-local Linear layers (K320: all of them; K640: QKV and GEGLU only); ``norm``: the block's
# GroupNorm; ``qkv`` / ``geglu`` / ``xattn_cfg`` / ``whole_rows`` / ``proj_out``: rowgemm_cfg of those launches (None: tile GEMM)
TransformerRoute = namedtuple("TransformerRoute", "rows norm qkv geglu xattn xattn_cfg whole_rows proj_out")


# ---- convolutions -------------------------------------------------------------------------------------------------------
def patch_eligible(H, W, B=None, N=None, subpix=False):
    """16-pixel-wide tiles: maps that waste little of them (the 24x24 / 12x12 levels stay on the implicit GEMM,
    whose split-K also fills the chip there) and - when the batch and width are given - enough workgroups for the
    256 CUs (a single member at 96x96 has 36-72 spatial tiles: the implicit GEMM's smaller tiles fill the chip)."""
    if not ((H >= 32 and W >= 32) or (H % 16 == 0 and W % 16 == 0)):
        return False
    if B is None:
        return True
    if N % 256 == 0:
        th, bn = 16, 256
    elif N == 320 or (subpix and N % 320 == 0):
        th, bn = 8, 320
    else:
        th, bn = 16, 128
    grid = B * -(-H // th) * -(-W // 16) * -(-N // bn) * (4 if subpix else 1)
    return grid >= 240


def big_gemm(M, Cin, cout):
    """A plain stride-1 3x3 convolution of M pixels on a hand-placed implicit-GEMM tile rather than a patch kernel?"""
    # (round 4) plain 512-channel VAE convolutions with >= 720 tiles of 256 x 256: the hand-placed implicit-GEMM tile
    # (variant 72, picked by the library) runs them at 1 284 TFLOP/s against 1 202 / 1 050 for the patch kernels
    if IGEMM72_VAE and cout % 256 == 0 and Cin >= 512 and -(-M // 256) * (cout // 256) >= 720:
        return True
    # ... and the plain N = 320 k convolutions with a chip's worth of 192 x 320 tiles (the 640-channel level at 48 x 48) on
    # variant 73: 640 -> 640 1 193 vs 1 147-1 182 for the four-wave patch kernel, 1280 -> 640 1 303 vs 1 267-1 277
    # (round 5: from 120 tiles - six members at 48 x 48; with eight the four-wave patch kernel ran these at 760-790 TFLOP/s
    # where the GEMM tile does 1 170-1 300: the >= 200 of round 4 had been set at E = 10 only)
    return bool(IGEMM73_CONV and cout % 320 == 0 and cout % 256 != 0 and Cin >= 320 and
                -(-M // 192) * (cout // 320) >= IGEMM73_CONV_MIN_TILES)


def conv_route(B, H, W, Cin, cout, stride=1, pad=1, up=None, extras=False):
    """Route of a 3x3 convolution of a [B][H][W][Cin] tensor.  ``up``: nearest up-sampling to that (H, W) first; ``extras``: the
    launch adds a row vector or a residual (the sub-pixel forms do neither)."""
    plain = stride == 1 and pad == 1
    subpix = up is not None and up == (2 * H, 2 * W) and plain and not extras
    if USE_PATCH and plain and not (up is None and big_gemm(B * H * W, Cin, cout)) and patch_eligible(H, W, B, cout, up is not None):
        if up is None:
            return CONV_PATCH
        if subpix:
            return CONV_PATCH_SUBPIX
    # exact 2x nearest up-sampling: four 2x2 convolutions on the low-resolution input (4/9 of the MACs)
    return CONV_IGEMM_SUBPIX if subpix else CONV_IGEMM


def fuse_norm_into_conv(B, H, W, Cin, N):
    """Apply the GroupNorm affine + SiLU inside the convolution's operand staging?  The fix-up runs once per
    workgroup and channel tile, i.e. (output-channel tiles) x 1.27 (halo) times per element, on VALU that the
    MFMAs do not hide: it pays when one workgroup covers all output channels (N <= 320) or when the separate
    pass would be HBM-bound on a tensor that no cache holds (profiles/r2_sweep3_patch_conv.log)."""
    mode = FUSE_GN
    if mode not in ("auto", "auto5"):
        return mode == "all"
    tiles_n = 1 if N in (128, 256, 320) else -(-N // (256 if N % 256 == 0 else 128))
    if mode == "auto5":   # the rule of rounds 2-5 (A/B)
        return tiles_n == 1 or B * H * W * Cin * 2 >= (192 << 20)
    # Round 6, measured layer by layer with the norm fused everywhere / nowhere (profiles/r6_ab_fuse_gn_per_layer.log): the
    # fix-up is VALU beside the MFMAs, the separate pass is HBM traffic - and with two maps in flight (section 6b) an HBM-bound
    # pass runs under the other map's matrix work.  Fused wins on the VAE's 128 / 256-channel levels (tensors of 0.75-1.5 GB:
    # +0.45 ... +0.97 ms per block unfused, and with two lanes the 256-channel level alone +1.4 ms per map); it LOSES where the plain convolution gets a hand-placed four-wave kernel that the
    # fused one does not - the UNet's 320-channel level from six members (-0.1 ... -0.66 ms per block) - and on the VAE's
    # 512-channel 192 x 192 level (two output-channel tiles repeat the fix-up: -0.17 ... -0.24 ms per block).
    if N == 320:
        return B * -(-H // 12) * -(-W // 16) < 280   # (six members: -1.1 ms with two lanes, -3 ms alone; five: a tie)
    return tiles_n == 1


def head_conv_ok(B, H, W, C, cout):
    """norm + SiLU + conv3x3 to <= 4 channels as one MG_OP_CONV3X3_HEAD launch?  The VAE decoder's head (768^2 maps: 0.80 ms
    against 0.58 + 1.22 ms for the normalising pass + the implicit GEMM at ten members); NOT the UNet's - its 96^2 maps are
    360 workgroups of ten LDS-bound passes (79-102 us at ten members, 64-101 at one) where the pass + GEMM pair takes 54 / 33 us
    (profiles/r5_ops_hipevents*.tsv of the two final sessions)."""
    return bool(HEAD_CONV and cout <= 4 and C % 32 == 0 and B * H * W >= HEAD_CONV_MIN_PIXELS)


def gn_byproduct_ok(HW, cout, groups):
    """Ask the patch convolution for its output's GroupNorm partial sums (``ops.conv3x3_gn_slots`` then says whether its tile
    gives them)?  (round 4) A by-product of the 12-wave tiles' epilogue - the tensors of the VAE's 768^2 / 384^2 levels are
    re-read at HBM speed otherwise (4.6 ms of statistics passes per decode at E = 10)."""
    return bool(GN_BYPRODUCT and cout % groups == 0 and cout // groups in (4, 8, 16, 32) and HW * cout * 2 >= (8 << 20))


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------
def gn_slab_ok(B, HW, chans, groups, apply):
    """One-launch GroupNorm (MG_OP_GN_SLAB: a workgroup owns whole groups of an image over all rows) of the channel concat of
    sources with ``chans`` channels?  UNet-sized maps with enough (image, channel window) pairs to fill the chip; the normalising
    form keeps the rows in registers (<= 48 rows per thread).  Large tensors (UNet level 0, the VAE) stay on the chunked
    statistics / apply passes."""
    C = sum(chans)
    if not GN_SLAB or len(chans) > 2 or C % groups or any(c % 4 for c in chans):
        return False
    cpg = C // groups
    cw = cpg * (4 // math.gcd(cpg, 4))
    nwg = B * (C // cw)
    # (round 5) few workgroups are fine while each one's share is small: a single member's 24 x 24 / 12 x 12 maps (368 KB -
    # 1.5 MB) took a statistics launch (13-16 us: tickets, last-block finalize) + an apply launch (8-9 us) for lack of 64 of them
    if not (16 <= cw <= 128) or HW > 16384 or (nwg < GN_SLAB_MIN_WG and B * HW * C * 2 > nwg * GN_SLAB_SMALL_KB * 1024):
        return False
    # measured per layer (profiles/r3_groupnorm_slab_vs_chunked.log): a slab pass beats statistics + apply only while
    # the tensor is small enough that the chunked passes are launch/latency-bound (<= 16 MiB: UNet levels 2-3), or
    # when it replaces the TWO statistics launches of a skip concat at levels 1-3; on the big level-0 / VAE tensors
    # its B * C / cw workgroups are too few and the chunked passes win by 1.3-1.8x
    if not ((len(chans) == 2 and HW <= 2304) or B * HW * C * 2 <= (16 << 20)):
        return False
    if apply:
        nt = 1024 if HW * cw * 2 >= 48 * 1024 else 256
        if -(-HW // (nt // (cw // 4))) > 48:
            return False
    return True


def norm_route(B, HW, chans, groups, consumer=False):
    """-> NormRoute of a GroupNorm over the concat of sources with ``chans`` channels.  ``consumer``: the launch that reads the
    tensor applies scale / shift itself (a fused convolution, the head convolution, the row-resident proj_in), so only the
    statistics are wanted."""
    if not consumer and gn_slab_ok(B, HW, chans, groups, True):   # statistics + normalisation (+ the concat) in one launch
        return NormRoute(STATS_SLAB, APPLY_SLAB)
    return NormRoute(STATS_SLAB if gn_slab_ok(B, HW, chans, groups, False) else STATS_CHUNKED, APPLY_CONSUMER if consumer else APPLY_PASS)


def gn_stats_chunks(B, HW):
    """Chunks per image of an MG_OP_GN_STATS launch."""
    # ~288 (chunk, image) blocks - about one per CU - of >= 32 rows: with eight row loads in flight per thread and the
    # chunk's tail fetched as one batch (round 3) a block streams its rows in 2-4 round trips, and the cost that is left
    # grows with the NUMBER of blocks (tickets, the last block's table reduction): 59 MB at E = 10 takes 16.3 us with 24-32
    # chunks per image against 23.5 with the 76 of round 2 (28.7 before the tail fix), profiles/r3_gn_stats_chunks.log
    return max(1, min(HW // 32, 64, max(8, 288 // B)))


# ---- ResNet blocks ------------------------------------------------------------------------------------------------------
def resnet_route(B, H, W, chans, cout, has_shortcut, groups):
    """-> ResnetRoute of a ResnetBlock2D on the concat of sources with ``chans`` channels (``has_shortcut``: the checkpoint has
    a conv_shortcut for it).  norm -> SiLU is applied inside the convolution's operand staging where ``fuse_norm_into_conv``
    says it pays - and a fused norm takes the patch kernel WHATEVER ``big_gemm`` says: only the patch kernel fuses, and fused
    beat the 192 x 320 GEMM tile where both apply (the 320-channel level below six members)."""
    patch = USE_PATCH and patch_eligible(H, W, B, cout)

    def norm_and_conv(cs):
        cin = sum(cs)
        if patch and fuse_norm_into_conv(B, H, W, cin, cout):
            return norm_route(B, H * W, cs, groups, consumer=True), CONV_PATCH
        return norm_route(B, H * W, cs, groups), conv_route(B, H, W, cin, cout)

    norm1, conv1 = norm_and_conv(tuple(chans))
    norm2, conv2 = norm_and_conv((cout,))
    # (round 5) where conv2 runs on the implicit GEMM (the 48 x 48 ... 12 x 12 levels) its conv_shortcut - a 1x1 convolution of the
    # block's INPUT - rides as extra K of conv2: one launch instead of two, no residual tensor written and read back
    if not has_shortcut:
        shortcut = SHORTCUT_IDENTITY
    elif FOLD_SHORTCUT and all(c % 64 == 0 for c in chans) and cout % 64 == 0 and conv2 == CONV_IGEMM:   # (so norm2 is not fused)
        shortcut = SHORTCUT_FOLDED
    else:
        shortcut = SHORTCUT_LAUNCH
    return ResnetRoute(norm1, conv1, norm2, conv2, shortcut)


# ---- transformer blocks -------------------------------------------------------------------------------------------------
def rowgemm_ok(C, HW, M):
    """Token-local Linear layers of a [M = B HW][C] activation on MG_OP_ROWGEMM?  K = 320 is what the kernel is built for (a wave
    keeps 32 rows x 320 channels in 80 registers); whole 32-row tiles inside an image (the V^T section and the folded
    GroupNorm are per image), enough 384-row workgroups for the chip, and the permuted V^T the QKV form writes."""
    return bool(ROWGEMM and C == 320 and HW % 32 == 0 and M >= ROWGEMM_MIN_M)


def rowgemm_wide_ok(C, HW, M):
    """The 640-channel level: MG_OP_ROWGEMM's K = 640 form (8 waves x 32 rows x 640 channels in 160 registers each) pays
    only where the columns can be split over two workgroups per 256-row block - the QKV projection (97 -> 80 us) and GEGLU
    (216 -> 194 us); the whole-row-statistics layers stay on the tile GEMM (90 workgroups: 64 vs 49 us),
    profiles/r3_rowgemm_k640.log."""
    return bool(ROWGEMM and ROWGEMM_WIDE and C == 640 and HW % 32 == 0 and M >= 60 * 256)


def rowgemm_cfg(M, N, whole_rows=False, xattn=False, K=320):
    """-> dict(waves=, nsplit=) of an MG_OP_ROWGEMM launch.  K = 640: 8 waves, the N / 128 column stages split so that workgroups
    <= CUs.  K = 320: 12 waves (384 rows) per workgroup when that still gives the chip >= 160 workgroups, else 8, else 4 with the
    N / 64 column stages shared out over several workgroups per row block (not for the forms that take whole-row statistics) -
    measured per ensemble size, profiles/r3_rowgemm_small_batch.log."""
    if K == 640:
        return dict(waves=8, nsplit=max(1, min(N // 128, 256 // -(-M // 256))))
    if M >= 160 * 384:
        return dict(waves=12)
    if M >= 120 * 256 or xattn:
        return dict(waves=8)
    if whole_rows:
        return dict(waves=4)
    nwg = -(-M // 128)
    return dict(waves=4, nsplit=max(1, min(N // 128, round(300 / nwg))))


def transformer_route(B, HW, C, heads, groups):
    """-> TransformerRoute of a Transformer2DModel block on a [B][HW][C] activation with ``heads`` heads of 64 channels."""
    M = B * HW
    rows = ROWS_K320 if rowgemm_ok(C, HW, M) else ROWS_K640 if rowgemm_wide_ok(C, HW, M) else ROWS_TILE
    k320 = rows == ROWS_K320
    # K = 320: the GroupNorm never runs as a pass - statistics only, its scale / shift applied while proj_in loads its rows
    norm = norm_route(B, HW, (C,), groups, consumer=k320)
    geglu = rowgemm_cfg(M, 8 * C, K=C) if rows != ROWS_TILE else None
    xattn_cfg = None
    # (round 6) at the 320-channel level the collapsed cross-attention is the PROLOGUE of the GEGLU launch: that launch holds the
    # rows in registers anyway - it updates them (and stores them once, for ff.out's residual), takes the next LayerNorm's
    # statistics from its own sums and goes on; no cross-attention launch, one read of the residual stream less
    if k320 and XATTN_IN_GEGLU and 2 * heads <= 64 and geglu.get("nsplit", 1) <= 1:
        xattn = XATTN_IN_GEGLU_LAUNCH
    elif XATTN_KSPLIT and ROWGEMM and 2 * heads <= 64 and C in (640, 1280) and M % 32 == 0:
        # the deep levels: 32-row workgroups whose four waves split K (scores) and the output channels (blend)
        xattn, xattn_cfg = XATTN_KSPLIT_ROWS, {}
    elif 2 * heads <= 64 and k320:
        # the same single launch in the row-resident form: the residual stream is read once (registers) and written once
        xattn, xattn_cfg = XATTN_ROWS, rowgemm_cfg(M, C, xattn=True)
    else:
        # ONE launch on the tile GEMM while the 2 * heads score columns fit one 64-column tile; more than 32 heads (no published
        # checkpoint): two launches - scores + pair softmax, then the blend
        xattn = XATTN_TILE if 2 * heads <= 64 and C % 32 == 0 else XATTN_TWO_LAUNCHES
    return TransformerRoute(rows, norm, rowgemm_cfg(M, 3 * C, K=C) if rows != ROWS_TILE else None, geglu, xattn, xattn_cfg,
                            rowgemm_cfg(M, C, whole_rows=True) if k320 else None, rowgemm_cfg(M, C) if k320 else None)


# ---- the VAE's attention ------------------------------------------------------------------------------------------------
def vae_attention_flash(B, T, C):
    """The flash form (MG_OP_FLASH_ATTN512) rather than scores GEMM -> row softmax -> P V?  round 4: flash form - the T x T
    scores (340 MB of fp32 per image at 96 x 96 latent pixels) never leave the registers.  One workgroup per 128 queries and CU:
    a launch that does not fill the chip (a single image: 72 workgroups - the encoder always, the decoder of a one-member shard)
    takes 0.93 ms against 0.50 ms for the three-stage form (profiles/r4_flash512.log; two-wave workgroups of 64 queries:
    1.12 ms), so launches of fewer than 100 query blocks take the three-stage form (round 5: -0.5 ms per map at every ensemble
    size); any width but the published 512 channels (the tiny test architecture) takes it too."""
    return C == 512 and B * ((T + 127) // 128) >= VAE_FLASH_SMALL_MIN_BLOCKS
