/*
 * marigold_hip.h - C ABI of libmarigold_hip.so, the MI355X (gfx950) engine behind the
 * Marigold inference hot path.
 *
 * The reference has no FFI: its hot path sits behind Python module attributes registered on
 * the pipeline (marigold/marigold_depth_pipeline.py:133-139) whose arithmetic lives in
 * diffusers/torch.  Each entry point below replaces one of those call sites (cited per op).
 * Plain pointers and sizes only: device pointers are raw HIP device addresses, `stream` is a
 * hipStream_t passed as void*.  All functions return 0 on success, non-zero on error
 * (message via mg_last_error()).  Activations are bf16 NHWC ([B][H][W][C] == [B*H*W][C]
 * token-major); latents and decoded maps at the pipeline boundary are fp32 NCHW like the
 * reference's tensors.
 *
 * Every kernel launch is described by one fixed-size `mg_op`; a sequence of them is a
 * *program* (mg_program_*) that the library replays with no host logic in between (and
 * optionally as a captured hipGraph).  The Python host mirrors the reference's
 * unet/vae/scheduler interface by building such programs (marigold_amd/engine.py, modules.py).
 *
 * The stream contract - a call enqueues all of its device work on the stream it is given, owns its workspace until that stream has
 * passed it, and does not synchronise except where its comment says so - is tested for every stand-alone call that takes a stream
 * (tests/test_gpu_stream_fidelity.py; tests/test_stream_fidelity_host.py holds that file's table to the prototypes below).
 */
#ifndef MARIGOLD_HIP_H
#define MARIGOLD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_ABI_VERSION 4

enum mg_op_kind {
  /* conv3x3 / conv1x1 / Linear / batched GEMM as ONE implicit-GEMM bf16 MFMA kernel.
   * Replaces torch conv2d / linear / matmul inside diffusers UNet2DConditionModel and
   * AutoencoderKL (reference call sites marigold_depth_pipeline.py:461-463, 491-492, 512-513).
   * The slots are named by the MG_IGEMM_* enumerators below, each with its meaning; what spans several of them:
   *  Second source (P_A1, I_C0, I_LDA1): channels [C0, Cin) of every tap come from A1, [0, C0) from A - the UNet's skip concat,
   *  never materialised.
   *  Statistics hand-off (P_LN_OUT, F_LN_EPS, I_TICKETS_LO / _HI): ln_out f32 [M][N/32 + 1][2] holds the LayerNorm statistics
   *  of the tensor this launch produces (bf16 epilogue, N % 32 == 0): every tile writes (sum, sum of squares) of its rows over each
   *  32-column slot into [M][N/32][2], and the last column tile of a row block to finish reduces them to (mean, rstd) rows [M][2]
   *  stored BEHIND the slots (at ln_out + M * (N/32) * 8 bytes) - that address is the ln_in of the consuming layers.  ln_out is
   *  taken from the fp32 values before they are rounded (and, in the fp16 build, saturated) to the 16-bit row that is stored.  Launches
   *  that write statistics share one ticket array: they must be stream-ordered with respect to each other.
   *  Folded LayerNorm (P_LN_IN, P_LN_G, P_LN_C; diffusers BasicTransformerBlock: norm1 -> attn1.to_q/k/v, norm2 -> attn2.to_q,
   *  norm3 -> ff.net.0.proj): A holds the raw rows x, Wt = W * gamma, and out = rstd[m] * (acc - mean[m] * ln_g[n]) + ln_c[n] with
   *  ln_g[n] = sum_k Wt[n][k], ln_c[n] = sum_k beta[k] W[n][k] + bias[n]; (mean, rstd) come from the producer's ln_out.  No
   *  separate normalisation pass, no normalised tensor in HBM.
   *  Folded shortcut (P_X0, P_X1, I_CX, I_CX0, I_LDX0, I_LDX1): a 1x1 convolution of a SECOND tensor folded in as extra K
   *  (diffusers ResnetBlock2D: conv2(h) + conv_shortcut(x) in ONE launch - no shortcut launch, no residual round trip):
   *  K = taps * Cin + Cx, weight row n = [conv weights (taps * Cin) | shortcut weights (Cx)], the extra K tiles read pixel (y, x)
   *  of X0 (channels [0, Cx0)) and X1 ([Cx0, Cx): the UNet's skip concat); taps = 9, stride 1, pad 1 only; Cx, Cx0 multiples of
   *  64; the bias is the two layers' sum. */
  MG_OP_IGEMM = 1,
  /* GroupNorm, 3 launches (stats partials -> per-(b,c) scale/shift -> apply [+SiLU]).
   * Replaces torch group_norm + silu in every ResNet block / Transformer2D input norm.
   * The slots are named by the MG_GN_STATS_* / MG_GN_FINALIZE_* / MG_GN_APPLY_* enumerators below.
   *  STATS:    P_X holds channels [I_COFF, I_COFF + I_C) of an I_CTOT-channel norm (the UNet's skip concat torch.cat([hidden, skip])
   *            is normalised source by source, never materialised); block (chunk, b) writes slot I_SLOT0 + chunk of P_PARTIALS.
   *            With P_SS != NULL the image's last-arriving block also does FINALIZE's job (no finalize launch): P_GAMMA, P_BETA,
   *            P_COUNTERS and F_EPS are then required.  P_X1 with I_C1: a second source (channels [coff + C, + C1)) in the same
   *            launch - blocks [chunks, 2 chunks) write slots slot0 + chunks + ...
   *  APPLY:    with P_X1 the output channels [0, I_C0) come from P_X ([B][HW][C0]) and [C0, C) from P_X1 ([B][HW][C - C0]) */
  MG_OP_GN_STATS = 2,
  MG_OP_GN_FINALIZE = 3,
  MG_OP_GN_APPLY = 4,
  /* GroupNorm as ONE launch (statistics + scale/shift [+ normalised output]): a workgroup owns whole groups of one image
   * (channel window lcm(C / groups, 4) <= 128) over all H x W rows - no partial table, no tickets, one read of the tensor.
   * The slots are named by the MG_GN_SLAB_* enumerators below.  The normalised form keeps the rows in registers: H x W x window
   *  <= 48 rows per thread of a 1024-thread workgroup (the UNet's 96^2 ... 12^2 levels at any width). */
  MG_OP_GN_SLAB = 9,
  /* Row-resident GEMM for the token-local Linear layers at K = 320 / 640 (the two widest transformer levels): out[M][N] =
   * epilogue(x[M][K] W[N][K]^T).  A wave keeps 32 whole rows of x in registers for the launch and the weights stream past
   * it in 64-column stages, pre-packed in MFMA fragment order with a per-stage trailer of per-channel constants
   * (marigold_amd/weights.py::pack_rowgemm; csrc/rowgemm.hip).  M % 32 == 0, N % 64 == 0, N >= 128; K = 640 runs 8 waves
   * per workgroup (I_WAVES = 0 | 8), K = 320 4 / 8 / 12.
   * The slots are named by the MG_ROWGEMM_* enumerators below.  The forms (I_FORM):
   *  0 bias [+ residual] [+ row statistics]; 1 GEGLU: stage = 32 value + 32 gate channels, out [M][N/2]; 2 QKV: columns >=
   *  I_TRANS_FROM go to V^T (P_VT) in MG_OP_FLASH_ATTN64's permuted key order.
   *  form 3: the collapsed 2-token cross-attention (as MG_EPI_XATTN2) in place on the residual stream: N = 64 score
   *  columns, I_SM_COLS = 2 x heads of them live, F_SM_SCALE the softmax scale; P_WP = weights.pack_rowgemm_xattn (scores stage +
   *  VO^T fragments + bias), P_LN_IN required, out[M][K] = P VO^T + bias + x, P_LN_OUT its row statistics; out may alias x.
   *  K = 640 / 1280 (the deeper levels): the K-split kernel - 32-row workgroups whose four waves split K and the output channels,
   *  P_WP = weights.pack_rowgemm_xattn_ksplit.
   *  form 1 with P_XATTN (round 6; K = 320, no column split): the collapsed cross-attention as the PROLOGUE of the GEGLU launch
   *  (BasicTransformerBlock: x += attn2(norm2(x)); ff(norm3(x))) - P_XATTN = a weights.pack_rowgemm_xattn image, P_LN_IN = (mean,
   *  rstd) of the rows AS LOADED (norm2's), I_SM_COLS = 2 x heads, F_SM_SCALE the softmax scale; the rows are updated in registers,
   *  written once to P_XOUT bf16 [M][ldx] (may alias x: ff.out's residual) and the GEGLU projection's folded LayerNorm (norm3,
   *  F_LN_EPS) takes its statistics from the wave's own sums.  Bit-identical to the form-3 launch followed by the plain form-1
   *  launch. */
  MG_OP_ROWGEMM = 10,
  /* Self-attention core, head dim 64, bf16 MFMA flash attention with LDS-staged K / V^T
   * tiles (replaces diffusers Attention / SDPA / xformers, run.py:217-220).
   * The slots are named by the MG_FLASH64_* enumerators below.
   *  With I_VT_PERM = 1 and Ntok % 256 == 0 (>= 256) the current kernel is the hand-placed one (flash4w.hip; variant 26 forces
   *  its 32x32x16-MFMA stream, 27 the 16x16x32 one with the row sums on the matrix pipe - chosen by itself at >= 4 096 tokens
   *  from two blocks of 256 queries per CU): softmax against a fixed per-query reference, exact, with an in-kernel running-maximum
   *  fallback for rows whose sums reach F_REDO_THR.  With the optional workspace P_WS (I_WS_KB, I_SPLIT) the blocks of 256 queries
   *  left over beyond a multiple of the CU count are split along the keys over the chip (bit-reproducible). */
  MG_OP_FLASH_ATTN64 = 6,
  /* Self-attention core of ONE head of width 512 (the mid-block attention of AutoencoderKL: diffusers Attention in
   * UNetMidBlock2D, marigold_depth_pipeline.py:491-492, 512-513), flash form: the scores stay in registers.
   * The slots are named by the MG_FLASH_ATTN512_* enumerators below. */
  MG_OP_FLASH_ATTN512 = 11,
  /* Row softmax fp32 -> bf16 (single-head attention of a width other than 512, materialised scores; the collapsed 2-token
   * cross-attention of marigold_depth_pipeline.py:381-394, 438-442 needs no softmax op: scores = LN(x) Wqk^T with
   * Wqk[(h,j)] = Wq_h^T k_{j,h}, p = softmax over the key pair, out = p VO + bias + x with VO[(h,j)] = Wo[:,h] v_{j,h} run as
   * MG_EPI_XATTN2 / MG_OP_ROWGEMM form 3).  The slots are named by the MG_SOFTMAX_ROWS_* enumerators below. */
  MG_OP_SOFTMAX_ROWS = 7,
  /* Scheduler update (DDIM / LCM, diffusers *.step at marigold_depth_pipeline.py:466-468):
   * out = F_CX * x + F_CM * model_out + F_CN * noise.  The slots are named by the MG_SCHED_STEP_* enumerators below. */
  MG_OP_SCHED_STEP = 12,
  /* Small-M dense layer in fp32 (time-embedding MLP and per-ResNet projections):
   * out[m][n] = act_out(sum_k act_in(x[m][k]) * W[n][k] + bias[n]).  The slots are named by the MG_LINEAR_SMALL_M_* enumerators below. */
  MG_OP_LINEAR_SMALL_M = 13,
  /* 1x1 conv on fp32 NCHW latents with input scale (post_quant_conv after /0.18215,
   * marigold_depth_pipeline.py:510-512).  The slots are named by the MG_LATENT_1X1_* enumerators below. */
  MG_OP_LATENT_1X1 = 14,
  /* Pointwise tail of a small-Cout convolution computed by MG_OP_IGEMM into a padded fp32 buffer:
   * out NCHW = post(in[m][0..Cout) * F_SCALE): MG_POST_DEPTH = mean over channels, clip, (x+1)/2 (marigold_depth_
   * pipeline.py:515,473-475); MG_POST_NORMALS = clip, L2 normalise (marigold_normals_pipeline.py:438-440); MG_POST_UNIT.
   * The clip to [-1, 1] and the normalise's 1e-6 floor of the norm keep NaN, like torch.clip / clamp(min=eps) (+-inf clip to
   * +-1): a NaN channel gives a NaN depth (DEPTH), a NaN pixel in all channels (NORMALS), a NaN in that channel (UNIT, NONE);
   * MG_POST_SCHED = the DDIM / LCM update of MG_OP_SCHED_STEP applied to conv_out's result in place of storing it:
   * out <- F_CX * out + F_CM * in + F_CN * noise (out = the latent x_t, NCHW; marigold_depth_pipeline.py:466-468).
   * The slots are named by the MG_POST_NCHW_* enumerators below. */
  MG_OP_POST_NCHW = 15,
  /* im2col of a 3x3 / pad 1 neighbourhood for the <= 8-channel convolutions at the latent / image
   * boundary (conv_in of the UNet incl. the torch.cat of marigold_depth_pipeline.py:456-458, of the
   * VAE encoder and decoder): fp32 NCHW (two sources) -> bf16 [B*H*W][Kp], k = tap*(C0+C1) + c,
   * columns >= 9*(C0+C1) zero.  The convolution itself is then an MG_OP_IGEMM with K = Kp.
   * The slots are named by the MG_IM2COL_SMALL_* enumerators below. */
  MG_OP_IM2COL_SMALL = 16,
  /* Patch-resident conv3x3 (stride 1, pad 1) with the ResNet block's GroupNorm + SiLU fused into the operand staging
   * (diffusers ResnetBlock2D: norm1 -> silu -> conv1, norm2 -> silu -> conv2), the UNet's skip concat folded into the
   * channel loop (torch.cat([hidden, skip]) in the up blocks) and Upsample2D's nearest-2x + conv in sub-pixel form.
   * The slots are named by the MG_CONV3X3_* enumerators below.  Cin = C0 + C1; weights k = (ky*3+kx)*Cin + c (sub-pixel mode:
   * [4][N][4*Cin], parity z = 2a+b, k = (ty*2+tx)*Cin + c - weights.py::pack_conv3x3_subpix, L_SW the parity stride).
   *  Output statistics (P_GN_PART, I_GN_CPG, I_GN_SLOTS): f32 [B][slots][N / cpg][2], (sum, sum of squares) of every group of cpg
   *  (4 | 8 | 16 | 32) output channels over each tile's pixels, of the values as stored - the partial table MG_OP_GN_FINALIZE
   *  reduces (slots = mg_conv3x3_gn_slots(op), HW = H W or 4 H W): the next GroupNorm's statistics without a pass over the tensor. */
  MG_OP_CONV3X3 = 17,
  /* The output heads: GroupNorm apply [+ SiLU] + conv3x3 (pad 1) to <= 4 channels in one launch (conv_norm_out -> conv_act ->
   * conv_out of the UNet and of the VAE decoder - the tail of the modules the reference calls at marigold_depth_pipeline.py:461-463
   * and :498-516; csrc/head_conv.hip: the raw input patch of a pixel tile is normalised on its
   * way into LDS, the taps are packed bf16 dot products - no MFMA work at <= 4 output channels, one HBM read of the input).
   * The slots are named by the MG_CONV3X3_HEAD_* enumerators below. */
  MG_OP_CONV3X3_HEAD = 18,
  /* Test-time ensembling (marigold/util/ensemble.py).
   * DEPTH_STATS : one pass over [E][HW]: per-member min,max,mean and the centred E x E
   *               second-moment matrix (closed form of the pairwise-RMSE cost, :138-145).
   * DEPTH_MEDIAN: aligned = s*d+t; lower-middle median over E (+MAD); block min/max.
   * (DEPTH_STATS scratch: >= nblk*E*(E+3) doubles, nblk = min(ceil(HW / 256), E > 256 ? 32 : 128) - 128*E*(E+3) always suffices.  Any E >= 1: <= 32 members are selected in registers, <= 128 in LDS,
   * larger ensembles by a bitwise selection over the members in memory - the reference has no limit, ensemble.py:39-49)
   * DEPTH_NORM  : out = (med - lo)/range ; unc /= range, in place.
   * NORMALS     : the member closest to the mean direction, or the normalised mean.
   * The slots are named by the MG_ENS_DEPTH_STATS_* / MG_ENS_DEPTH_MEDIAN_* / MG_ENS_DEPTH_NORM_* / MG_ENS_NORMALS_* enumerators below. */
  MG_OP_ENS_DEPTH_STATS = 20,
  MG_OP_ENS_DEPTH_MEDIAN = 21,
  MG_OP_ENS_DEPTH_NORM = 22,
  MG_OP_ENS_NORMALS = 23,
  /* Image resampling either side of the path (marigold/util/image_util.py:90-120, marigold_depth_
   * pipeline.py:306-312, ensemble.py:158-161): torchvision resize(..., antialias=True) semantics.
   * The slots are named by the MG_RESIZE_* enumerators below. */
  MG_OP_RESIZE = 24,
  /* Colour-mapped depth image (marigold/util/image_util.py:38-76 colorize_depth_maps followed by the pipeline's
   * (x * 255).astype(uint8), marigold_depth_pipeline.py:318-327): out[px] = LUT[min(int(clip((d - F_MIN_DEPTH) / (F_MAX_DEPTH -
   * F_MIN_DEPTH), 0, 1) * 256), 255)]; a NaN depth is a black pixel.  The slots are named by the MG_COLORIZE_* enumerators below.
   *  The depth output stage: with P_CLIPPED and / or P_U16 the same launch also stores what the depth pipeline and its command line
   *  keep of the map (marigold_depth_pipeline.py:314-316, script/depth/run.py): clip(d, 0, 1) as numpy.clip gives it (NaN stays, +-inf ->
   *  1 / 0, -0.0 stays) and uint16(clip(d, 0, 1) * 65535) - one fp32 product, truncated; NaN -> 0 (MG_OP_IID_VIS's convention).  Both
   *  are defined for F_MIN_DEPTH = 0, F_MAX_DEPTH = 1 only; P_OUT (and with it P_LUT) is then optional.  P_CLIPPED may be P_DEPTH.  A lane
   *  owns four neighbouring elements (16-byte load, 16- / 8- / 12-byte stores) when n % 4 == 0 and every pointer given is aligned for
   *  its access, else one element.  With both NULL the colour bytes are those of the op without them. */
  MG_OP_COLORIZE = 25,
  /* Scoring of one prediction against its ground truth on the device (the validation loop of the reference,
   * src/trainer/marigold_depth_trainer.py:510-601, with src/util/alignment.py and src/util/metric.py; csrc/evalscore.hip).
   * Every sum is fp64 and reduced wave -> block -> a per-block partial table -> one block that adds the table in block order:
   * no floating-point atomics, the same bits on every launch.  Pixels outside the mask never enter a sum.
   * EVAL_DEPTH_LS: the five sums n, Sx, Sy, Sxx, Sxy of the least-squares fit gt ~ s * pred + t over the valid pixels
   *   (align_depth_least_square, alignment.py:35-82).
   * EVAL_DEPTH_METRICS: a = clip(clip(pred * s + t)) per valid pixel in fp32 (scale and shift from P_SUMS by the 2 x 2 normal equations in
   *   fp64, cast to fp32; disparity: a = 1 / max(a, 1e-3); then [min_depth, max_depth], then the 1e-6 floor) and the ten scores of
   *   script/depth/eval.py:58-69 (metric.py:64-199), finished in fp64.
   * EVAL_NORMALS: per-pixel angle in degrees (compute_cosine_error, metric.py:206-233) and its statistics; the median is exact
   *   (np.median: mean of the two middle order statistics), by a three-pass radix selection on the angles' bit patterns.
   * The slots are named by the MG_EVAL_DEPTH_LS_* / MG_EVAL_DEPTH_METRICS_* / MG_EVAL_NORMALS_* enumerators below. */
  MG_OP_EVAL_DEPTH_LS = 26,
  MG_OP_EVAL_DEPTH_METRICS = 27,
  MG_OP_EVAL_NORMALS = 28,
  MG_OP_MEMSET = 30, /* hipMemsetAsync; the slots are named by the MG_MEMSET_* enumerators below */
  MG_OP_COPY = 31,   /* hipMemcpyAsync, device to device; the slots are named by the MG_COPY_* enumerators below */
  /* Scoring of one intrinsic-image target (albedo, shading, ...) against its ground truth on the device: compute_iid_metric of the
   * reference (src/util/metric.py:263-338) with the PSNR / SSIM of torchmetrics it is called with (script/iid/eval.py); same
   * file, same reduction scheme and the same guarantees as the EVAL ops above.  The three ops share their fields, slot for slot (one op
   * can be launched as each kind in turn, as mg_eval_iid does): the MG_IIDSCORE_PREP_* / MG_IIDSCORE_PSNR_* / MG_IIDSCORE_SSIM_*
   * enumerators below.  P_OUT f64 [8] = psnr, ssim, alignment scale, quantile, brightness scale, valid elements, two reserved slots (at
   * present PREP leaves the two order statistics of its quantile there for the tests: not part of the interface); PREP leaves the
   * mapping in P_WS for the two score ops of the same target, which map both images on load with it (they are never stored).
   * IIDSCORE_PREP (shading, residual): s = S p g / S p p over the valid elements in fp64 (compute_alignment_scale, :319-334);
   *   the brightness 0.3 g0 + 0.59 g1 + 0.11 g2 of the ground truth over the pixels of mask channel 0, its 0.9 quantile q with
   *   linear interpolation at the fp32 position 0.9 (n - 1) like torch.quantile / np.quantile - the two order statistics are
   *   exact, by the radix selection of EVAL_NORMALS on order-preserving keys; scale = q < 1e-4 ? 0 : 0.8 / q (quantile_map,
   *   :337-375).  The mapping is pred <- clamp(scale * (fp32(s) * pred), 0, 1), gt <- clamp(scale * gt, 0, 1).  Writes out[2],
   *   out[3], out[4] and the reserved slots (no pixel: NaN).  Slot 3 of i (the score ops' I_UP_TO_SCALE) is ignored.
   * IIDSCORE_PSNR: 10 log10(1 / mean(d^2)) over the valid elements, d taken in fp64 (identical images: +inf); writes out[5], out[0]
   *   when I_WRITE_PSNR != 0 and, for a plain target, out[2] = out[4] = 1 (no valid element: NaN).
   * IIDSCORE_SSIM: mean SSIM (11 x 11 Gaussian window, sigma 1.5, c1 = 1e-4, c2 = 9e-4, reflect padding by 5 and the padded border
   *   cropped: 3 (H - 10)(W - 10) values) with the invalid elements of both images set to 0; the five window moments are fp64 sums of
   *   exact products; needs H, W >= 11; writes out[1] (no valid element: NaN). */
  MG_OP_IIDSCORE_PREP = 32,
  MG_OP_IIDSCORE_PSNR = 33,
  MG_OP_IIDSCORE_SSIM = 34,
  /* The intrinsic-image output stage (MarigoldIIDOutput.fill_entry, marigold/marigold_iid_pipeline.py:117-136) for all targets of one
   * image: per target, if linear and up to scale x <- x / max(max over its 3 H W elements, 1e-6) (IEEE division, the maximum keeps
   * NaN); if linear x <- powf(x, fp32(1 / 2.2)); then (x * 255).astype(uint8) as x86-64 numpy does it: truncation to int32, low 8
   * bits; NaN and |x * 255| >= 2^31 -> 0.  At most two launches (the maxima, skipped when no target needs one; the map), no atomics:
   * the same bits on every launch.  The slots are named by the MG_IID_VIS_* enumerators below. */
  MG_OP_IID_VIS = 35,
  /* The two remaining ends of the device I/O boundary (csrc/resize.hip); they take free numbers below the last kind.  Their slots are
   * named by the MG_RGB_PREP_* / MG_NORMALS_VIS_* enumerators below.
   * RGB_PREP: the input stage of every pipeline (marigold/marigold_depth_pipeline.py:229-255: pil_to_tensor, resize_max_res,
   *   `rgb / 255.0 * 2.0 - 1.0`, the cast to the pipeline's dtype) on the uint8 picture as uploaded: [Hin][Win][3] (PIL's layout, I_HWC)
   *   or [3][Hin][Win] -> [3][Hout][Wout] in fp32 or the build's 16-bit operand type (I_OUT16).  Same size: one launch.  Sizes
   *   differ: MG_OP_RESIZE's launches on the three planes with the uint8 rounding (bicubic: the clamp first) and the normalisation in
   *   the last one's store - no uint8 intermediate.  The normalisation is torch's, rounding for rounding, in fp32: x / 255 (IEEE
   *   division: the host kernel) or x * fp32(1 / 255) (I_RECIPROCAL: what torch's device kernel makes of a division by a scalar), then
   *   * 2, then - 1.
   * NORMALS_VIS: the normals picture (marigold/marigold_normals_pipeline.py:297-301), the counterpart of MG_OP_COLORIZE: fp32
   *   [3][H][W] -> uint8 [H][W][3], out = uint8((clip(x, -1, 1) + 1) * 127.5) - the clip keeps NaN like numpy.clip, the sum and the
   *   product are two fp32 roundings, the cast truncates; NaN -> 0 (MG_OP_IID_VIS's convention).  (The call mg_normals_finish runs
   *   the same kernel and can also store the clipped map; the op's fields are the two pointers below and stay so.) */
  MG_OP_RGB_PREP = 5,
  MG_OP_NORMALS_VIS = 8,
  /* Gaussian noise without a host generator (csrc/randn.hip): what torch.randn(generator=...) is to the reference's initial latents
   * and LCM step noises (marigold/marigold_depth_pipeline.py:430-435, :466-468), for hosts that have no torch.  Stateless:
   * Philox4x32-10 (Salmon et al., SC'11; Random123's constants) with key = (seed lo, seed hi) and counter = (block lo, block hi,
   * stream lo, stream hi); element L_OFFSET + i of the stream is word (L_OFFSET + i) % 4 of block (L_OFFSET + i) / 4 and depends on
   * nothing else - not on the grid, on L_N or on where a draw was split.  Words (0, 1) and (2, 3) of a block are two Box-Muller pairs
   * (a, b): u = ((a >> 9) + 1) 2^-23 in (0, 1], v = (b >> 8) 2^-24, r = sqrtf(-2 logf(u)), outputs r cospi(2 v) and r sinpi(2 v);
   * |z| <= sqrt(46 ln 2) = 5.647.  The 16-bit store rounds the fp32 value to nearest even.  A free number below the last kind; the
   * slots are named by the MG_RANDN_* enumerators below. */
  MG_OP_RANDN = 29,
  /* Test-time ensembling of the intrinsic-image members (ensemble_iid, marigold/util/ensemble.py:252-270; csrc/ensemble.hip): a
   * reduction over the E members of every element on its own - P_PREDS fp32 [E][n] -> P_PRED [n] and, when P_UNC is not NULL,
   * P_UNC [n].  I_REDUCTION 0: the median, the lower middle value for an even E as torch.median gives it, with the median of the
   * absolute deviations from it (same rule) as the uncertainty; 1: the mean (the members added in order, divided by E) with the
   * unbiased standard deviation.  A NaN member makes both results of its element NaN.  No alignment, no extrema: the op has no
   * min / max table, no scratch and no atomics, leaves nothing to zero between launches and gives the same bits on every launch -
   * those of MG_OP_ENS_DEPTH_MEDIAN without alignment, whose selection and summation order it keeps.  Any E >= 1: up to 32 members
   * are selected in registers, larger ensembles straight from memory.  A lane owns four neighbouring elements (one 16-byte load
   * per member, one 16-byte store per output) when n % 4 == 0, E <= 32 and the three pointers are 16-byte aligned, else one element.  The
   * free number below the first ensembling kind; the slots are named by the MG_ENS_IID_* enumerators below. */
  MG_OP_ENS_IID = 19
};
#define MG_IID_VIS_PARTS 128

enum { MG_EPI_BF16 = 0, MG_EPI_GEGLU = 1, MG_EPI_F32 = 2,
       MG_EPI_SOFTMAX2 = 3 /* bf16 out = softmax over column pairs (2h, 2h+1) of F_SM_SCALE * acc; I_SM_COLS = real columns, the rest -> 0:
                              the collapsed 2-token cross-attention's probabilities straight from the scores GEMM */,
       MG_EPI_XATTN2 = 4   /* the whole collapsed cross-attention in one launch (diffusers Attention with a 2-token context,
                              BasicTransformerBlock.attn2): N = 64 score columns as in MG_EPI_SOFTMAX2; the probabilities stay in
                              registers as the operand of a second MFMA stage against P_OUT2 = W2 bf16 [I_C2][64] (the context's
                              values pushed through to_out), out[M][I_C2] = P W2^T + bias (P_BIAS, of the second stage) + residual
                              (P_RESIDUAL); P_LN_OUT = f32 [M][2] (mean, rstd) of the OUTPUT rows (one wave owns whole rows: no slots, no
                              ticket).  out may alias A and the residual (a row block belongs to one workgroup). */ };
enum { MG_POST_NONE = 0, MG_POST_DEPTH = 1, MG_POST_NORMALS = 2, MG_POST_UNIT = 3 /* IID: clip, (x+1)/2 */,
       MG_POST_SCHED = 4 /* scheduler update in place of the store, see MG_OP_POST_NCHW */ };

typedef struct mg_op {
  int32_t kind;
  int32_t i[40];
  float f[8];
  void* p[16];
  int64_t l[4];
} mg_op;

/* Field names of every kind: MG_<KIND>_<array>_<NAME> is the index of that field in mg_op's i / f / p / l array (<KIND> is the kind's name
 * without MG_OP_; MG_OP_FLASH_ATTN64's is FLASH64).  This is the one table of the wire format (the values are positions: they never change, new fields are appended);
 * marigold_amd/_lib.py mirrors it (tests/test_host.py compares the two) and marigold_amd/ops.py decodes an op by these names. */
enum mg_igemm_i {
  MG_IGEMM_I_B = 0,             /* images */
  MG_IGEMM_I_H = 1,             /* input height */
  MG_IGEMM_I_W = 2,             /* input width */
  MG_IGEMM_I_CIN = 3,           /* input channels (both sources together; % 64 == 0) */
  MG_IGEMM_I_HO = 4,            /* output height */
  MG_IGEMM_I_WO = 5,            /* output width: M = B * Ho * Wo rows */
  MG_IGEMM_I_N = 6,             /* output columns */
  MG_IGEMM_I_TAPS = 7,          /* 1 | 9 | 4 = the sub-pixel form of nearest-2x + conv3x3: batch_z = 4 output parities, see MG_OP_CONV3X3 */
  MG_IGEMM_I_STRIDE = 8,
  MG_IGEMM_I_PAD = 9,
  MG_IGEMM_I_HU = 10,           /* virtual nearest-up-sampled input height (0 = none) */
  MG_IGEMM_I_WU = 11,           /* ... and width */
  MG_IGEMM_I_EPI = 12,          /* epilogue (MG_EPI_*) */
  MG_IGEMM_I_LDO = 13,          /* row stride of out */
  MG_IGEMM_I_TRANS_FROM = 14,   /* columns >= this go to out2 as [img][n - trans_from][ldt] transposed; -1 = none */
  MG_IGEMM_I_BATCH_Z = 15,      /* batched GEMMs (0 = 1), strides in l[] */
  MG_IGEMM_I_LDR = 16,          /* row stride of the residual (0 = N) */
  MG_IGEMM_I_LDA = 17,          /* row stride of A (0 = C0, the channels A holds) */
  MG_IGEMM_I_LDT = 18,          /* row stride of the transposed section */
  MG_IGEMM_I_VARIANT = 19,      /* tile variant: 0 = automatic; 22-26, 29, 32, 35, 36, 46, 51, 54, 62, 72, 73 force a tile (the tuning
                                   table, its sweep and the parity tests - igemm2.hip::dispatch_tile) */
  MG_IGEMM_I_LDW = 20,          /* row stride of Wt (0 = taps * Cin + Cx) */
  MG_IGEMM_I_ROWVEC_BCAST = 21, /* 1 = rowvec is a single [N] row shared by every image */
  MG_IGEMM_I_N_ALG = 22,        /* un-padded N for FLOP accounting (0 = as launched; ignored by the kernel) */
  MG_IGEMM_I_K_ALG = 23,        /* un-padded K for FLOP accounting (0 = as launched; ignored by the kernel) */
  MG_IGEMM_I_C0 = 24,           /* with A1: the channels A holds (% 64 == 0) */
  MG_IGEMM_I_LDA1 = 25,         /* row stride of A1 (0 = Cin - C0) */
  MG_IGEMM_I_TRANS_PERM = 26,   /* 1 = the transposed section stores its tokens in accumulator order inside groups of 16 (MG_FLASH64_I_VT_PERM) */
  MG_IGEMM_I_SM_COLS = 27,      /* MG_EPI_SOFTMAX2 / _XATTN2: real score columns, the rest -> 0 */
  MG_IGEMM_I_C2 = 28,           /* MG_EPI_XATTN2: output channels of the second stage */
  MG_IGEMM_I_TICKETS_LO = 29,   /* low / high 32 bits of the device address of the caller's row-block tickets for the P_LN_OUT */
  MG_IGEMM_I_TICKETS_HI = 30,   /* hand-off (65536 zeroed uint32, one buffer per program / stream; 0 = the library's global buffer: single stream only) */
  MG_IGEMM_I_SPLITS = 31,       /* split-K: 0 = automatic (few output tiles x long K: fp32 partials + a fixed-order reduce launch), n >= 1 =
                                   exactly n K ranges per tile (1 = none) - bf16 epilogue without row statistics / folded LayerNorm / batching only */
  MG_IGEMM_I_CX = 32,           /* folded shortcut: its input channels (% 64 == 0) */
  MG_IGEMM_I_CX0 = 33,          /* ... of which X0 holds the first Cx0 (with X1) */
  MG_IGEMM_I_LDX0 = 34,         /* row stride of X0 (0 = the channels it holds) */
  MG_IGEMM_I_LDX1 = 35          /* row stride of X1 (0 = Cx - Cx0) */
};
enum mg_igemm_f {
  MG_IGEMM_F_SCALE = 0,         /* scale on the accumulator (0 = 1) */
  MG_IGEMM_F_LN_EPS = 1,        /* eps of the statistics written to P_LN_OUT */
  MG_IGEMM_F_SM_SCALE = 2       /* softmax scale of MG_EPI_SOFTMAX2 / _XATTN2 */
};
enum mg_igemm_p {
  MG_IGEMM_P_A = 0,             /* bf16 [B][H][W][lda >= C0] */
  MG_IGEMM_P_WT = 1,            /* bf16 [N][ldw >= taps * Cin], k = (ky*3+kx)*Cin + c */
  MG_IGEMM_P_OUT = 2,
  MG_IGEMM_P_BIAS = 3,          /* f32 [N] | NULL */
  MG_IGEMM_P_ROWVEC = 4,        /* f32 [B][N] | NULL (time-embedding add) */
  MG_IGEMM_P_RESIDUAL = 5,      /* bf16 [M][ldr] | NULL */
  MG_IGEMM_P_OUT2 = 6,          /* the transposed section (MG_EPI_XATTN2: W2 bf16 [c2][64]) */
  MG_IGEMM_P_A1 = 7,            /* bf16 [B][H][W][lda1] | NULL: second channel source */
  MG_IGEMM_P_LN_OUT = 8,        /* f32 [M][N/32 + 1][2] | NULL: row statistics of the output (MG_EPI_XATTN2: f32 [M][2]) */
  MG_IGEMM_P_LN_IN = 9,         /* f32 [M][2] (mean, rstd) | NULL: LayerNorm folded into this layer */
  MG_IGEMM_P_LN_G = 10,         /* f32 [N] */
  MG_IGEMM_P_LN_C = 11,         /* f32 [N] */
  MG_IGEMM_P_X0 = 12,           /* bf16 [B][H][W][ldx0] | NULL: folded shortcut's input */
  MG_IGEMM_P_X1 = 13,           /* bf16 [B][H][W][ldx1] | NULL: its second source */
  MG_IGEMM_P_SPLITK_WS = 14     /* split-K workspace of the caller (64 MiB, 16-byte aligned) | NULL = the library's own, which programs on ONE
                                   stream may share (stream-ordered reuse); programs that run concurrently on several streams each bring their own */
};
enum mg_igemm_l { MG_IGEMM_L_SA = 0, MG_IGEMM_L_SW = 1, MG_IGEMM_L_SO = 2, MG_IGEMM_L_SR = 3 };   /* z-strides (elements) of A, Wt, out, residual */

enum mg_conv3x3_i {
  MG_CONV3X3_I_B = 0,
  MG_CONV3X3_I_H = 1,
  MG_CONV3X3_I_W = 2,
  MG_CONV3X3_I_C0 = 3,            /* channels of A0 (% 64 == 0) */
  MG_CONV3X3_I_C1 = 4,            /* channels of A1 (0 without) */
  MG_CONV3X3_I_N = 5,             /* output channels */
  MG_CONV3X3_I_SUBPIX = 6,        /* sub-pixel 2x mode */
  MG_CONV3X3_I_SILU = 7,          /* SiLU after the fused scale / shift */
  MG_CONV3X3_I_LDA0 = 8,          /* row strides, 0 = dense: C0, */
  MG_CONV3X3_I_LDA1 = 9,          /* C1, */
  MG_CONV3X3_I_LDO = 10,          /* N, */
  MG_CONV3X3_I_LDR = 11,          /* N, */
  MG_CONV3X3_I_LDW = 12,          /* 9 * Cin (sub-pixel: 4 * Cin) */
  MG_CONV3X3_I_ROWVEC_BCAST = 13, /* 1 = rowvec is a single [N] row shared by every image */
  MG_CONV3X3_I_VARIANT = 14,      /* tile variant (0 = automatic) */
  MG_CONV3X3_I_GN_CPG = 15,       /* channels per group of the output statistics (4 | 8 | 16 | 32) */
  MG_CONV3X3_I_GN_SLOTS = 16      /* slots per image of their table = mg_conv3x3_gn_slots(op) */
};
enum mg_conv3x3_p {
  MG_CONV3X3_P_A0 = 0,            /* bf16 [B][H][W][lda0 >= C0] */
  MG_CONV3X3_P_WT = 1,            /* bf16 [N][ldw >= 9 * Cin] */
  MG_CONV3X3_P_OUT = 2,           /* bf16 [B][H][W][ldo] (sub-pixel: [B][2H][2W][ldo]) */
  MG_CONV3X3_P_BIAS = 3,          /* f32 [N] | NULL */
  MG_CONV3X3_P_ROWVEC = 4,        /* f32 [B][N] | NULL */
  MG_CONV3X3_P_RESIDUAL = 5,      /* bf16 (out's shape, row stride ldr) | NULL */
  MG_CONV3X3_P_A1 = 6,            /* bf16 [B][H][W][lda1 >= C1] | NULL (second channel source) */
  MG_CONV3X3_P_SS = 7,            /* scale_shift f32 [B][2][Cin] | NULL: input = silu?(x * scale + shift) for in-image pixels
                                     (MG_OP_GN_FINALIZE's output; zero padding stays zero) */
  MG_CONV3X3_P_GN_PART = 8        /* (optional) the output's GroupNorm partial sums, see the op */
};
enum mg_conv3x3_l { MG_CONV3X3_L_SW = 0 };   /* parity stride of Wt in elements (sub-pixel mode) */

enum mg_rowgemm_i {
  MG_ROWGEMM_I_M = 0,
  MG_ROWGEMM_I_K = 1,
  MG_ROWGEMM_I_N = 2,
  MG_ROWGEMM_I_LDX = 3,           /* row strides, 0 = dense: K, */
  MG_ROWGEMM_I_LDO = 4,           /* N (GEGLU: N / 2; form 3: K), */
  MG_ROWGEMM_I_LDR = 5,           /* N */
  MG_ROWGEMM_I_FORM = 6,          /* 0 plain, 1 GEGLU, 2 QKV, 3 collapsed cross-attention - see the op */
  MG_ROWGEMM_I_TOKENS = 7,        /* tokens per image (forms with P_VT / P_GN_SS; % 32 == 0) */
  MG_ROWGEMM_I_LDT = 8,           /* row stride of V^T */
  MG_ROWGEMM_I_TRANS_FROM = 9,    /* first V column (% 64 == 0) */
  MG_ROWGEMM_I_WAVES = 10,        /* waves per workgroup (0 = 12; 4 / 8 / 12; K = 640: 0 | 8) */
  MG_ROWGEMM_I_SM_COLS = 11,      /* 2 x heads live score columns (form 3, P_XATTN) */
  MG_ROWGEMM_I_NSPLIT = 12        /* column split (0 / 1 = none; n: the N / 64 stages are shared out over n workgroups per row block - few
                                     rows, many columns; not with P_LN_OUT) */
};
enum mg_rowgemm_f {
  MG_ROWGEMM_F_LN_EPS = 0,        /* LayerNorm eps of P_LN_OUT */
  MG_ROWGEMM_F_SM_SCALE = 1       /* softmax scale (form 3, P_XATTN) */
};
enum mg_rowgemm_p {
  MG_ROWGEMM_P_X = 0,             /* bf16 [M][ldx] */
  MG_ROWGEMM_P_WP = 1,            /* packed weights */
  MG_ROWGEMM_P_OUT = 2,           /* bf16 [M][ldo] */
  MG_ROWGEMM_P_RESIDUAL = 3,      /* bf16 [M][ldr] | NULL (may alias out) */
  MG_ROWGEMM_P_LN_IN = 4,         /* (mean, rstd) f32 [M][2] of the rows of x | NULL: LayerNorm folded (the packed trailer holds its g and c vectors) */
  MG_ROWGEMM_P_LN_OUT = 5,        /* (mean, rstd) f32 [M][2] of the OUTPUT rows | NULL */
  MG_ROWGEMM_P_VT = 6,            /* V^T bf16 [B][N - trans_from][ldt] (QKV form) */
  MG_ROWGEMM_P_GN_SS = 7,         /* GroupNorm scale/shift f32 [B][2][K] | NULL: x is normalised while it is loaded (bf16(x * scale + shift)) */
  MG_ROWGEMM_P_DBG = 8,           /* (tuning only) per-wave phase cycle stamps | NULL */
  MG_ROWGEMM_P_XATTN = 9,         /* a weights.pack_rowgemm_xattn image | NULL: the cross-attention prologue of the GEGLU form */
  MG_ROWGEMM_P_XOUT = 10          /* bf16 [M][ldx]: where the prologue writes the updated rows */
};

enum mg_flash64_i {
  MG_FLASH64_I_B = 0,
  MG_FLASH64_I_HEADS = 1,
  MG_FLASH64_I_NTOK = 2,
  MG_FLASH64_I_LDQ = 3,           /* row stride of Q and K */
  MG_FLASH64_I_LDO = 4,
  MG_FLASH64_I_LDVT = 5,
  MG_FLASH64_I_VARIANT = 6,       /* 0 = automatic; 19 / 20 / 21 / 25 force a form of the compiled kernel, 26 / 27 the hand-placed stream */
  MG_FLASH64_I_VT_PERM = 7,       /* 1 = Vt's keys are in the order [0-3, 8-11, 4-7, 12-15] inside every group of 16 (as written by
                                     MG_IGEMM_I_TRANS_PERM; Ntok % 16 == 0) */
  MG_FLASH64_I_WS_KB = 8,         /* size of P_WS in KB */
  MG_FLASH64_I_SPLIT = 9          /* key split of the left-over blocks: 0 = when it pays, 1 = always, 2 = never */
};
enum mg_flash64_f {
  MG_FLASH64_F_SCALE = 0,         /* softmax scale */
  MG_FLASH64_F_REDO_THR = 1       /* row-sum bound of the running-maximum fallback (0 = 2^100; tests force the fallback with a tiny value) */
};
enum mg_flash64_p {
  MG_FLASH64_P_Q = 0,             /* bf16 (row stride ldq) */
  MG_FLASH64_P_K = 1,             /* bf16 (row stride ldq) */
  MG_FLASH64_P_VT = 2,            /* bf16 [B][heads*64][ldvt] */
  MG_FLASH64_P_O = 3,             /* bf16 (row stride ldo) */
  MG_FLASH64_P_DBG = 4,           /* tuning only: cycle stamps | NULL */
  MG_FLASH64_P_WS = 5             /* workspace | NULL (16-byte aligned, ZEROED once by the caller, then owned by this op's launches on ONE stream -
                                     tickets return to zero); 4 KB + 69 632 bytes x 4 x (blocks % CUs) suffice */
};
enum mg_flash64_l { MG_FLASH64_L_SQ = 0, MG_FLASH64_L_SK = 1, MG_FLASH64_L_SVT = 2, MG_FLASH64_L_SO = 3 };   /* batch strides of Q, K, Vt, O */

enum mg_rgb_prep_i {
  MG_RGB_PREP_I_HIN = 0,          /* source height */
  MG_RGB_PREP_I_WIN = 1,          /* source width */
  MG_RGB_PREP_I_HOUT = 2,         /* destination height */
  MG_RGB_PREP_I_WOUT = 3,         /* destination width */
  MG_RGB_PREP_I_MODE = 4,         /* when the sizes differ: 0 bilinear, 1 bicubic, 2 nearest-exact (MG_OP_RESIZE's modes) */
  MG_RGB_PREP_I_HWC = 5,          /* 1 = the source is [Hin][Win][3] (3-byte pixels), 0 = [3][Hin][Win] planes */
  MG_RGB_PREP_I_OUT16 = 6,        /* 1 = the destination holds the build's 16-bit operand type (bf16 / fp16), 0 = fp32 */
  MG_RGB_PREP_I_RECIPROCAL = 7    /* 1 = x * fp32(1 / 255) in place of the IEEE division x / 255 */
};
enum mg_rgb_prep_p {
  MG_RGB_PREP_P_SRC = 0,          /* uint8, any alignment (four pixels per lane when Win % 4 == 0 and it is 4-byte aligned) */
  MG_RGB_PREP_P_DST = 1,          /* [3][Hout][Wout] */
  MG_RGB_PREP_P_TMP = 2           /* f32 [3][Hin][Wout] | NULL: needed by bilinear / bicubic when both sizes change */
};
enum mg_normals_vis_i {
  MG_NORMALS_VIS_I_H = 0,
  MG_NORMALS_VIS_I_W = 1
};
enum mg_normals_vis_p {
  MG_NORMALS_VIS_P_PRED = 0,      /* f32 [3][H][W], 4-byte aligned (four pixels per lane when H W % 4 == 0 and it is 16-byte aligned) */
  MG_NORMALS_VIS_P_OUT = 1        /* uint8 [H][W][3] */
};

enum mg_randn_i {
  MG_RANDN_I_MODE = 0,            /* 0 = normals, 1 = the raw uint32 words (dst uint32 [n]; tests and debugging) */
  MG_RANDN_I_OUT16 = 1            /* 1 = the destination holds the build's 16-bit operand type (bf16 / fp16), 0 = fp32; mode 0 only */
};
enum mg_randn_p {
  MG_RANDN_P_DST = 0              /* [n], aligned to its element (a lane stores a block of four at once when that address is 16- / 8-byte aligned) */
};
enum mg_randn_l {
  MG_RANDN_L_N = 0,               /* elements to draw (>= 1) */
  MG_RANDN_L_OFFSET = 1,          /* index of the first one in its stream (>= 0; offset + n <= 2^62) */
  MG_RANDN_L_SEED = 2,            /* the 64-bit seed (the bits of a uint64) */
  MG_RANDN_L_STREAM = 3           /* the 64-bit stream id: independent sequences of one seed */
};

enum mg_ens_iid_i {
  MG_ENS_IID_I_E = 0,             /* members (>= 1) */
  MG_ENS_IID_I_REDUCTION = 1      /* 0 = median (+ median absolute deviation), 1 = mean (+ unbiased standard deviation) */
};
enum mg_ens_iid_p {
  MG_ENS_IID_P_PREDS = 0,         /* f32 [E][n], 4-byte aligned */
  MG_ENS_IID_P_PRED = 1,          /* f32 [n] */
  MG_ENS_IID_P_UNC = 2            /* f32 [n] | NULL: no uncertainty is computed */
};
enum mg_ens_iid_l {
  MG_ENS_IID_L_N = 0              /* elements per member (>= 1) */
};

enum mg_gn_stats_i {
  MG_GN_STATS_I_B = 0,
  MG_GN_STATS_I_HW = 1,
  MG_GN_STATS_I_C = 2,            /* channels of x */
  MG_GN_STATS_I_CHUNKS = 3,       /* blocks per image and source */
  MG_GN_STATS_I_CTOT = 4,         /* channels of the whole norm (0 = C) */
  MG_GN_STATS_I_COFF = 5,         /* first channel of the norm that x holds */
  MG_GN_STATS_I_GROUPS = 6,
  MG_GN_STATS_I_SLOT0 = 7,        /* first slot this launch writes */
  MG_GN_STATS_I_SLOTS = 8,        /* slots per image of the table (0 = chunks) */
  MG_GN_STATS_I_C1 = 9            /* channels of x1 */
};
enum mg_gn_stats_f { MG_GN_STATS_F_EPS = 0 };
enum mg_gn_stats_p {
  MG_GN_STATS_P_X = 0,            /* bf16 [B][HW][C] */
  MG_GN_STATS_P_PARTIALS = 1,     /* f32 [B][slots][groups][2], 8-byte aligned */
  MG_GN_STATS_P_GAMMA = 2,        /* f32 [Ctot] (fused finalize) */
  MG_GN_STATS_P_BETA = 3,         /* f32 [Ctot] (fused finalize) */
  MG_GN_STATS_P_SS = 4,           /* scale_shift f32 [B][2][Ctot] | NULL = no fused finalize */
  MG_GN_STATS_P_COUNTERS = 5,     /* uint32 [B] arrival counters (zero before the first use; left zero) */
  MG_GN_STATS_P_X1 = 6            /* bf16 [B][HW][C1] | NULL: second source */
};
enum mg_gn_finalize_i {
  MG_GN_FINALIZE_I_B = 0,
  MG_GN_FINALIZE_I_C = 1,
  MG_GN_FINALIZE_I_GROUPS = 2,
  MG_GN_FINALIZE_I_SLOTS = 3,
  MG_GN_FINALIZE_I_HW = 4
};
enum mg_gn_finalize_f { MG_GN_FINALIZE_F_EPS = 0 };
enum mg_gn_finalize_p {
  MG_GN_FINALIZE_P_PARTIALS = 0,  /* f32 [B][slots][groups][2] */
  MG_GN_FINALIZE_P_GAMMA = 1,     /* f32 [C] */
  MG_GN_FINALIZE_P_BETA = 2,      /* f32 [C] */
  MG_GN_FINALIZE_P_SS = 3         /* scale_shift f32 [B][2][C] */
};
enum mg_gn_apply_i {
  MG_GN_APPLY_I_B = 0,
  MG_GN_APPLY_I_HW = 1,
  MG_GN_APPLY_I_C = 2,
  MG_GN_APPLY_I_SILU = 3,
  MG_GN_APPLY_I_C0 = 4            /* with x1: the channels x holds */
};
enum mg_gn_apply_p {
  MG_GN_APPLY_P_X = 0,            /* bf16 [B][HW][C] (with x1: [B][HW][C0]) */
  MG_GN_APPLY_P_SS = 1,           /* scale_shift f32 [B][2][C] */
  MG_GN_APPLY_P_OUT = 2,          /* bf16 [B][HW][C] */
  MG_GN_APPLY_P_X1 = 3            /* bf16 [B][HW][C - C0] | NULL */
};
enum mg_gn_slab_i {
  MG_GN_SLAB_I_B = 0,
  MG_GN_SLAB_I_HW = 1,
  MG_GN_SLAB_I_C = 2,
  MG_GN_SLAB_I_C0 = 3,            /* with x1: the channels x0 holds */
  MG_GN_SLAB_I_GROUPS = 4,
  MG_GN_SLAB_I_SILU = 5
};
enum mg_gn_slab_f { MG_GN_SLAB_F_EPS = 0 };
enum mg_gn_slab_p {
  MG_GN_SLAB_P_X0 = 0,            /* bf16 [B][HW][C0] */
  MG_GN_SLAB_P_X1 = 1,            /* bf16 [B][HW][C - C0] | NULL (second channel source: the UNet's skip concat) */
  MG_GN_SLAB_P_OUT = 2,           /* bf16 [B][HW][C] | NULL (statistics only) */
  MG_GN_SLAB_P_GAMMA = 3,         /* f32 [C] */
  MG_GN_SLAB_P_BETA = 4,          /* f32 [C] */
  MG_GN_SLAB_P_SS = 5             /* scale_shift f32 [B][2][C] */
};

enum mg_flash_attn512_i {
  MG_FLASH_ATTN512_I_B = 0,
  MG_FLASH_ATTN512_I_NTOK = 1,
  MG_FLASH_ATTN512_I_LDQ = 2,     /* row stride of Q and K */
  MG_FLASH_ATTN512_I_LDO = 3,
  MG_FLASH_ATTN512_I_LDVT = 4     /* >= Ntok rounded up to 32 */
};
enum mg_flash_attn512_f { MG_FLASH_ATTN512_F_SCALE = 0 };   /* softmax scale */
enum mg_flash_attn512_p {
  MG_FLASH_ATTN512_P_Q = 0,       /* bf16 (row stride ldq) */
  MG_FLASH_ATTN512_P_K = 1,       /* bf16 (row stride ldq) */
  MG_FLASH_ATTN512_P_VT = 2,      /* bf16 [B][512][ldvt] (natural key order, pad columns zero) */
  MG_FLASH_ATTN512_P_O = 3        /* bf16 (row stride ldo) */
};
enum mg_flash_attn512_l { MG_FLASH_ATTN512_L_SQ = 0, MG_FLASH_ATTN512_L_SK = 1, MG_FLASH_ATTN512_L_SVT = 2, MG_FLASH_ATTN512_L_SO = 3 };   /* batch strides of Q, K, Vt, O */

enum mg_softmax_rows_i {
  MG_SOFTMAX_ROWS_I_R = 0,        /* rows */
  MG_SOFTMAX_ROWS_I_NCOLS = 1,
  MG_SOFTMAX_ROWS_I_LDS = 2,      /* row stride of the scores */
  MG_SOFTMAX_ROWS_I_LDP = 3       /* row stride of the probabilities (pad columns zeroed) */
};
enum mg_softmax_rows_p {
  MG_SOFTMAX_ROWS_P_SCORES = 0,   /* f32 [R][lds] */
  MG_SOFTMAX_ROWS_P_PROBS = 1     /* bf16 [R][ldp] */
};

enum mg_sched_step_f { MG_SCHED_STEP_F_CX = 0, MG_SCHED_STEP_F_CM = 1, MG_SCHED_STEP_F_CN = 2 };   /* coefficients of x, model_out, noise */
enum mg_sched_step_p {
  MG_SCHED_STEP_P_X = 0,          /* f32 [n] */
  MG_SCHED_STEP_P_MODEL_OUT = 1,  /* f32 [n] */
  MG_SCHED_STEP_P_NOISE = 2,      /* f32 [n] | NULL */
  MG_SCHED_STEP_P_OUT = 3         /* f32 [n] */
};
enum mg_sched_step_l { MG_SCHED_STEP_L_N = 0 };   /* elements */

enum mg_linear_small_m_i {
  MG_LINEAR_SMALL_M_I_M = 0,
  MG_LINEAR_SMALL_M_I_N = 1,
  MG_LINEAR_SMALL_M_I_K = 2,
  MG_LINEAR_SMALL_M_I_ACT_IN = 3,   /* 0 none, 1 silu */
  MG_LINEAR_SMALL_M_I_ACT_OUT = 4,  /* 0 none, 1 silu */
  MG_LINEAR_SMALL_M_I_LDO = 5       /* row stride of out (0 = N) */
};
enum mg_linear_small_m_p {
  MG_LINEAR_SMALL_M_P_X = 0,      /* f32 [M][K] */
  MG_LINEAR_SMALL_M_P_W = 1,      /* f32 [N][K] */
  MG_LINEAR_SMALL_M_P_BIAS = 2,   /* f32 [N] | NULL */
  MG_LINEAR_SMALL_M_P_OUT = 3     /* f32 [M][ldo] */
};

enum mg_latent_1x1_i { MG_LATENT_1X1_I_B = 0, MG_LATENT_1X1_I_CI = 1, MG_LATENT_1X1_I_CO = 2, MG_LATENT_1X1_I_HW = 3 };
enum mg_latent_1x1_f { MG_LATENT_1X1_F_SCALE = 0 };   /* input scale (0 = 1) */
enum mg_latent_1x1_p {
  MG_LATENT_1X1_P_X = 0,          /* f32 [B][Ci][HW] */
  MG_LATENT_1X1_P_W = 1,          /* f32 [Co][Ci] */
  MG_LATENT_1X1_P_BIAS = 2,       /* f32 [Co] */
  MG_LATENT_1X1_P_OUT = 3         /* f32 [B][Co][HW] */
};

enum mg_post_nchw_i {
  MG_POST_NCHW_I_B = 0,
  MG_POST_NCHW_I_HW = 1,
  MG_POST_NCHW_I_COUT = 2,        /* 1 | 3 | 4 | 8 | 12 */
  MG_POST_NCHW_I_LDI = 3,         /* row stride of the input */
  MG_POST_NCHW_I_POST = 4         /* MG_POST_* */
};
enum mg_post_nchw_f {
  MG_POST_NCHW_F_SCALE = 0,       /* scale on the input (0 = 1) */
  MG_POST_NCHW_F_CX = 1,          /* MG_POST_SCHED: coefficient of out (the latent x_t), */
  MG_POST_NCHW_F_CM = 2,          /* of the input (the model's output), */
  MG_POST_NCHW_F_CN = 3           /* of the noise */
};
enum mg_post_nchw_p {
  MG_POST_NCHW_P_X = 0,           /* f32 [B*HW][ldi] */
  MG_POST_NCHW_P_OUT = 1,         /* f32 NCHW */
  MG_POST_NCHW_P_NOISE = 2        /* f32 NCHW | NULL (MG_POST_SCHED) */
};

enum mg_im2col_small_i {
  MG_IM2COL_SMALL_I_B = 0,
  MG_IM2COL_SMALL_I_H = 1,
  MG_IM2COL_SMALL_I_W = 2,
  MG_IM2COL_SMALL_I_C0 = 3,
  MG_IM2COL_SMALL_I_C1 = 4,
  MG_IM2COL_SMALL_I_KP = 5,               /* columns of out (>= 9 (C0 + C1)) */
  MG_IM2COL_SMALL_I_SRC0_BROADCAST = 6,   /* 1 = src0 row 0 for every b, 0 = row b */
  MG_IM2COL_SMALL_I_MEMBERS_PER_SRC0 = 7  /* 0 = src0_broadcast decides; m > 0 = row b reads src0 row b / m (several images in one program,
                                             m ensemble members each; requires src0_broadcast = 0 and B % m == 0) */
};
enum mg_im2col_small_p {
  MG_IM2COL_SMALL_P_SRC0 = 0,     /* f32 [B | 1 | B / members_per_src0][C0][H][W] */
  MG_IM2COL_SMALL_P_SRC1 = 1,     /* f32 [B][C1][H][W] | NULL */
  MG_IM2COL_SMALL_P_OUT = 2       /* bf16 [B*H*W][Kp] */
};

enum mg_conv3x3_head_i {
  MG_CONV3X3_HEAD_I_B = 0,
  MG_CONV3X3_HEAD_I_H = 1,
  MG_CONV3X3_HEAD_I_W = 2,
  MG_CONV3X3_HEAD_I_C = 3,        /* % 32 == 0 */
  MG_CONV3X3_HEAD_I_COUT = 4,     /* 1..4 */
  MG_CONV3X3_HEAD_I_LDO = 5,      /* row stride of out (0 = Cout) */
  MG_CONV3X3_HEAD_I_SILU = 6
};
enum mg_conv3x3_head_p {
  MG_CONV3X3_HEAD_P_X = 0,        /* bf16 [B][H][W][C] */
  MG_CONV3X3_HEAD_P_SS = 1,       /* scale_shift f32 [B][2][C] | NULL */
  MG_CONV3X3_HEAD_P_WT = 2,       /* bf16 [>= Cout][9 C], k = (ky*3+kx)*C + c */
  MG_CONV3X3_HEAD_P_BIAS = 3,     /* f32 | NULL */
  MG_CONV3X3_HEAD_P_OUT = 4       /* f32 [B H W][ldo] (columns [0, Cout): what MG_OP_POST_NCHW reads) */
};

enum mg_ens_depth_stats_i { MG_ENS_DEPTH_STATS_I_E = 0 };
enum mg_ens_depth_stats_p {
  MG_ENS_DEPTH_STATS_P_D = 0,         /* f32 [E][HW] */
  MG_ENS_DEPTH_STATS_P_SCRATCH = 1,   /* f64 per-block partials (size: see the op) */
  MG_ENS_DEPTH_STATS_P_OUT = 2        /* f64 [3E + E*E] */
};
enum mg_ens_depth_stats_l { MG_ENS_DEPTH_STATS_L_HW = 0 };
enum mg_ens_depth_median_i {
  MG_ENS_DEPTH_MEDIAN_I_E = 0,
  MG_ENS_DEPTH_MEDIAN_I_REDUCTION = 1,  /* 0 median, 1 mean */
  MG_ENS_DEPTH_MEDIAN_I_HAS_SHIFT = 2
};
enum mg_ens_depth_median_p {
  MG_ENS_DEPTH_MEDIAN_P_D = 0,        /* f32 [E][HW] */
  MG_ENS_DEPTH_MEDIAN_P_ST = 1,       /* f32 [s[E], t[E]] | NULL (no alignment) */
  MG_ENS_DEPTH_MEDIAN_P_MED = 2,      /* f32 [HW] | NULL */
  MG_ENS_DEPTH_MEDIAN_P_MAD = 3,      /* f32 [HW] | NULL */
  MG_ENS_DEPTH_MEDIAN_P_MINMAX = 4,   /* f32 [2 + 2E] = min, max of the prediction and the raw member values d[.][argmin px], d[.][argmax px]
                                         (exact sub-gradient of the regulariser on the host) */
  MG_ENS_DEPTH_MEDIAN_P_SCRATCH = 5   /* >= 12288 B */
};
enum mg_ens_depth_median_l { MG_ENS_DEPTH_MEDIAN_L_HW = 0 };
enum mg_ens_depth_norm_i { MG_ENS_DEPTH_NORM_I_SHIFT_INVARIANT = 0 };
enum mg_ens_depth_norm_p {
  MG_ENS_DEPTH_NORM_P_MED = 0,        /* f32 [HW] */
  MG_ENS_DEPTH_NORM_P_MAD = 1,        /* f32 [HW] | NULL */
  MG_ENS_DEPTH_NORM_P_MINMAX = 2      /* MG_ENS_DEPTH_MEDIAN_P_MINMAX */
};
enum mg_ens_depth_norm_l { MG_ENS_DEPTH_NORM_L_HW = 0 };
enum mg_ens_normals_i {
  MG_ENS_NORMALS_I_E = 0,
  MG_ENS_NORMALS_I_REDUCTION = 1      /* 0 closest, 1 mean */
};
enum mg_ens_normals_p {
  MG_ENS_NORMALS_P_NORMALS = 0,       /* f32 [E][3][HW] */
  MG_ENS_NORMALS_P_OUT = 1,           /* f32 [3][HW] */
  MG_ENS_NORMALS_P_UNC = 2            /* f32 [HW] | NULL */
};
enum mg_ens_normals_l { MG_ENS_NORMALS_L_HW = 0 };

enum mg_resize_i {
  MG_RESIZE_I_PLANES = 0,         /* = B * C */
  MG_RESIZE_I_HIN = 1,
  MG_RESIZE_I_WIN = 2,
  MG_RESIZE_I_HOUT = 3,
  MG_RESIZE_I_WOUT = 4,
  MG_RESIZE_I_MODE = 5,           /* 0 bilinear, 1 bicubic, 2 nearest-exact */
  MG_RESIZE_I_U8 = 6              /* 1: uint8 in / out - computed in float, rounded half-to-even; 0: fp32 */
};
enum mg_resize_p {
  MG_RESIZE_P_SRC = 0,
  MG_RESIZE_P_DST = 1,
  MG_RESIZE_P_TMP = 2             /* f32 [planes][Hin][Wout] | NULL (needed when both sizes change) */
};

enum mg_colorize_f { MG_COLORIZE_F_MIN_DEPTH = 0, MG_COLORIZE_F_MAX_DEPTH = 1 };
enum mg_colorize_p {
  MG_COLORIZE_P_DEPTH = 0,        /* f32 [n] */
  MG_COLORIZE_P_LUT = 1,          /* uint8 [256][3] (matplotlib's table); required with P_OUT */
  MG_COLORIZE_P_OUT = 2,          /* uint8 [n][3] (HWC) | NULL when P_CLIPPED or P_U16 is given */
  MG_COLORIZE_P_CLIPPED = 3,      /* f32 [n] | NULL: clip(depth, 0, 1), NaN kept; may alias P_DEPTH (range (0, 1) only) */
  MG_COLORIZE_P_U16 = 4           /* uint16 [n] | NULL: uint16(clip(depth, 0, 1) * 65535), NaN -> 0 (range (0, 1) only) */
};
enum mg_colorize_l { MG_COLORIZE_L_N = 0 };

enum mg_eval_depth_ls_i {
  MG_EVAL_DEPTH_LS_I_H = 0,
  MG_EVAL_DEPTH_LS_I_W = 1,
  MG_EVAL_DEPTH_LS_I_DISPARITY = 2,   /* 1 = y = 1 / gt, valid &= gt > 0 & pred > 0 (script/depth/eval.py:185-201) */
  MG_EVAL_DEPTH_LS_I_FIT_W = 3        /* width of the sub-sampled fit (alignment_max_res: floor(W * factor), only the width shrinks; 0 = every pixel) */
};
enum mg_eval_depth_ls_f { MG_EVAL_DEPTH_LS_F_INV_FACTOR = 0 };   /* fp32(1 / factor): source column = min(floor(dst * inv_factor), W - 1) */
enum mg_eval_depth_ls_p {
  MG_EVAL_DEPTH_LS_P_PRED = 0,        /* f32 [H][W] */
  MG_EVAL_DEPTH_LS_P_GT = 1,          /* f32 [H][W] */
  MG_EVAL_DEPTH_LS_P_MASK = 2,        /* uint8 [H][W] (non-zero = valid) */
  MG_EVAL_DEPTH_LS_P_OUT = 3,         /* f64 [5] */
  MG_EVAL_DEPTH_LS_P_SCRATCH = 4      /* f64 [512][5] */
};
enum mg_eval_depth_metrics_i {
  MG_EVAL_DEPTH_METRICS_I_H = 0,
  MG_EVAL_DEPTH_METRICS_I_W = 1,
  MG_EVAL_DEPTH_METRICS_I_DISPARITY = 2,
  MG_EVAL_DEPTH_METRICS_I_CLIP_MIN = 3,   /* 1 = clip below at F_MIN_DEPTH */
  MG_EVAL_DEPTH_METRICS_I_CLIP_MAX = 4    /* 1 = clip above at F_MAX_DEPTH */
};
enum mg_eval_depth_metrics_f { MG_EVAL_DEPTH_METRICS_F_MIN_DEPTH = 0, MG_EVAL_DEPTH_METRICS_F_MAX_DEPTH = 1 };
enum mg_eval_depth_metrics_p {
  MG_EVAL_DEPTH_METRICS_P_PRED = 0,
  MG_EVAL_DEPTH_METRICS_P_GT = 1,
  MG_EVAL_DEPTH_METRICS_P_MASK = 2,
  MG_EVAL_DEPTH_METRICS_P_SUMS = 3,       /* the five sums f64 [5] | NULL (s = 1, t = 0) */
  MG_EVAL_DEPTH_METRICS_P_OUT = 4,        /* f64 [13] = abs_relative_difference, squared_relative_difference, rmse_linear, rmse_log, log10,
                                             delta1_acc, delta2_acc, delta3_acc, i_rmse, silog_rmse, scale, shift, n */
  MG_EVAL_DEPTH_METRICS_P_SCRATCH = 5     /* f64 [512][11] */
};
enum mg_eval_normals_i { MG_EVAL_NORMALS_I_MASKED = 0 };   /* drop the pixels whose gt vector has zero norm */
enum mg_eval_normals_p {
  MG_EVAL_NORMALS_P_PRED = 0,         /* f32 [3][HW] */
  MG_EVAL_NORMALS_P_GT = 1,           /* f32 [3][HW] */
  MG_EVAL_NORMALS_P_OUT = 2,          /* f64 [9] = mean, median, percentages below 5 / 7.5 / 11.25 / 22.5 / 30 degrees, rmse, n (n = 0: NaN) */
  MG_EVAL_NORMALS_P_ERR = 3,          /* error map f32 [HW] | NULL (dropped pixels hold -1) */
  MG_EVAL_NORMALS_P_WS = 4            /* workspace (MG_EVAL_WS_BYTES, 8-byte aligned; owned by the launch) */
};
enum mg_eval_normals_l { MG_EVAL_NORMALS_L_HW = 0 };

enum mg_memset_i { MG_MEMSET_I_VALUE = 0 };   /* byte value */
enum mg_memset_p { MG_MEMSET_P_DST = 0 };
enum mg_memset_l { MG_MEMSET_L_BYTES = 0 };
enum mg_copy_p { MG_COPY_P_SRC = 0, MG_COPY_P_DST = 1 };
enum mg_copy_l { MG_COPY_L_BYTES = 0 };

enum mg_iidscore_prep_i {
  MG_IIDSCORE_PREP_I_H = 0,
  MG_IIDSCORE_PREP_I_W = 1,
  MG_IIDSCORE_PREP_I_GAMMA = 2        /* MG_IID_GAMMA_*: x <- x^gamma in fp32 on every load of both images */
};
enum mg_iidscore_prep_p {
  MG_IIDSCORE_PREP_P_PRED = 0,        /* f32 [3][H][W] */
  MG_IIDSCORE_PREP_P_GT = 1,          /* f32 [3][H][W] */
  MG_IIDSCORE_PREP_P_MASK = 2,        /* uint8 [3][H][W] (non-zero = valid) | NULL (every element valid) */
  MG_IIDSCORE_PREP_P_OUT = 3,         /* f64 [8], see the op */
  MG_IIDSCORE_PREP_P_WS = 4           /* workspace (MG_EVAL_WS_BYTES, 8-byte aligned) */
};
enum mg_iidscore_psnr_i {
  MG_IIDSCORE_PSNR_I_H = 0,
  MG_IIDSCORE_PSNR_I_W = 1,
  MG_IIDSCORE_PSNR_I_GAMMA = 2,
  MG_IIDSCORE_PSNR_I_UP_TO_SCALE = 3, /* 1 = an up-to-scale target: map both images on load with what PREP found */
  MG_IIDSCORE_PSNR_I_WRITE_PSNR = 4   /* 1 = write out[0] (0: only count the valid elements) */
};
enum mg_iidscore_psnr_p {
  MG_IIDSCORE_PSNR_P_PRED = 0,
  MG_IIDSCORE_PSNR_P_GT = 1,
  MG_IIDSCORE_PSNR_P_MASK = 2,
  MG_IIDSCORE_PSNR_P_OUT = 3,
  MG_IIDSCORE_PSNR_P_WS = 4
};
enum mg_iidscore_ssim_i {
  MG_IIDSCORE_SSIM_I_H = 0,
  MG_IIDSCORE_SSIM_I_W = 1,
  MG_IIDSCORE_SSIM_I_GAMMA = 2,
  MG_IIDSCORE_SSIM_I_UP_TO_SCALE = 3
};
enum mg_iidscore_ssim_p {
  MG_IIDSCORE_SSIM_P_PRED = 0,
  MG_IIDSCORE_SSIM_P_GT = 1,
  MG_IIDSCORE_SSIM_P_MASK = 2,
  MG_IIDSCORE_SSIM_P_OUT = 3,
  MG_IIDSCORE_SSIM_P_WS = 4
};

enum mg_iid_vis_i {
  MG_IID_VIS_I_N = 0,                 /* targets (<= 16) */
  MG_IID_VIS_I_H = 1,
  MG_IID_VIS_I_W = 2,
  MG_IID_VIS_I_LINEAR_BITS = 3,       /* bit t: target t is in linear space */
  MG_IID_VIS_I_UP_TO_SCALE_BITS = 4   /* bit t: target t is up to scale */
};
enum mg_iid_vis_p {
  MG_IID_VIS_P_PRED = 0,              /* f32 [n][3][H][W] */
  MG_IID_VIS_P_OUT = 1,               /* uint8 [n][H][W][3] (HWC) */
  MG_IID_VIS_P_WS = 2                 /* f32 [n][MG_IID_VIS_PARTS] (may be NULL when no target is both linear and up to scale) */
};

typedef struct mg_program mg_program;

/* Library / device */
int mg_abi_version(void);
/* The 16-bit operand type every "bf16" buffer of this build holds: 0 = bf16 (libmarigold_hip.so), 1 = IEEE fp16 (libmarigold_hip_f16.so,
 * the same sources built with OPERAND_F16=1 - the reference's `--fp16` arithmetic, script/depth/run.py:203-211).  Same ABI, same ops. */
int mg_operand_bits(void);
const char* mg_last_error(void);
int mg_init(int device);                 /* idempotent; allocates the zero page */
/* GEGLU weight-row interleave the host must pack ff.net.0.proj with (32: 16 u rows, then their 16 gate rows). */
int mg_geglu_interleave(void);
int mg_device_info(int* cu_count, int* lds_bytes, int64_t* hbm_bytes, char* arch, int arch_len);

/* One launch (also the body of mg_program_run) */
int mg_launch(const mg_op* op, void* stream);

/* Programs: replace the per-step Python loop of single_infer
 * (marigold_depth_pipeline.py:455-468) and the module forwards it calls. */
mg_program* mg_program_create(const mg_op* ops, int n_ops);
int mg_program_num_ops(const mg_program* prog);
int mg_program_run(mg_program* prog, void* stream);
/* Check every op of the program against its kernel's shape / alignment contract WITHOUT touching
 * the device (no GPU needed): 0 = launchable, else the first violation in mg_last_error(). */
int mg_program_validate(mg_program* prog);
int mg_program_run_range(mg_program* prog, int first, int count, void* stream);
/* Capture the program into a hipGraph on `stream` and replay that on later runs. */
int mg_program_capture(mg_program* prog, void* stream);
/* Time every op with HIP events on `stream` (ms per op written to `ms`, length n_ops). */
int mg_program_profile(mg_program* prog, void* stream, float* ms);
void mg_program_destroy(mg_program* prog);

/* Module-level entry points over a MODEL IMAGE: the pipeline's three native programs for one problem shape (image size,
 * members per call, scheduler steps), their kernel-ready weights and a memory plan, written once by
 * marigold_amd/image.py::export_model_image and run from any host language without Python.  They stand where single_infer's
 * calls stand (marigold/marigold_depth_pipeline.py:396-477): encode_rgb (:479-496), the T-step unet + scheduler.step loop
 * (:455-468), decode_depth / decode_normals (:498-516, :473-475).  All device pointers are the caller's (fp32, NCHW, contiguous);
 * the model owns its weights and workspace (mg_model_device_bytes: the handle's private memory; weights that several handles
 * share are counted by mg_model_shared_bytes, below).  One stream at a time per model.
 *  mg_model_load(path, device): device >= 0 binds the library to that GPU (mg_init) and uploads; device < 0 = host-only: the
 *  image is parsed and relocated against fake addresses so that mg_model_validate can check every op's contract without a GPU.
 *  mg_model_info: cfg16 = the MG_CFG_WORDS configuration words, named by enum mg_cfg below.  cfg16[13] = K, the pictures per call the
 *  image was exported for (export_model_image(images_per_program=K)), is MG_CFG_PICTURES: 0 in an image of one picture per call -
 *  every image written before the field existed, and every K = 1 export since - else the written value, K > 1 (read it with
 *  MG_CFG_PICTURES_OF); B = cfg16[MG_CFG_MEMBERS] is then the members of EACH picture.
 *  mg_model_vae_encode: rgb [1,3,H,W] in [-1,1] -> latent [1,4,h,w] (x 0.18215, posterior mean).
 *  mg_model_denoise: rgb_latent [1,4,h,w], x [B,C,h,w] in / out (the initial noise -> the denoised latent), step_noise
 *  [n][B,C,h,w] for the LCM scheduler's n noisy steps (NULL for DDIM).
 *  mg_model_vae_decode: latent [B*modalities,4,h,w] -> pred [B, channels, Hout, Wout] with the pipeline's pointwise tail.
 *  On an image of K > 1 pictures per call the three calls copy by slot size as before and carry the batch: rgb [K,3,H,W], rgb_latent
 *  [K,4,h,w]; x, latent and pred have K B rows, image-major (row i B + j = member j of picture i), step_noise [n][K B,C,h,w].
 *  mg_model_load checks that the slots of the three programs chain for K pictures of B members before anything can run. */
typedef struct mg_model mg_model;
/* The configuration words of mg_model_info / mg_model_config_info (and of the image file): position = word. */
enum mg_cfg {
  MG_CFG_MEMBERS = 0,       /* B: the ensemble members of each picture */
  MG_CFG_HEIGHT = 1,        /* H x W: the size fed to the VAE */
  MG_CFG_WIDTH = 2,
  MG_CFG_LATENT_H = 3,      /* h x w */
  MG_CFG_LATENT_W = 4,
  MG_CFG_STEPS = 5,         /* scheduler steps */
  MG_CFG_CHANNELS = 6,      /* prediction channels */
  MG_CFG_POST = 7,          /* MG_POST_*: the decoder's pointwise tail */
  MG_CFG_STEP_NOISES = 8,   /* step-noise tensors (the LCM scheduler's) */
  MG_CFG_OP_BYTES = 9,      /* sizeof(mg_op) */
  MG_CFG_MODALITIES = 10,   /* 1; an intrinsic-image model: its targets */
  MG_CFG_OUT_H = 11,        /* the decoded size */
  MG_CFG_OUT_W = 12,
  MG_CFG_PICTURES = 13,     /* K, written 0 for 1: read it with MG_CFG_PICTURES_OF */
  MG_CFG_VAE = 14,          /* MG_VAE_* */
  MG_CFG_WORDS = 16         /* (word 15 is reserved, written 0) */
};
enum { MG_VAE_KL = 0, MG_VAE_TINY = 1 };
#define MG_CFG_PICTURES_OF(cfg) ((cfg)[MG_CFG_PICTURES] ? (cfg)[MG_CFG_PICTURES] : 1)
mg_model* mg_model_load(const char* path, int device);
void mg_model_destroy(mg_model* m);
int mg_model_info(const mg_model* m, int* cfg16);
long long mg_model_device_bytes(const mg_model* m);
int mg_model_validate(mg_model* m);
int mg_model_vae_encode(mg_model* m, const float* rgb, float* latent, void* stream);
int mg_model_denoise(mg_model* m, const float* rgb_latent, float* x, const float* step_noise, void* stream);
int mg_model_vae_decode(mg_model* m, const float* latent, float* pred, void* stream);

/* One image, several CONFIGURATIONS (export_model_image(configs=[...]), a version-2 file): a configuration is what a version-1
 * image is - (members, height, width, steps, pictures per call) and its three programs.  The kernel-ready weights are stored and
 * uploaded once, the SHARED allocation; a handle's private memory (mg_model_device_bytes) holds every configuration's constants and
 * zeroed state and ONE scratch region sized to the largest configuration's scratch, which the configurations overlay: they never
 * run at the same time on one handle and no program reads scratch it has not written.  A version-1 image loads as one
 * configuration with nothing shared.
 *  mg_model_num_configs / mg_model_config_info: the count; the 16 words of mg_model_info for configuration `index`.
 *  mg_model_find_config: the first configuration of that processed size H x W, E members, steps and K pictures per call (K = 1: a
 *  one-picture configuration); -1 in a field = any value.  No match: -1, and mg_last_error lists the sizes the image holds.
 *  mg_model_select: the SELECTED configuration is what mg_model_info, mg_model_validate, mg_model_vae_encode / _denoise /
 *  _vae_decode and every mg_model_predict* act on - with their refusals, in their words (a K > 1 configuration refuses the
 *  one-picture calls).  Configuration 0 is selected after the load; selecting launches nothing and costs nothing.  Not while a call
 *  on this handle is being issued from another thread.
 *  mg_processed_size: the size the pipelines feed the VAE for a picture of Hin x Win at processing_res (util/image_util.py::
 *  resize_max_res: the longer edge becomes processing_res, the other is truncated; the arithmetic is the reference's, in doubles);
 *  processing_res = 0 leaves the size as it is.  With it a host picks the configuration for a picture itself:
 *  mg_processed_size -> mg_model_find_config -> mg_model_select -> mg_model_predict_out.
 *  mg_model_shared_bytes: the bytes of the shared weights (0 for a version-1 image), counted once however many handles read them;
 *  mg_model_device_bytes counts the handle's PRIVATE memory only: its arena and its temporaries.
 *  mg_model_replica: a second handle over the SAME shared weights with a private arena of its own (constants copied device to
 *  device from `m`, zeroed state zeroed, scratch as allocated), its own programs and temporaries: what a host needs to keep a second
 *  picture in flight.  Each handle may be driven from its own host thread on its own stream.  The replica starts on the
 *  configuration `m` has selected.  Call it while `m` is idle.  Parent and replica are destroyed in either order (mg_model_destroy);
 *  the shared weights are freed with the last handle.  A host-only model replicates too.  NULL on failure (mg_last_error). */
int mg_model_num_configs(const mg_model* m);
int mg_model_config_info(const mg_model* m, int index, int* cfg16);
int mg_model_find_config(const mg_model* m, int H, int W, int E, int steps, int K);
int mg_model_select(mg_model* m, int index);
int mg_processed_size(int Hin, int Win, int processing_res, int* H, int* W);
long long mg_model_shared_bytes(const mg_model* m);
mg_model* mg_model_replica(const mg_model* m);

/* Model images with the TINY autoencoder (export_model_image(tiny_vae=True), a version-3 file in the version-2 layout, for one
 * configuration or several): cfg[MG_CFG_VAE] names the image's VAE - MG_VAE_KL an AutoencoderKL (every version-1 and version-2 image), MG_VAE_TINY the tiny
 * autoencoder - and one image has one.  Where an AutoencoderKL image runs its encode and decode programs, a tiny image calls
 * mg_tiny_vae_encode (the K pictures of a call) and mg_tiny_vae_decode (all K B members, times the modalities, in ONE call; a member's
 * result does not depend on the batch) on the same named slots, on the caller's stream, with the tail cfg[MG_CFG_POST], without
 * synchronising: in mg_model_vae_encode / mg_model_vae_decode and in every mg_model_predict*.  Nothing else differs, and a host written
 * for AutoencoderKL images runs a tiny one unchanged, provided it sizes its buffers from cfg16 as documented: the latent size
 * cfg[MG_CFG_LATENT_H] x cfg[MG_CFG_LATENT_W] is the tiny encoder's, a CEILING per stride-2 layer (30 x 44 -> 4 x 6) where the AutoencoderKL floors (3 x 5),
 * and the decoded size cfg[MG_CFG_OUT_H] x cfg[MG_CFG_OUT_W] is 8 x that (32 x 48), which may exceed the picture.  In the file the two VAE entries of a
 * configuration hold no ops, only their slots (rgb, latent | latent, pred) and a workspace slot (ws) of at least
 * mg_tiny_vae_workspace_bytes - scratch of that configuration, in the region the configurations overlay; the members of struct
 * mg_tiny_vae lie in the shared weights (mg_model_shared_bytes; replicas read the same ones), recorded as (buffer, byte offset), the six
 * bias-free layers as absent.  mg_model_load checks all of that - every member inside its buffer with the bytes its layout implies and
 * 16-byte aligned, NULL members exactly where the layout has them, the slot sizes chained under the ceiling rule, the workspaces - and
 * mg_model_validate runs the two calls' own argument checks without a device.  A library built before version 3 refuses such a file
 * as an unknown version.
 *  mg_model_scratch_fill: a test hook - every scratch buffer of the handle (all configurations') is set to `byte` on `stream`, so that
 *  a test can show that no result depends on what scratch held before a call (0xff: NaN in every float format).  Does not
 *  synchronise; refuses a host-only model. */
int mg_model_scratch_fill(mg_model* m, int byte, void* stream);

/* The whole prediction of one picture as ONE call, from the uint8 bytes and a seed to the ensembled map - __call__ of the reference's
 * pipelines (marigold/marigold_depth_pipeline.py:154-338, marigold_normals_pipeline.py:139-308) up to match_input_res, for a host
 * that has neither torch nor a noise file.  All pointers are device pointers.  The chain: mg_rgb_prepare to the model's H x W (rgb
 * uint8 [Hin][Win][3] with hwc != 0, else [3][Hin][Win]; mode and reciprocal as in mg_rgb_prepare) -> encode -> MG_OP_RANDN of
 * stream 0 as the initial latents [B,C,h,w] -> denoise (an LCM image: step noise k = stream k + 1, cfg[MG_CFG_STEP_NOISES] of them) -> decode ->
 * ensemble: depth by mg_ensemble_depth, normals by MG_OP_ENS_NORMALS, a single member (B == 1) is copied.  pred_out fp32 [channels]
 * [cfg[MG_CFG_OUT_H]][cfg[MG_CFG_OUT_W]] (the decoded size); unc_out fp32 [cfg[MG_CFG_OUT_H]][cfg[MG_CFG_OUT_W]] | NULL, written when B > 1 (the pipelines return none for
 * one member); info4 | NULL as in mg_ensemble_depth (zeros where no alignment ran).  opts NULL = the reference's defaults
 * (ensemble.py:39-49, :199-203), which MG_PREDICT_OPTS_DEFAULT spells out.  An intrinsic-image model is refused (its entry point is
 * mg_model_predict_iid, below).  The resampling
 * temporary is the model's: allocated at the first call that needs it, counted by mg_model_device_bytes, freed by mg_model_destroy.
 * Synchronises the stream where mg_ensemble_depth does (depth, B > 1) and nowhere else.  The Python pipelines give the same map, bit
 * for bit, from the same bytes with generator=marigold_amd.NativeNoise(seed) and match_input_res=False. */
typedef struct mg_predict_opts {
  int scale_invariant, shift_invariant;   /* depth: the alignment (the pipeline's constructor arguments) */
  int reduction;                          /* depth: 0 median / 1 mean */
  int max_iter, max_res;                  /* depth: BFGS iterations; the alignment runs on members down-sampled to max_res (<= 0: never) */
  int normals_reduction;                  /* normals: 0 closest / 1 mean */
  double regularizer_strength, tol;       /* depth */
} mg_predict_opts;
#define MG_PREDICT_OPTS_DEFAULT {1, 1, 0, 50, 1024, 0, 0.02, 1e-6}
int mg_model_predict(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                     const mg_predict_opts* opts_or_null, float* pred_out, float* unc_out_or_null, double* info4_or_null, void* stream);

/* mg_model_predict carried on through match_input_res to what the pipelines return (marigold/marigold_depth_pipeline.py:306-329,
 * marigold_normals_pipeline.py:282-301) and what script/depth/run.py writes: the map at the size asked for, clipped, the 16-bit depth
 * and the picture.  Arguments up to opts are mg_model_predict's; the chain up to the ensemble is the same, call for call.  Then:
 * with out_opts.out_h x out_w set and different from the decoded size cfg[MG_CFG_OUT_H] x cfg[MG_CFG_OUT_W] the ensembled prediction - not the
 * uncertainty - is resampled to them (MG_OP_RESIZE in mode out_opts.out_mode); then one launch of the output stage on what was
 * stored to pred_out, clipping it in place: depth - MG_OP_COLORIZE with P_CLIPPED = P_DEPTH (clip to [0, 1], the 16-bit values, the
 * colour picture from out_opts.lut256x3, a DEVICE pointer to the colour map's 256 x 3 uint8 table); normals - mg_normals_finish (clip
 * to [-1, 1], the picture).
 *  pred_out    fp32 [channels][out_h][out_w] (the decoded size when out_h = out_w = 0), clipped
 *  unc_out     fp32 [cfg[MG_CFG_OUT_H]][cfg[MG_CFG_OUT_W]] | NULL, written when B > 1
 *  u16_out     uint16 [out_h][out_w] | NULL = uint16(pred_out * 65535), a depth model only
 *  picture_out uint8 [out_h][out_w][3] | NULL; a depth model needs out_opts.lut256x3 for it
 *  info4       as in mg_model_predict
 * out_opts NULL = MG_OUTPUT_OPTS_DEFAULT: the decoded size, no table.  Refused: a host-only model, an intrinsic-image model (its entry
 * point is mg_model_predict_iid), a bad out_mode or size, picture_out of a depth model without a table, u16_out or a table with a
 * normals model.  The temporaries (the ensembled map ahead of a resize, the resize's fp32 intermediate) are the model's: grown on
 * demand, counted by mg_model_device_bytes, freed by mg_model_destroy.  Synchronises where mg_ensemble_depth does and nowhere else.
 * The Python pipelines give the same arrays and pictures, bit for bit, with generator=marigold_amd.NativeNoise(seed) and
 * match_input_res=True (tests/test_gpu_predict_out_c_host.py; examples/host_picture.cpp).  No speed is claimed: the stage is
 * microseconds beside a map. */
typedef struct mg_output_opts {
  int out_h, out_w;          /* match_input_res: size of pred_out, u16_out and picture_out; 0, 0 = the model's output size */
  int out_mode;              /* resample mode of that resize, the numbering of MG_OP_RESIZE */
  const uint8_t* lut256x3;   /* depth: the colour map's table on the device (marigold_amd.image.export_color_table writes its bytes) | NULL */
} mg_output_opts;
#define MG_OUTPUT_OPTS_DEFAULT {0, 0, 0, 0}
int mg_model_predict_out(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                         const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out,
                         float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null,
                         void* stream);

/* mg_model_predict_out for n pictures in ONE call, on an image exported for K >= n pictures per call (cfg[MG_CFG_PICTURES]): the pictures share
 * one encode, one denoise and one decode program - the programs map_images(images_per_program=K) runs - and every stage before and
 * after them runs per picture, the very code of mg_model_predict_out (one picture is its n = K = 1 case).
 *  rgb         a HOST array of n DEVICE pointers, every picture uint8 Hin x Win in the layout `hwc` names
 *  seeds       a HOST array of n seeds: picture i draws what its lone call draws from seeds[i] (MG_OP_RANDN stream 0 = its B initial
 *              latents, stream k + 1 = its LCM step noise k), into rows [i B, (i + 1) B) of the denoise program
 *  pred_out    fp32 [n][channels][out_h][out_w], clipped     unc_out  fp32 [n][cfg[MG_CFG_OUT_H]][cfg[MG_CFG_OUT_W]] | NULL, written when B > 1
 *  u16_out     uint16 [n][out_h][out_w] | NULL               picture_out uint8 [n][out_h][out_w][3] | NULL
 *  info4       double [n][4] | NULL, per picture as in mg_model_predict
 * opts and out_opts apply to every picture, with the defaults of mg_model_predict_out.  A call with n < K feeds picture n - 1 and its
 * seed to the spare rows as well (no row ever reads what an earlier call left there), discards their results and writes nothing
 * beyond row n - 1 of any output.  Refused before anything is launched, the message starting with "mg_model_predict_many:": n < 1
 * or n > K, a null rgb or seeds array or a null picture, a host-only model, an intrinsic-image model (exported for one picture per
 * call only), and every output-option refusal of mg_model_predict_out in the same words.  On an image of K > 1 pictures per call
 * mg_model_predict, mg_model_predict_out and mg_model_predict_iid refuse and name mg_model_predict_many.  The temporaries (input
 * resampling for one picture, the ensembled map ahead of a resize, the resize's intermediate) are the model's and serve the pictures
 * in turn: grown on demand, counted by mg_model_device_bytes.  Synchronises where mg_ensemble_depth does - once per picture for
 * depth with B > 1 - and nowhere else.  map_images(images_per_program=K, generators=[NativeNoise(seed_i)], match_input_res=True)
 * gives the same arrays and pictures, bit for bit (tests/test_gpu_predict_many_c_host.py; examples/host_many.cpp). */
int mg_model_predict_many(mg_model* m, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                          const uint64_t* seeds, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                          float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                          double* info4_or_null, void* stream);

/* Image SEQUENCES: mg_model_predict_out with the recipe of frame-by-frame video processing - frame k starts from
 * (1 - strength) noise + strength latent, where latent is the denoised latent of frame k - 1 on this handle.  The handle keeps ONE
 * carried buffer, the bytes of the denoise program's x slot, allocated at the first mg_model_predict_next and counted by
 * mg_model_device_bytes.  mg_model_predict_next is mg_model_predict_out, argument for argument, with two additions to its chain: after
 * MG_OP_RANDN of stream 0, if a latent is carried, mg_latent_carry blends it into the x slot; after the denoise program the x slot is
 * copied, device to device, into the carried buffer.  The noise is drawn as mg_model_predict_out draws it (the LCM step noises too).
 * The first call after mg_model_load, mg_model_replica, mg_model_seq_reset or mg_model_select carries nothing and returns the bits of
 * mg_model_predict_out; a replica has a state of its own, empty at first.  mg_model_predict_out itself neither reads nor changes the
 * state.  Refused before anything is launched, with mg_model_predict_out's refusals: a strength outside [0, 1] (or NaN), a
 * configuration of K > 1 pictures per call, an intrinsic-image model.  Synchronises where mg_model_predict_out does.  The Python
 * pipelines give the same arrays and pictures, bit for bit, with map_video(frames, strength, generators=[NativeNoise(seed_k)],
 * match_input_res=True) (tests/test_gpu_sequence.py; examples/host_sequence.cpp).
 *  mg_model_seq_reset: forget the carried latent (the buffer stays allocated); the next mg_model_predict_next starts a sequence.
 *  mg_latent_carry: the blend itself, in place on device pointers: x[i] = fl(fl(a x[i]) + fl(b prev[i])) with b = strength and
 *  a = (float)(1.0 - (double)strength) - three fp32 roundings, no fused multiply-add: the bits of torch's (x * a) + (prev * b).
 *  NaN and infinities propagate as IEEE 754 has them.  Four elements per lane when both pointers are 16-byte aligned, one otherwise;
 *  nothing at or beyond x + n is written.  n == 0 is a no-op; n < 0, a null pointer with n > 0, and a strength outside [0, 1] or NaN
 *  are refused before any GPU work.  Does not synchronise. */
int mg_latent_carry(float* x, const float* prev, int64_t n, float strength, void* stream);
int mg_model_seq_reset(mg_model* m);
int mg_model_predict_next(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                          const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out,
                          float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null,
                          void* stream, float strength);

/* The same for an intrinsic-image model (appearance, lighting): __call__ of the reference's MarigoldIIDPipeline with fill_outputs
 * (marigold/marigold_iid_pipeline.py:239-411) as ONE call.  It takes an intrinsic-image model only (MG_POST_UNIT, cfg[MG_CFG_MODALITIES] = n_targets
 * >= 1, 3 n_targets prediction channels, a DDIM image: the pipeline refuses the LCM scheduler and so does this call); a depth or
 * normals model is refused.  The chain up to the decoder is that of mg_model_predict, argument for argument; the denoised latent
 * [B, 4 n_targets, h, w] is the decoder's batch [B n_targets, 4, h, w] as it lies.  Then: B > 1 - one MG_OP_ENS_IID over the members,
 * straight out of the decoder's output (opts.reduction; unc_out, when given, receives the uncertainty); B == 1 - a copy, unc_out is
 * not written (the pipeline returns none).  With opts.out_h, out_w set and different from the decoded size cfg[MG_CFG_OUT_H] x cfg[MG_CFG_OUT_W] the
 * ensembled prediction is resampled to them (the pipeline's match_input_res: MG_OP_RESIZE in mode opts.out_mode; the uncertainty
 * is not resampled, reference :378-385).  With pictures_out the targets' pictures are made of what was stored to pred_out
 * (MG_OP_IID_VIS; bit t of linear_bits / up_to_scale_bits describes target t).
 *  pred_out fp32 [3 n_targets][out_h][out_w] (the decoded size when out_h = out_w = 0)
 *  unc_out  fp32 [3 n_targets][cfg[MG_CFG_OUT_H]][cfg[MG_CFG_OUT_W]] | NULL
 *  pictures_out uint8 [n_targets][out_h][out_w][3] | NULL
 * opts NULL = MG_IID_OPTS_DEFAULT: the median, every target in sRGB space, no resampling.  The temporaries (input resampling,
 * the prediction before its resampling with that pass's intermediate, the picture stage's workspace) are the model's: allocated at the
 * first call that needs them, grown when a later call needs more, counted by mg_model_device_bytes, freed by mg_model_destroy.
 * Synchronises nowhere.  The Python pipeline gives the same arrays, uncertainties and pictures, bit for bit, from the same bytes with
 * generator=marigold_amd.NativeNoise(seed) (tests/test_gpu_iid_c_host.py; examples/host_iid.cpp). */
typedef struct mg_iid_opts {
  int reduction;          /* 0 median / 1 mean */
  int linear_bits;        /* bit t: target t is predicted in linear space      (target_properties[name].prediction_space == "linear") */
  int up_to_scale_bits;   /* bit t: target t is linear and up to scale         (...["up_to_scale"])                                    */
  int out_h, out_w;       /* match_input_res: size of pred_out and pictures; 0, 0 = the model's output size */
  int out_mode;           /* resample mode of that resize, the numbering of MG_OP_RESIZE */
} mg_iid_opts;
#define MG_IID_OPTS_DEFAULT {0, 0, 0, 0, 0, 0}
int mg_model_predict_iid(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                         const mg_iid_opts* opts_or_null, float* pred_out, float* unc_out_or_null, uint8_t* pictures_out_or_null,
                         void* stream);

/* ensemble_depth(depth[E,1,H,W], scale_invariant, shift_invariant, output_uncertainty, reduction, regularizer_strength, max_iter,
 * tol, max_res) of marigold/util/ensemble.py:39-196 as ONE call on device pointers: member statistics, init_param, the native
 * scipy-BFGS alignment (mg_ens_align_minimize), align -> median (+ MAD) | mean (+ std) -> min / max normalisation.  preds fp32
 * [E][H*W]; depth_out [H*W]; unc_out [H*W] | NULL; reduction 0 median / 1 mean; max_res <= 0 = no down-sampling for the alignment;
 * info4 (optional) = achieved cost, cost evaluations, BFGS iterations, scipy's status (0 converged, 1 maxiter, 2 precision loss,
 * 3 NaN -> the alignment falls back to its starting point).  Same results as marigold_amd.ensemble.ensemble_depth, bit for bit
 * (tests/test_gpu_pipeline.py).  The reference's ValueErrors come back as error messages with the reference's texts.
 * Synchronises the stream. */
int mg_ensemble_depth(const float* preds, int E, int H, int W, int scale_invariant, int shift_invariant, int reduction,
                      double regularizer_strength, int max_iter, double tol, int max_res, float* depth_out, float* unc_out,
                      double* info4, void* stream);

/* Named wrappers - what a binding for the reference's seams would call directly. */
int mg_conv2d_igemm(const mg_op* conv_desc, void* stream);   /* kind must be MG_OP_IGEMM */
/* Host-only test hook (no device work): how MG_OP_FLASH_ATTN64's hand-placed kernel would share out B x heads sequences of Ntok
 * tokens over a chip of n_cu CUs given a workspace of ws_bytes and the split mode (MG_FLASH64_I_SPLIT): out[0] whole blocks of 256 queries,
 * out[1] blocks split along the keys, out[2] workgroups over the split blocks; bounds[0 .. out[2]] (or NULL): the workgroups'
 * piece boundaries in 64-key tiles over the concatenated split blocks. */
int mg_flash4w_plan_test(int B, int heads, int Ntok, int n_cu, long long ws_bytes, int split, int* out, unsigned* bounds);
int mg_conv3x3(const mg_op* conv_desc, void* stream);        /* kind must be MG_OP_CONV3X3 (ResnetBlock2D norm+silu+conv) */
/* Slots per image of the partial table this MG_OP_CONV3X3 can fill with the GroupNorm statistics of its OUTPUT (MG_CONV3X3_P_GN_PART, see the
 * op), or 0 when the tile variant it runs on does not produce them (then leave it NULL and use MG_OP_GN_STATS). */
int mg_conv3x3_gn_slots(const mg_op* conv_desc);
int mg_sched_step(const float* x, const float* model_out, const float* noise, float* out,
                  int64_t n, float cx, float cm, float cn, void* stream);
int mg_ensemble_normals(const float* normals, float* out, float* unc, int E, int64_t hw,
                        int reduction, void* stream);
/* MG_OP_ENS_IID as a call: preds fp32 [E][n] -> pred_out [n] (+ unc_out [n]); reduction 0 median / 1 mean.  Does not synchronise. */
int mg_ensemble_iid(const float* preds, int E, int64_t n, int reduction, float* pred_out, float* unc_out_or_null, void* stream);

/* One-pass validation (src/trainer/marigold_depth_trainer.py:510-601; script/depth/eval.py:176-240, script/normals/eval.py): score one
 * prediction against its ground truth on the device, with no host round trip between the fit and the scores.  The caller reads the
 * results back when it needs them - none of these calls synchronises.  workspace: MG_EVAL_WS_BYTES of device memory, 8-byte aligned, owned
 * by the call until the stream has passed it (one workspace per stream).
 *  mg_eval_depth: pred, gt fp32 [H][W], mask uint8 [H][W]; alignment MG_EVAL_ALIGN_*; align_max_res <= 0 = fit on every pixel;
 *  min_depth / max_depth: the dataset's clip limits, NaN = none; out13 f64 = the ten scores in script/depth/eval.py's order, scale,
 *  shift, n (MG_OP_EVAL_DEPTH_LS + MG_OP_EVAL_DEPTH_METRICS).
 *  mg_eval_normals: pred, gt fp32 [3][HW]; masked = drop pixels whose gt vector has zero norm; out9 f64 and the optional error map
 *  as MG_OP_EVAL_NORMALS writes them. */
#define MG_EVAL_WS_BYTES (128 * 1024)
enum { MG_EVAL_ALIGN_NONE = 0, MG_EVAL_ALIGN_LS = 1, MG_EVAL_ALIGN_LS_DISPARITY = 2 };
int mg_eval_depth(const float* pred, const float* gt, const uint8_t* mask, int H, int W, int alignment, int align_max_res,
                  double min_depth, double max_depth, double* out13, void* workspace, void* stream);
int mg_eval_normals(const float* pred, const float* gt, int64_t HW, int masked, double* out9, float* err_map_or_null,
                    void* workspace, void* stream);
/*  mg_eval_iid: one target of one image, pred, gt fp32 [3][H][W] (H, W >= 11), mask uint8 [3][H][W] or NULL; up_to_scale != 0 for
 *  shading / residual (MG_OP_IIDSCORE_PREP first); gamma_mode MG_IID_GAMMA_*: the conversions script/iid/eval.py applies before it
 *  scores (2.2 for a target evaluated in linear space, 1 / 2.2 for Hypersim's albedo; BOTH = 2.2, then 1 / 2.2); metrics_mask
 *  MG_IID_PSNR | MG_IID_SSIM.  out8 f64 = psnr, ssim, alignment scale, quantile, brightness scale, valid elements, two reserved
 *  slots (do not read them); a slot nothing was asked to fill holds NaN; no valid element: all NaN and n = 0.  Same workspace
 *  rule; does not synchronise. */
enum { MG_IID_GAMMA_NONE = 0, MG_IID_GAMMA_2_2 = 1, MG_IID_GAMMA_INV_2_2 = 2, MG_IID_GAMMA_BOTH = 3 };
enum { MG_IID_PSNR = 1, MG_IID_SSIM = 2 };
int mg_eval_iid(const float* pred, const float* gt, const uint8_t* mask_or_null, int H, int W, int up_to_scale, int gamma_mode,
                int metrics_mask, double* out8, void* workspace, void* stream);
/*  mg_eval_iid_lpips: LPIPS (AlexNet features, fp32 throughout; csrc/lpips.hip, the definition: evaluation/metrics.py:lpips) of the
 *  same target as mg_eval_iid sees it - gamma, mask (invalid elements of both images -> 0) and, for an up-to-scale target, the (s, q)
 *  of MG_OP_IIDSCORE_PREP, which the call runs itself into eval_ws (PREP is bit-reproducible: they are mg_eval_iid's).  H, W >= 31.
 *  net: DEVICE pointers to fp32 weights in the layout the kernels read, layer l = 0..4 (Cin 3, 64, 192, 384, 256; Cout 64, 192, 384,
 *  256, 256; k 11, 5, 3, 3, 3):
 *    conv_w[l]  [k * k * Cin][Cout], row (ky * k + kx) * Cin + ci  (torch's [Cout][Cin][k][k] permuted to [k][k][Cin][Cout])
 *    conv_b[l]  [Cout]
 *    lin_w[l]   [Cout]  (the 1 x 1 "lin" layer of the tap, no bias)
 *  out8 f64 = LPIPS, the number of valid elements of either image outside [0, 1] (NaN counts; the caller refuses the score when it
 *  is not 0), the five per-tap terms, NaN.  eval_ws: MG_EVAL_WS_BYTES, 8-byte aligned; act_ws: mg_lpips_workspace_bytes(H, W) bytes
 *  (-1 with mg_last_error for a size the call refuses), 16-byte aligned; both owned by the call until the stream has passed it.
 *  Every argument is checked before the first device call.  No split-K and no floating-point atomics: the same bits on every call.
 *  Does not synchronise. */
typedef struct mg_lpips_net {
  const float* conv_w[5];
  const float* conv_b[5];
  const float* lin_w[5];
} mg_lpips_net;
long long mg_lpips_workspace_bytes(int H, int W);
int mg_eval_iid_lpips(const mg_lpips_net* net, const float* pred, const float* gt, const uint8_t* mask_or_null, int H, int W,
                      int up_to_scale, int gamma_mode, double* out8, void* eval_ws, void* act_ws, long long act_ws_bytes, void* stream);

/* The tiny autoencoder (diffusers' AutoencoderTiny with the TAESD layout: csrc/tinyvae.hip, DESIGN.md "Tiny VAE") as plain calls - no
 * op kind.  Every convolution is 3 x 3 / pad 1 and 64 channels wide; activations between layers are NHWC in the build's 16-bit operand
 * type (one pixel = one 128-byte line), sums are fp32.
 *  struct mg_tiny_vae: DEVICE pointers, in the layout the kernels read.  For either half (enc_ / dec_):
 *    in_w   fp32 [9 * Cin][64], row (ky * 3 + kx) * Cin + ci (Cin 3 / 4); values already rounded to the operand type
 *    in_b   fp32 [64]
 *    w[l]   operand type [9][64 out][64 in], tap ky * 3 + kx (torch's [out][in][ky][kx] permuted to [ky][kx][out][in]), the
 *           MG_TINY_VAE_LAYERS 64 -> 64 layers in execution order: encoder = Block, then three times (stride-2 conv, three Blocks);
 *           decoder = three times (three Blocks, conv on the nearest x2 input), then a Block; a Block is three layers
 *    b[l]   fp32 [64]; NULL (and ignored) for the bias-free layers: encoder 3, 13, 23, decoder 9, 19, 29
 *    out_w  fp32 [9][64 in][4], columns >= Cout (4 / 3) zero; values already rounded to the operand type
 *    out_b  fp32 [4]
 *    All 16-byte aligned.  A call reads only its own half; the other may be NULL.
 *  mg_tiny_vae_workspace_bytes(which, B, H, W): which 0 = encode (H, W: the image), 1 = decode (H, W: the latent); -1 with
 *    mg_last_error for a refused size (B, H, W < 1, more than 2^26 full-size pixels).
 *  mg_tiny_vae_encode: rgb fp32 [B][3][H][W] in [-1, 1] -> (x + 1) / 2 -> encoder -> latent fp32 [B][4][h][w], the SCALED latent
 *    (scaling factor 1), h = ceil(ceil(ceil(H / 2) / 2) / 2).
 *  mg_tiny_vae_decode: latent fp32 [B][4][h][w] -> 3 tanh(z / 3) -> decoder -> y 2 - 1 -> post (MG_POST_NONE, _DEPTH, _NORMALS, _UNIT with
 *    the semantics of MG_OP_POST_NCHW, NaN rules included) -> out fp32 [B][3 or 1 (DEPTH)][8 h][8 w].
 *  mg_tiny_conv3x3: the single 64 -> 64 layer.  x [B][H][W][64] -> out [B][Ho][Wo][64]: stride 1: Ho = H; stride 2: Ho = (H - 1) / 2 + 1;
 *    up2 (stride 1 only): the layer reads the nearest x2 of x (pixel (y >> 1, x >> 1)) and Ho = 2 H.  Epilogue in this order: + bias,
 *    + residual (operand type, at the output's pixel), ReLU (keeps NaN), one rounding to the operand type (overflow -> inf).  out may
 *    not alias x or the residual.
 *  ws: 16-byte aligned, owned by the call until the stream has passed it.  Every argument is checked before the first device call.  No
 *  split-K and no atomics: the same bits on every call, and a member's result does not depend on the batch it runs in.  None
 *  synchronises. */
#define MG_TINY_VAE_LAYERS 33
typedef struct mg_tiny_vae {
  const float* enc_in_w;
  const float* enc_in_b;
  const void* enc_w[MG_TINY_VAE_LAYERS];
  const float* enc_b[MG_TINY_VAE_LAYERS];
  const float* enc_out_w;
  const float* enc_out_b;
  const float* dec_in_w;
  const float* dec_in_b;
  const void* dec_w[MG_TINY_VAE_LAYERS];
  const float* dec_b[MG_TINY_VAE_LAYERS];
  const float* dec_out_w;
  const float* dec_out_b;
} mg_tiny_vae;
long long mg_tiny_vae_workspace_bytes(int which, int B, int H, int W);
int mg_tiny_vae_encode(const mg_tiny_vae* net, const float* rgb, float* latent, int B, int H, int W, void* ws, long long ws_bytes,
                       void* stream);
int mg_tiny_vae_decode(const mg_tiny_vae* net, const float* latent, float* out, int B, int h, int w, int post, void* ws,
                       long long ws_bytes, void* stream);
int mg_tiny_conv3x3(const void* x, const void* w, const float* bias_or_null, const void* residual_or_null, void* out, int B, int H, int W,
                    int stride, int up2, int relu, void* stream);

/* The device I/O boundary on raw pointers (csrc/resize.hip): MG_OP_RGB_PREP and MG_OP_NORMALS_VIS as calls; neither synchronises.
 *  mg_rgb_prepare: src uint8 [Hin][Win][3] (hwc != 0) or [3][Hin][Win] -> dst [3][Hout][Wout], fp32 or (out16 != 0) the build's 16-bit
 *  operand type; mode 0 bilinear / 1 bicubic / 2 nearest-exact when the sizes differ; reciprocal: see MG_RGB_PREP_I_RECIPROCAL;
 *  tmp: fp32 [3][Hin][Wout], needed by modes 0 and 1 when both sizes change.
 *  mg_normals_visualize: pred fp32 [3][H][W] -> out uint8 [H][W][3]. */
int mg_rgb_prepare(const uint8_t* src, int hwc, int Hin, int Win, void* dst, int out16, int Hout, int Wout, int mode, int reciprocal,
                   float* tmp_or_null, void* stream);
int mg_normals_visualize(const float* pred, int H, int W, uint8_t* out_hwc, void* stream);
/* The output stages of the depth and the normals pipeline as calls, one launch each; neither synchronises.  At least one output.
 *  mg_depth_visualize: MG_OP_COLORIZE over the range (0, 1) with its optional outputs - depth fp32 [n] -> clipped fp32 [n] (may be
 *  `depth` itself), u16 uint16 [n], picture uint8 [n][3] (needs lut256x3, the table on the device).
 *  mg_normals_finish: MG_OP_NORMALS_VIS's kernel - pred fp32 [3][H][W] -> clipped fp32 [3][H][W] = clip(pred, -1, 1), NaN kept (may be
 *  `pred` itself), picture uint8 [H][W][3]; four pixels per lane when H W % 4 == 0 and the pointers are 16- / 4-byte aligned, else
 *  one.  mg_normals_visualize is this call without the clipped map. */
int mg_depth_visualize(const float* depth, const uint8_t* lut256x3_or_null, int64_t n, float* clipped_out_or_null,
                       uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, void* stream);
int mg_normals_finish(const float* pred, int H, int W, float* clipped_out_or_null, uint8_t* picture_out_or_null, void* stream);

/* MG_OP_RANDN as a call: elements [offset, offset + n) of stream stream_id of seed -> dst (fp32, or with out16 != 0 the build's 16-bit
 * operand type).  Does not synchronise. */
int mg_randn(uint64_t seed, uint64_t stream_id, int64_t offset, int64_t n, void* dst, int out16, void* stream);
/* The ops that finish a picture, as calls (a C host need not fill in an mg_op): MG_OP_RESIZE (u8 != 0: uint8 planes, else fp32; tmp:
 * fp32 [planes][Hin][Wout] when modes 0 / 1 change both sizes), MG_OP_COLORIZE (lut256x3: the colour map's 256 x 3 uint8 table, e.g.
 * matplotlib's Spectral sampled at k / 255) and MG_OP_IID_VIS (bit t of linear_bits / up_to_scale_bits: target t; workspace fp32
 * [n_targets][MG_IID_VIS_PARTS] when a target is both).  None of them synchronises. */
int mg_resize(const void* src, void* dst, float* tmp_or_null, int planes, int Hin, int Win, int Hout, int Wout, int mode, int u8,
              void* stream);
int mg_colorize(const float* depth, const uint8_t* lut256x3, uint8_t* out_hwc, int64_t n, float min_depth, float max_depth, void* stream);
int mg_iid_visualize(const float* pred, uint8_t* out_hwc, float* workspace_or_null, int n_targets, int H, int W, int linear_bits,
                     int up_to_scale_bits, void* stream);

/* Host arithmetic of ensemble_depth's alignment objective (marigold/util/ensemble.py:129-152, as the closed form of
 * marigold_amd/ensemble.py): pairwise-RMSE cost of the aligned members and its gradient w.r.t. scales s[E] / shifts t[E],
 * from the per-member means mean[E] and the centred second-moment matrix C[E*E] gathered by MG_OP_ENS_DEPTH_STATS.
 * No device work; fp64; summation order = numpy's (bit-identical to the numpy form it replaces). */
int mg_ens_align_cost_grad(int E, const double* s, const double* t, const double* mean, const double* C,
                           double* cost, double* gs, double* gt);
/* scipy.optimize.minimize(fn, x, jac=True, method="BFGS", tol=gtol, options={"maxiter": maxiter}) restated natively
 * (scipy 1.15: _minimize_bfgs, DCSRCH line search with the Wolfe-2 fall-back, one objective evaluation per distinct point;
 * csrc/bfgs.hip).  fn(user, n, x, &f, g) returns 0.  x in / out; status = scipy's warnflag (0 converged, 1 maxiter,
 * 2 precision loss, 3 NaN).  Any n. */
int mg_bfgs_minimize(int (*fn)(void* user, int n, const double* x, double* f, double* g), void* user, int n, double* x,
                     double gtol, int maxiter, double* fval, int* nit, int* nfev, int* status);
/* The whole alignment of ensemble_depth (marigold/util/ensemble.py:154-173: compute_param + scipy BFGS) as one call: the
 * objective of mg_ens_align_cost_grad + the regulariser from one device pass per evaluation - reg_op, an
 * MG_OP_ENS_DEPTH_MEDIAN op whose scale / shift input st_host [2E] and (min, max, member values) output mm_host [2 + 2E]
 * live in host-mapped memory - times the forward-difference survival factor of the reference's fp32 parameter cast.
 * affine: scale + shift (n = 2E) or scale only; reduction 0 median / 1 mean; lam = regulariser strength. */
int mg_ens_align_minimize(const mg_op* reg_op, void* stream, int E, int affine, int reduction, double lam, const double* mean,
                          const double* C, float* st_host, const float* mm_host, double* x, double gtol, int maxiter,
                          double* fval, int* nit, int* nfev, int* status);

/* TILED predictions of a large picture (marigold_amd/tiles.py, pipe.predict_tiled): the picture is cut into overlapping
 * tiles of one size on a grid, every tile is predicted on its own, and the tiles are stitched on the device - depth tiles are first
 * fitted, scale and shift, to a low-resolution prediction of the whole picture (the guide), then every kind is blended with feathered
 * weights.  Plain C calls on device pointers, no op kind.  Every argument check comes before any GPU work and every message starts with
 * the function's name; nothing synchronises.  Lengths, tile extents and starts are in pixels of the working canvas Hw x Ww.
 *  The GRID: ny starts along y and nx along x (host arrays, 1 <= ny, nx <= MG_TILE_MAX_PER_AXIS; they travel as kernel arguments), tile
 *  i = iy * nx + ix (row-major) has its corner at (ystarts[iy], xstarts[ix]) and the extent th x tw.  Tiles are stored one after the
 *  other, fp32: [n][th][tw] (fit), [n][C][th][tw] (blend), 16-byte aligned.  th, tw, Hw, Ww are multiples of 8; every tile lies inside
 *  the canvas.
 *  mg_tile_plan: the starts along ONE axis - picture length L, tile length T, minimum overlap O, all multiples of 8.  L <= T: one
 *    tile at 0 (of extent L).  Else n = ceil((L - O) / (T - O)) tiles of extent T, start_i = 8 floor(i (L - T) / (n - 1) / 8) for
 *    i < n - 1 and start_{n-1} = L - T: consecutive tiles overlap by at least O, and THREE tiles may cover one coordinate (L = 120,
 *    T = 64, O = 16: 0, 24, 56).  Returns n and writes starts[0 .. n); -1 with mg_last_error for a length below 8 or no multiple of 8,
 *    O < 8, O > T / 2, n > MG_TILE_MAX_PER_AXIS, n > cap, a null `starts`.  Host only.
 *  mg_tiles_workspace_bytes: what mg_tile_fit needs for n tiles of th x tw (-1 with mg_last_error for a refused shape).
 *  mg_tile_fit (depth): per tile the (s, t) that minimise the unweighted sum over its pixels p of (s d(p) + t - G(p))^2, where G is the
 *    guide [hg][wg] sampled bilinearly at p's canvas position - align_corners = False with edge clamp, F.interpolate(guide, (Hw, Ww),
 *    mode="bilinear") - and only pixels where d and G are both finite count.  Sampling and the five sums N, Sd, Sg, Sdd, Sdg are fp64:
 *    chunks of MG_TILE_FIT_CHUNK pixels, lanes -> wave shuffle -> LDS -> one partial per chunk in `ws`, then a second launch adds the
 *    partials in a fixed order (a wave per tile) and solves s = (N Sdg - Sd Sg) / (N Sdd - Sd^2), t = (Sg - s Sd) / N.  No atomics:
 *    two runs give the same bits.  A tile is DEGENERATE when N < 2, when N Sdd - Sd^2 <= 1e-12 N^2 (a constant tile) or when s <= 0: it
 *    gets s = 0, t = Sg / N (t = 0 when N = 0) and flags[i] = 1, else flags[i] = 0.  coef [n][2] fp64 (s, t), flags [n] int32, ws
 *    16-byte aligned.
 *  mg_tile_blend: out(p) = sum_i w_i(p) v_i(p) / sum_i w_i(p) over the tiles covering p in row-major order, per channel (C = 1 depth,
 *    3 normals), v_i = fma(s_i, d_i, t_i) with (s_i, t_i) = coef[i] rounded to fp32, or v_i = d_i when coef is NULL.  w_i = wy wx; per
 *    axis, with u the coordinate inside the tile, T its extent and O the axis' overlap: min(lo, hi), lo = min(1, (u + 0.5) / O) where
 *    the tile has a neighbour before it and 1 at the canvas border, hi = min(1, (T - u - 0.5) / O) likewise behind it.  Every weight is
 *    positive (0.5 / O at a tile's edge), so any number of covering tiles may meet and the result is continuous across seams.  fp32, in
 *    this order: num = fma(w, v, num), den = den + w, out = num / den (IEEE division).  normalize = 1 (C = 3 only): the blended vector
 *    is divided by max(sqrt(x^2 + y^2 + z^2), 1e-6).  NaN and infinities propagate.  out [C][Hw][Ww] fp32, 16-byte aligned; four
 *    consecutive x per lane, float4 loads and stores.  The grid must cover the canvas - first start 0, last start + extent = the
 *    length, strictly ascending multiples of 8, consecutive tiles overlapping by at least O (oy along y, ox along x; >= 8, a multiple of 8,
 *    at most half the extent on an axis with several tiles). */
#define MG_TILE_MAX_PER_AXIS 32
#define MG_TILE_FIT_CHUNK 4096
int mg_tile_plan(int L, int T, int O, int* starts, int cap);
long long mg_tiles_workspace_bytes(int n, int th, int tw);
int mg_tile_fit(const float* tiles, int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx, int Hw, int Ww,
                const float* guide, int hg, int wg, double* coef, int* flags, void* ws, long long ws_bytes, void* stream);
int mg_tile_blend(const float* tiles, int C, int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx, int Hw, int Ww,
                  int oy, int ox, const double* coef_or_null, int normalize, float* out, void* stream);
/*  mg_tile_crop: the GATHER of the tiles out of the picture - `count` tiles of the grid, from tile `first` on in row-major order, copied
 *    into dst as `count` contiguous uint8 pictures of th x tw in the layout of src: src [Hw][Ww][3] and dst [count][th][tw][3] with
 *    hwc != 0, else src [3][Hw][Ww] and dst [count][3][th][tw].  One launch, no synchronisation; nothing outside dst[0, count 3 th tw)
 *    is written.  Starts and extents are multiples of 8, so every tile row begins on a multiple of 24 bytes (hwc) or 8 bytes (chw) of
 *    either buffer: a lane moves 8 bytes, as one 8-byte load and store where src and dst are both 8-byte aligned, byte by byte
 *    otherwise (the pointers themselves need no alignment).  Refused: a null pointer, th, tw, Hw, Ww or a start that is no multiple
 *    of 8, a tile outside the canvas, a canvas above 2^28 pixels, ny or nx outside 1 .. MG_TILE_MAX_PER_AXIS, first < 0, count < 1 or
 *    first + count > ny nx.  The grid need not cover the canvas. */
int mg_tile_crop(const uint8_t* src, int hwc, int Hw, int Ww, int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx,
                 int first, int count, uint8_t* dst, void* stream);

/* EDGE-GUIDED UPSAMPLING of a prediction to the picture's size (marigold_amd/guided.py, pipe(..., guided_upsample=True)):
 * joint bilateral upsampling - the low-resolution prediction is enlarged while the full-size picture decides which low-resolution
 * neighbours a pixel may borrow from.  A plain C call on device pointers, no op kind; one launch, no atomics (two runs give the same
 * bits), fp32 - the same bits from the bf16- and the fp16-operand build; it does not synchronise.
 *  pred      fp32 [C][h][w], 1 <= C <= 16 (1 depth, 3 normals, 3 per target for intrinsic images); 4-byte aligned
 *  guide_lo  uint8 planes [3][h][w]: the picture resampled to the prediction's size (mg_resize, u8, bilinear)
 *  guide_hi  uint8, the picture itself at H x W: [H][W][3] with hwc != 0, else [3][H][W]
 *  radius    R, 1 .. 4 (2 is the usual choice);  sigma  > 0, on the 0 .. 1 colour scale (0.1 is the usual choice)
 *  out       fp32 [C][H][W]; 4-byte aligned.  Any H, W, h, w >= 1, smaller or larger, up to 2^30 pixels either side.
 * For output pixel (Y, X), all in fp32:
 *    sy = (h / H) (Y + 0.5) - 0.5 with the scale float(h) / float(H) computed first, fy = floor(sy); sx, fx likewise
 *    taps i = fy - R + 1 .. fy + R and j = fx - R + 1 .. fx + R: (2R)^2 of them
 *    spatial weight  max(0, 1 - |sy - i| / R) max(0, 1 - |sx - j| / R)
 *    the tap's index is clamped into [0, h) x [0, w) AFTERWARDS (edge replication); the tap keeps its weight
 *    range weight    expf(-d2 / (2 sigma^2)) + 1e-4,  d2 = sum over the 3 colours of (guide_hi[Y, X, c] / 255 - guide_lo[c, i, j] / 255)^2
 *    out[c] = sum weight pred[c, i, j] / sum weight, evaluated as sum (weight / sum weight) pred[c, i, j] with IEEE divisions, the taps
 *    in row-major order: a pixel with ONE tap of non-zero weight returns that tap's value bit for bit (equal sizes and R = 1: out = pred)
 * The weights are computed once per pixel and serve every channel.  The floor 1e-4 keeps the denominator positive and lets the result
 * fall back to the spatial (tent) filter where no tap resembles the pixel; with R = 1 and a constant picture the result is bilinear
 * enlargement.  Non-finite values of pred propagate as this arithmetic gives (a tap of weight 0 with an infinite value gives NaN);
 * there is no special case.  Refused before anything is launched, the message starting with "mg_guided_upsample:": a null pointer, C
 * outside 1 .. 16, a size below 1 or above 2^30 pixels, a radius outside 1 .. 4, a sigma that is not > 0 or not finite (or whose
 * 2 sigma^2 leaves the fp32 range), pred or out not 4-byte aligned.  Guided output is no out_mode of the one-call predictions: a host
 * composes it (examples/host_guided.cpp). */
int mg_guided_upsample(const float* pred, int C, int h, int w, const uint8_t* guide_lo, const uint8_t* guide_hi, int hwc, int H, int W,
                       int radius, float sigma, float* out, void* stream);

/* DEPTH ALIGNMENT (marigold_amd/align.py, pipe(..., align=state), map_video(align=True)): the scale and shift that carry
 * one affine-invariant depth map into the range of another - a reference with trusted values at some pixels, or the frame before -
 * fitted robustly on the device, and their application.  Plain C calls on device pointers, no op kind.  Every argument check comes
 * before any GPU work and every message starts with the function's name; nothing synchronises.
 *  mg_depth_align_workspace_bytes: what mg_depth_align_fit needs for n pixels, 1 <= n <= 2^30 (-1 with mg_last_error otherwise).
 *  mg_depth_align_fit: d, ref fp32 [n]; mask uint8 [n] or NULL.  A pixel COUNTS when its mask byte is non-zero (or there is no mask) and
 *    d and ref are both finite.  All arithmetic is fp64.  One SOLVE, with weights w over the pixels that count: the sums N = sum w,
 *    Sd = sum w d, Sg = sum w ref, Sdd = sum w d^2, Sdg = sum w d ref - the terms are w d, (w d) d and (w d) ref, each product rounded -
 *    then, with fit_shift != 0, s = (N Sdg - Sd Sg) / (N Sdd - Sd^2), t = (Sg - s Sd) / N; with fit_shift = 0, s = Sdg / Sdd, t = 0.
 *    iters = 0: one solve with w = 1 - plain least squares; start_mode and the start values are ignored.  iters = k >= 1: k solves with
 *    the Cauchy weights w = 1 / (1 + r^2), r = ((s d + t) - ref) / delta, each from the coefficients of the solve before it; the first
 *    from (s_start, t_start) under MG_ALIGN_START_GIVEN, from an extra unweighted solve done first under MG_ALIGN_START_LS.  delta is
 *    in the units of ref: a residual of delta halves a pixel's weight.  The coefficients never leave the device between solves: the
 *    solve launch writes them to `coef`, where the next partial-sum launch reads them.  Sums as in mg_tile_fit: fixed chunks of
 *    pixels, lanes -> wave shuffle -> LDS -> one partial per chunk in `ws`, then a second launch (one wave) adds the partials in a fixed
 *    order and solves.  No atomics: two runs give the same bits, and so do the bf16- and the fp16-operand build.  The fit is
 *    DEGENERATE when fewer than 2 pixels count, when N Sdd - Sd^2 <= 1e-12 N^2 (with shift) or Sdd <= 1e-12 N (without), or when a
 *    solve yields s <= 0 or a coefficient that is not finite: then coef = (1, 0) and flag = 1, and the remaining solves change
 *    nothing; else flag = 0.  coef DEVICE fp64 [2] (s, t), flag DEVICE int32 [1], ws 16-byte aligned.  Refused: n < 1 or > 2^30, a
 *    null d, ref, coef, flag or ws, pointers not aligned to their elements, ws_bytes too small or ws not 16-byte aligned, iters outside
 *    0 .. MG_ALIGN_MAX_ITERS, and with iters >= 1 an unknown start_mode, a delta that is not finite or <= 0, start values that are not
 *    finite under MG_ALIGN_START_GIVEN.
 *  mg_depth_align_apply: out[i] = (float)((double)x[i] * coef[0] + (use_shift ? coef[1] : 0)) - the product and the sum each rounded
 *    in fp64, then one rounding to fp32.  With clip_lo <= clip_hi the result v is clamped as v < lo ? lo : (v > hi ? hi : v), so a NaN
 *    stays a NaN; clip_lo > clip_hi (or a NaN bound) means no clamp.  out may be x.  Four elements per lane where x and out are both
 *    16-byte aligned, element by element otherwise and for the n % 4 tail.  use_shift = 0 is how an uncertainty map follows its
 *    depth map.  Refused: n < 1 or > 2^30, a null x, coef or out, pointers not aligned to their elements.
 * Alignment is no stage of the one-call predictions: a host composes it (examples/host_align.cpp). */
#define MG_ALIGN_MAX_ITERS 32
enum { MG_ALIGN_START_GIVEN = 0, MG_ALIGN_START_LS = 1 };
long long mg_depth_align_workspace_bytes(long long n);
int mg_depth_align_fit(const float* d, const float* ref, const unsigned char* mask_or_null, long long n,
                       int fit_shift, int iters, int start_mode, double s_start, double t_start, double delta,
                       double* coef, int* flag, void* ws, long long ws_bytes, void* stream);
int mg_depth_align_apply(const float* x, long long n, const double* coef, int use_shift,
                         float clip_lo, float clip_hi, float* out, void* stream);

/* DEPTH TO 3D (marigold_amd/points.py): camera-space points and surface normals from a depth map on the device - the
 * dense normals map, and the kept pixels compacted into a point cloud in row-major order without the host learning their number.
 * Plain C calls on device pointers, no op kind.  Every argument check comes before any GPU work and every message starts with the
 * function's name; nothing synchronises.  No atomics: two runs give the same bits, and so do the bf16- and the fp16-operand build.
 * All arithmetic is fp64, every product, sum and quotient rounded on its own in the order written here; results are rounded once to
 * fp32.
 *  CAMERA.  fx, fy, cx, cy in pixels of the map's own grid.  Pixel (row y, column x) sits at image coordinates (x, y), integer
 *    coordinates at pixel centres.  The camera frame is x right, y down, z forward.
 *  DEPTH.  z = (double)d without coef; with coef, a DEVICE fp64 [2] (what mg_depth_align_fit leaves, or two uploaded numbers),
 *    z = (double)d * coef[0] + coef[1], the product and the sum each rounded.
 *  USABLE pixel: its mask byte is non-zero (or there is no mask), d and z are finite, and z_min < z <= z_max (z_min >= 0; z_max may be
 *    +inf).
 *  JOINED: two usable 4-neighbours p, q are joined when edge_rel == 0 or |z_p - z_q| <= edge_rel * min(z_p, z_q) - the flying-pixel
 *    rule.
 *  KEPT pixel: usable and joined to every usable in-bounds 4-neighbour.  Neighbours that are not usable do not count against it.
 *  POINT: X = ((x - cx) * z) / fx, Y = ((y - cy) * z) / fy, Z = z; each rounded to fp32 for the record, the fp64 values serve the normal.
 *  NORMAL of a kept pixel p: the horizontal tangent Tu is P_east - P_west when both neighbours are joined to p, the one-sided
 *    difference P_east - P_p or P_p - P_west with one of them, and with none there is no normal; the vertical tangent Tv likewise,
 *    south minus north.  N = Tv x Tu, each component a b - c d with both products rounded:
 *    (Tv.y Tu.z - Tv.z Tu.y, Tv.z Tu.x - Tv.x Tu.z, Tv.x Tu.y - Tv.y Tu.x).  A dot product is (a.x b.x + a.y b.y) + a.z b.z.  If
 *    N . P > 0, N is negated: the normal looks at the camera.  Then N is divided, component by component, by sqrt(N . N); there is no
 *    normal when N . N is zero or not finite.  normals_frame MG_NORMALS_FRAME_CAMERA gives N in the camera frame (a wall facing the
 *    camera: (0, 0, -1)); MG_NORMALS_FRAME_MARIGOLD gives (Nx, -Ny, -Nz): x right, y up, z toward the viewer (that wall: (0, 0, 1)) -
 *    how this model family's normal maps are published and what mg_eval_normals takes.
 *  mg_depth_normals: d fp32 [h][w], mask uint8 [h][w] or NULL, coef or NULL -> out fp32 [3][h][w] and valid uint8 [h][w].  A pixel
 *    that is not kept or has no normal gets zeros and a zero byte.  One launch.
 *  mg_depth_points_workspace_bytes: what mg_depth_points needs for n = h w pixels, 1 <= n <= 2^30 (-1 with mg_last_error otherwise).
 *  mg_depth_points: colors uint8 [h][w][3] with hwc != 0, planes [3][h][w] with hwc = 0, or NULL.  Outputs: xyz fp32 [capacity][3];
 *    rgb uint8 [capacity][3], given exactly when colors is; nrm fp32 [capacity][3] or NULL; index int32 [capacity] or NULL, the source
 *    pixel's row-major index; count DEVICE int64 [2]: the kept pixels, and the records written = min(kept, capacity).  The records are
 *    in row-major pixel order; nothing at or past record `written` is touched; a kept pixel without a normal is still a record, with
 *    the normal (0, 0, 0).  Three launches, none of which waits on another workgroup: the kept pixels of every chunk of 2048 are
 *    counted; one workgroup adds the counts in chunk order into the chunks' offsets and `count`; the scatter decides again what is
 *    kept and ranks a pixel within its chunk with 64-lane ballots and population counts.  ws, 16-byte aligned, holds the chunks' counts
 *    and offsets and nothing else; it is the call's until the stream has passed it.
 * Refused by both calls: a null d, out, valid, xyz, count or ws; colors without rgb or rgb without colors; h or w below 1 or more than
 * 2^30 pixels; fx or fy not finite or <= 0; cx or cy not finite; z_min negative or not finite; z_max NaN or <= z_min; edge_rel
 * negative or not finite; an unknown normals_frame; capacity < 1; fp32, int32, int64 or fp64 pointers not aligned to their elements;
 * ws_bytes too small or ws not 16-byte aligned.
 * Points are no stage of the one-call predictions: a host composes them (examples/host_points.cpp). */
enum { MG_NORMALS_FRAME_CAMERA = 0, MG_NORMALS_FRAME_MARIGOLD = 1 };
int mg_depth_normals(const float* d, const unsigned char* mask_or_null, const double* coef_or_null, int h, int w,
                     double fx, double fy, double cx, double cy, double z_min, double z_max, double edge_rel, int normals_frame,
                     float* out, unsigned char* valid, void* stream);
long long mg_depth_points_workspace_bytes(long long n);
int mg_depth_points(const float* d, const unsigned char* colors_or_null, int hwc, const unsigned char* mask_or_null,
                    const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy,
                    double z_min, double z_max, double edge_rel, int normals_frame, long long capacity,
                    float* xyz, unsigned char* rgb_or_null, float* nrm_or_null, int* index_or_null, long long* count,
                    void* ws, long long ws_bytes, void* stream);

/* DEPTH TO MESH (marigold_amd/mesh.py): the depth map as a triangle mesh on the device - vertices, and triangles that
 * stop at depth edges, both compacted without the host learning a count.  CAMERA, DEPTH, USABLE, POINT and the arithmetic are those of
 * DEPTH TO 3D above, unchanged; JOINED(p, q), edge_rel == 0 or |z_p - z_q| <= edge_rel * min(z_p, z_q), is asked here of any two usable
 * pixels, diagonal neighbours included.  A plain C call on device pointers, no op kind; every check before any GPU work; nothing
 * synchronises; no atomics: every output byte is a function of the inputs alone, and the same in both operand builds.
 *  CELL (x, y), 0 <= x < w - 1, 0 <= y < h - 1, has the corners A = (x, y), B = (x + 1, y), C = (x, y + 1), D = (x + 1, y + 1).
 *  CANDIDATE triangles of a cell.  Four usable corners: the cell is split along A-D when |z_A - z_D| <= |z_B - z_C| (fp64, each
 *    difference rounded on its own), else along B-C.  Split A-D: T0 = (A, C, D), T1 = (A, D, B).  Split B-C: T0 = (A, C, B),
 *    T1 = (B, C, D).  Exactly three usable corners: one candidate, in slot T0 - D missing: (A, C, B); A missing: (B, C, D); B missing:
 *    (A, C, D); C missing: (A, D, B).  Fewer than three: none.  In every order above (P1 - P0) x (P2 - P0) points toward the camera,
 *    the orientation of N = Tv x Tu.
 *  FACE: a candidate all three of whose edges are joined.  With four usable corners the split is chosen first; then each of its two
 *    triangles stands or falls on its own.  Faces are ordered by cell in row-major order, inside a cell T0 before T1.
 *  VERTEX: a usable pixel that is a corner of at least one face.  Vertices are in row-major pixel order; the three int32 entries of a
 *    face are its corners' ranks in that order.
 *  Vertex record: xyz fp32, the POINT, one rounding; rgb, given exactly when colors is: the picture's bytes; index or NULL: the
 *    row-major pixel index; nrm or NULL: the NORMAL rule above - central, one-sided or no tangent per axis, turned toward the camera,
 *    either frame - where a 4-neighbour counts for a tangent when it is usable and joined to this pixel.  The demotion of a KEPT pixel
 *    (a usable neighbour that is not joined) does not apply to a vertex.  A vertex without a normal gets zeros.
 *  count DEVICE int64 [4]: V, V_written = min(V, capacity_v), F, F_written = min(F, capacity_f) when V <= capacity_v, else 0 - a mesh
 *    whose vertices were cut has no faces that could be trusted.  Nothing at or past the written records is touched.  A map with
 *    h == 1 or w == 1 has no cells: the call succeeds with four zeros.
 *  mg_depth_mesh_workspace_bytes: what mg_depth_mesh needs for n = h w pixels, 1 <= n <= 2^30 (-1 with mg_last_error otherwise): the
 *    face and vertex counts and offsets of the chunks of 2048 pixels, an int32 [n] map of the vertices' ranks and a byte per cell.
 *  mg_depth_mesh: the arguments of mg_depth_points with capacity_v, capacity_f, faces int32 [capacity_f][3] and count [4].  Five
 *    launches, none of which waits on another workgroup: every cell's code (its split or three-corner form, which of T0 / T1 are
 *    faces) and the chunks' face counts; the chunks' vertex counts from the codes of the up to four cells around a pixel; one workgroup
 *    adds both tables in chunk order into offsets and writes count; the vertex scatter, which also writes the rank map; the face
 *    scatter, which reads it.  Ranks inside a chunk come from 64-lane ballots and population counts.
 * Refused, the message starting with "mg_depth_mesh:": everything mg_depth_points refuses about d, colors and rgb, the map, the camera,
 * the range, edge_rel and the frame; a null xyz, faces, count or ws; capacity_v or capacity_f below 1; xyz, nrm, index, faces, count or
 * coef not aligned to their elements; ws not 16-byte aligned or ws_bytes too small.  examples/host_mesh.cpp composes a prediction, the
 * colours and this call into a PLY. */
long long mg_depth_mesh_workspace_bytes(long long n);
int mg_depth_mesh(const float* d, const unsigned char* colors_or_null, int hwc, const unsigned char* mask_or_null,
                  const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy,
                  double z_min, double z_max, double edge_rel, int normals_frame, long long capacity_v, long long capacity_f,
                  float* xyz, unsigned char* rgb_or_null, float* nrm_or_null, int* index_or_null, int* faces, long long* count,
                  void* ws, long long ws_bytes, void* stream);

/* DEPTH TO VIEW (marigold_amd/view.py): the picture seen from a moved camera - the FACES of DEPTH TO MESH above, transformed
 * into a second pinhole camera, drawn into a 64-bit depth-and-id buffer with integer atomic minima and resolved to a picture, a depth
 * map and a validity map, with optional filling of the disocclusion holes.  CAMERA, DEPTH, USABLE, POINT, JOINED, CELL, CANDIDATE and
 * FACE are those above, unchanged.  A plain C call on device pointers, no op kind; every check before any GPU work; nothing
 * synchronises.  Integer minima and integer sums commute, and there are no float atomics, no tickets and no workgroup that waits on
 * another: every output byte is a function of the inputs alone, and the same in both operand builds.  All floating arithmetic is fp64,
 * every product, sum and quotient rounded on its own in the order written here; all coverage arithmetic is int64.
 *  TARGET CAMERA.  fx2, fy2, cx2, cy2 and a size h2 x w2, under the CAMERA conventions.  pose is a HOST pointer to 12 doubles, the
 *    rows of [R | t] (R00 R01 R02 t0, R10 ...), read before the call returns, or NULL for the identity.  R need not be orthonormal,
 *    only finite; a mirror is a legal input.
 *  TRANSFORM of a corner with the fp64 POINT (X, Y, Z) - not the record rounded to fp32: X' = ((R00 X + R01 Y) + R02 Z) + t0, Y' and
 *    Z' likewise with rows 1 and 2; u = (fx2 X') / Z' + cx2, v = (fy2 Y') / Z' + cy2, q = 1 / Z'.
 *  DROPPED faces.  A face is dropped, and counted once, under the first reason that applies:
 *    1. near: some corner's Z' is not finite or is < z_near (z_near > 0).  There is no clipping.
 *    2. off: some corner's |u| or |v| is not <= 2^20 (a NaN is off).
 *    3. back: with the snapped corners xi = llrint(256 u), yi = llrint(256 v) (round half to even), the doubled signed area
 *       A = (x2 - x0) (y1 - y0) - (x1 - x0) (y2 - y0) <= 0.  The identity view gives A > 0 for every face.
 *    4. span: the box of pixel centres ceil(min xi / 256) .. floor(max xi / 256), and the same in y, before clamping to the target,
 *       is wider or taller than MG_VIEW_MAX_SPAN pixels.  The cap is a condition, not a tuning: it bounds one lane's loop at 4096
 *       pixel tests and keeps every edge value below 2^30, so that its conversion to fp64 is exact.  A surface magnified that far
 *       gives holes and a non-zero count.
 *    A face that is not dropped is drawn, whether or not it covers a pixel centre of the target.
 *  COVERAGE.  With E(a, b, c) = (c.x - a.x) (b.y - a.y) - (b.x - a.x) (c.y - a.y), so that A = E(P0, P1, P2), the pixel centre
 *    p = (256 px, 256 py) has the edge values e0 = E(p, P1, P2), e1 = E(P0, p, P2), e2 = E(P0, P1, p); e0 + e1 + e2 == A.  It is
 *    covered when all three are >= 0: the rule is inclusive on every edge.  A pixel on a shared edge or on a vertex is offered by
 *    every face that touches it and the depth buffer decides: there are no cracks, and the last row and column of an identity view
 *    are covered.
 *  DEPTH and KEY of an offer: s = (e0 q0 + e1 q1) + e2 q2, Zv = (float)((double)A / s); the offer is skipped unless Zv is finite and
 *    > 0.  key = (bits of Zv) << 32 | face_id, face_id = 2 * (row-major index of the cell's corner A) + slot (T0: 0, T1: 1; below
 *    2^31).  The smallest key wins: the nearest surface, and the lowest face id on equal fp32 depth.
 *  COLOUR of the winner, per channel, c0 c1 c2 the picture's bytes at its corners: c = (((e0 q0) c0 + (e1 q1) c1) + (e2 q2) c2) / s,
 *    byte = min((int)(c + 0.5), 255).  At a vertex this is the vertex's byte.
 *  FILL.  fill_radius r, 0 .. MG_VIEW_MAX_FILL, 0: none.  A pixel that no face covers looks along its row for the nearest covered
 *    pixel within r on the left and within r on the right - covered by a face, never by a fill - and takes the depth and the colour
 *    of the one with the larger depth (the background); with only one, that one; on equal depth the left.
 *  Outputs: rgb uint8 in the layout of colors ([h2][w2][3] with hwc != 0, planes [3][h2][w2] with hwc = 0); depth fp32 [h2][w2];
 *    valid uint8 [h2][w2]: 1 where a face covers the pixel, 2 where filled, 0 elsewhere, where depth and rgb are zeros; face int32
 *    [h2][w2] or NULL: the winning face id, -1 where no face covers the pixel, filled or not; count DEVICE int64 [8]: faces, drawn,
 *    near, off, back, span, pixels covered, pixels filled.  A map with h == 1 or w == 1 has no cells: zeros everywhere.
 *  mg_depth_view_workspace_bytes: what mg_depth_view needs for n2 = h2 w2 target pixels, 1 <= n2 <= 2^30 (-1 with mg_last_error
 *    otherwise): 8 bytes per target pixel, rounded up to 16 bytes; the counts are summed in count itself.
 *  mg_depth_view: three launches - the key buffer to "no offer" and count to zeros; the splat, one lane per cell, a 64-bit atomic
 *    minimum per offer, the face counts summed per workgroup and added with integer atomics; the resolve, one lane per target pixel,
 *    which computes the winning face again from its id and fills from the key buffer, so that filled pixels never feed other fills.
 * Refused, the message starting with "mg_depth_view:": a null d, colors, rgb, depth, valid, count or ws; everything mg_depth_points
 * refuses about the map, the camera, the range and edge_rel; a target below 1 x 1 or above 2^30 pixels; fx2 or fy2 not finite or <= 0;
 * cx2 or cy2 not finite; a pose entry that is not finite; z_near not finite or <= 0; fill_radius outside 0 .. MG_VIEW_MAX_FILL; d,
 * depth, face, count or coef not aligned to their elements; ws not 16-byte aligned or ws_bytes too small.  examples/host_view.cpp
 * composes a prediction, the colours and two of these calls into a stereo pair. */
#define MG_VIEW_MAX_SPAN 64
#define MG_VIEW_MAX_FILL 64
long long mg_depth_view_workspace_bytes(long long n2);
int mg_depth_view(const float* d, const unsigned char* colors, int hwc, const unsigned char* mask_or_null,
                  const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy,
                  double z_min, double z_max, double edge_rel, const double* pose_or_null,
                  double fx2, double fy2, double cx2, double cy2, int h2, int w2, double z_near, int fill_radius,
                  unsigned char* rgb, float* depth, unsigned char* valid, int* face_or_null, long long* count,
                  void* ws, long long ws_bytes, void* stream);

/* DEPTH TO FOCUS (marigold_amd/focus.py): the picture refocused from its depth map - a synthetic shallow depth of field.
 * Every pixel is blurred by the circle of confusion its distance from a focus distance implies; near, blurred surfaces spread over what
 * is behind them, and a sharp foreground is not polluted by its blurred background.  DEPTH (z, coef) and USABLE (mask, z_min, z_max) are
 * those of DEPTH TO 3D above, unchanged; there is no camera.  A plain C call on device pointers, no op kind; every check before any GPU
 * work; nothing synchronises.  Everything after the blur radius is integer arithmetic, and integer sums commute: every output byte is a
 * function of the inputs alone, and the same in both operand builds.  There are no float atomics, no tickets and no workgroup that
 * waits on another.
 *  FOCUS DISTANCE zf.  With focus_x >= 0 and focus_y >= 0 it is the fp64 z of pixel (row focus_y, column focus_x), read on the device:
 *    a host can focus on a pixel of a prediction it has never seen.  With focus_x == focus_y == -1 it is the host double z_focus.
 *  BLUR RADIUS of a usable pixel, fp64, every operation rounded on its own: b = gain * fabs(1.0 / z - 1.0 / zf) in
 *    MG_FOCUS_SPACE_LENS - the thin lens: gain = 0.5 * fx * aperture, the aperture in the units of z - and b = gain * fabs(z - zf) in
 *    MG_FOCUS_SPACE_LINEAR.  r16 = !(b < max_radius) ? 16 * max_radius : (int)llrint(16.0 * b) (round half to even): the radius in
 *    sixteenths of a pixel, capped; a NaN is capped.  gain is finite and >= 0, max_radius 0 .. MG_FOCUS_MAX_RADIUS.  z_min >= 0, as
 *    USABLE requires, so a usable z is > 0 and 1.0 / z is finite or +inf.
 *  BAD FOCUS: the focus pixel is not usable, or zf is not finite, or zf <= 0 in MG_FOCUS_SPACE_LENS.  Then count[4] = 1, every r16 is 0
 *    and rgb is the source, byte for byte.  Otherwise count[4] = 0.
 *  ORDER.  q is in front of or level with p when (float)z_q <= (float)z_p, each z rounded once to fp32.
 *  CONTRIBUTION.  For a usable target p and every usable q inside the picture at the offset (dx, dy), |dx|, |dy| <= max_radius:
 *    e = r16_q when q is in front of or level with p, else e = min(r16_q, r16_p); q contributes when
 *    256 * (dx * dx + dy * dy) <= e * e, in integers.  p always contributes to itself.
 *  WEIGHT.  W[e] = floor(2^24 / N[e]), N[e] the number of integer offsets of the whole plane with 256 * (dx^2 + dy^2) <= e^2: N[0] = 1,
 *    N[16] = 5, N[512] = 3209, so W >= 5228.  N is not clipped at the picture's border.
 *  RESULT.  D = sum of W and C_k = sum of W * c_k over the contributions, c_k the source byte of channel k, in unsigned 64-bit integers
 *    (at most 4225 * 2^24 * 255 < 2^45); the output byte is (C_k + D / 2) / D, integer divisions.  A target that is not usable keeps its
 *    source bytes.
 *  Inputs: d fp32 [h][w]; colors uint8 [h][w][3] with hwc != 0, planes [3][h][w] with hwc = 0; mask uint8 [h][w] or NULL; coef or NULL.
 *  Outputs: rgb uint8 in the layout of colors; valid uint8 [h][w]: 1 usable, 0 not; radius uint16 [h][w] or NULL: r16, 0xFFFF where
 *    the pixel is not usable; count DEVICE int64 [5]: usable pixels, sharp pixels (r16 == 0), capped pixels (r16 == 16 * max_radius,
 *    counted when max_radius > 0), contributions summed over all targets, the bad-focus flag.
 *  mg_depth_focus_workspace_bytes: what mg_depth_focus needs for n = h w pixels, 1 <= n <= 2^30 (-1 with mg_last_error otherwise):
 *    (float)z and r16 of every pixel, 6 bytes, each of the two arrays rounded up to 16 bytes.
 *  mg_depth_focus: three launches - count to zeros; the prepare, one lane per pixel, which writes (float)z and r16 to the workspace,
 *    valid and radius, and adds the three pixel counts with integer atomics, one per workgroup; the gather, a workgroup per tile of
 *    32 x 8 targets, which takes the largest r16 within max_radius of its tile - no tap beyond that radius can contribute - stages
 *    the tile and a halo of that radius in LDS and sums every target's window from there.  The weights are a compile-time table.
 * Refused, the message starting with "mg_depth_focus:": a null d, colors, rgb, valid, count or ws; everything mg_depth_points refuses
 * about the map and the range; a space other than the two; gain not finite or < 0; max_radius outside 0 .. MG_FOCUS_MAX_RADIUS; a
 * focus pair that is neither a pixel nor (-1, -1), or a pixel outside the picture; d, radius, count or coef not aligned to their
 * elements; ws not 16-byte aligned or ws_bytes too small.  examples/host_focus.cpp composes a prediction, the colours and this call
 * into a picture. */
#define MG_FOCUS_MAX_RADIUS 32
enum { MG_FOCUS_SPACE_LENS = 0, MG_FOCUS_SPACE_LINEAR = 1 };
long long mg_depth_focus_workspace_bytes(long long n);
int mg_depth_focus(const float* d, const unsigned char* colors, int hwc, const unsigned char* mask_or_null,
                   const double* coef_or_null, int h, int w, double z_min, double z_max,
                   int space, double gain, int max_radius, int focus_x, int focus_y, double z_focus,
                   unsigned char* rgb, unsigned char* valid, unsigned short* radius_or_null, long long* count,
                   void* ws, long long ws_bytes, void* stream);

/* The TILED prediction of a large picture as ONE call (pipe.predict_tiled for a host without Python): from the uint8 bytes of the
 * picture and a seed to the stitched, clipped map at the size asked for, the stitched uncertainty, the 16-bit depth and the picture.
 * It runs on a model image of several configurations (export_model_image(configs=[...])), which the host finds with
 * mg_model_find_config:
 *  tiled.tile_config   the tiles' configuration: its size cfg[MG_CFG_HEIGHT] x cfg[MG_CFG_WIDTH] is the tile size th x tw (multiples of 8, decoded at that
 *                      size, at most the picture's), K = cfg[MG_CFG_PICTURES] >= 1 tiles per call, B = cfg[MG_CFG_MEMBERS] members each
 *  tiled.guide_config  depth only (ignored for normals): a configuration of ONE picture per call, of the same kind and with the same
 *                      B, whose size is the processed size of the guide (mg_processed_size(Hin, Win, guide_res))
 *  tiled.overlap_y/_x  the minimum overlap of neighbouring tiles
 *  tiled.tail_config   -1, or the configuration that runs the SHORT LAST GROUP: of the tile configuration's kind, size and B, with
 *                      exactly r = n mod K pictures per call (ignored when r = 0).  map_images runs a group of r < K tiles as a
 *                      program of r pictures, so with it the call is predict_tiled bit for bit; with -1 the last group follows
 *                      mg_model_predict_many's rule for n < K on tile_config - the same up to the arithmetic of the larger batch
 * The call selects the configurations itself and leaves the handle on the one that was selected before it (the sequence state of
 * mg_model_predict_next is neither read nor changed).  The chain, every step the code the other calls run:
 *  1. the plan: mg_tile_plan(Hin, th, overlap_y) and mg_tile_plan(Win, tw, overlap_x); n = ny nx tiles
 *  2. depth: the guide = the chain of mg_model_predict on guide_config with `seed`, clipped to [0, 1]; its info4 goes to `info4`
 *  3. the tiles in groups of K in row-major order: mg_tile_crop gathers a group, which runs the chain of mg_model_predict_many on
 *     tile_config - tile i with the seed (seed + 1 + i) mod 2^64 - to the decoded size, clipped; a short last group follows that
 *     call's rule for n < K, or runs whole on tail_config.  The maps go to one buffer [n][C][th][tw], with B > 1 and unc_out given the uncertainties to [n][th][tw]
 *  4. depth: mg_tile_fit against the guide, mg_tile_blend with its coefficients; normals: mg_tile_blend(normalize = 1).  The
 *     uncertainty: normals - mg_tile_blend of the tiles' uncertainties; depth - mg_tile_blend with the coefficients (s_i, 0), the
 *     scales of the fit: a tile's uncertainty is in units of its own normalised depth.  A degenerate tile (s_i = 0) contributes 0
 *     with its weight.
 *  5. with out_opts.out_h x out_w set and different from Hin x Win the stitched prediction - not the uncertainty - is resampled to
 *     them; then the output stage of mg_model_predict_out.
 *  rgb, mode, reciprocal, opts, out_opts   as in mg_model_predict_out; mode and reciprocal act in mg_rgb_prepare of the guide; the
 *              tiles are not resampled and always take reciprocal = 1, as the crops predict_tiled cuts on the device do;
 *              out_opts NULL or 0 x 0: Hin x Win
 *  pred_out    fp32 [channels][out_h][out_w], clipped; 16-byte aligned
 *  unc_out     fp32 [Hin][Win] | NULL, written when B > 1; 16-byte aligned
 *  u16_out, picture_out   as in mg_model_predict_out, at out_h x out_w
 *  info4       HOST double [4] | NULL: the guide's, as in mg_model_predict (zeros for normals)
 *  degenerate  DEVICE int32 [n] | NULL, depth only: mg_tile_fit's flag of every tile; their sum is the `degenerate_tiles` of
 *              pipe.predict_tiled.  Left to the device so that the call need not wait for it.
 * The working size is Hin x Win (multiples of 8): a host that wants another (predict_tiled's tiled_res) resamples the picture itself.
 * The temporaries - crops, tile maps, tile uncertainties, fit workspace, coefficients, canvas - are the model's: grown on demand,
 * counted by mg_model_device_bytes, freed by mg_model_destroy; mg_model_scratch_fill fills them too.  Synchronises where
 * mg_ensemble_depth does (depth, B > 1: once for the guide and once per tile) and nowhere else.  Refused before anything is launched,
 * the message starting with "mg_model_predict_tiled:": a null model, picture, tiled or pred_out; a host-only model; an
 * intrinsic-image model; Hin or Win that is no multiple of 8; configuration indices out of range; a tile configuration whose size is
 * no multiple of 8, is not decoded at its own size or exceeds the picture; a plan of ONE tile (that picture goes through
 * mg_model_predict_out); a guide configuration with K > 1, another B or another kind than the tile configuration; a tail configuration of
 * another kind, size or B than the tile configuration or with another K than n mod K; outputs that are
 * not 16-byte aligned; every refusal of mg_tile_plan and every output-option refusal of mg_model_predict_out, in their own words.
 * pipe.predict_tiled(tile_size=(th, tw), tile_overlap=..., guide_res=..., tiles_per_program=K, in_flight=1,
 * generator=NativeNoise(seed), match_input_res=True, ensemble_kwargs=dict(output_uncertainty=True)) gives the same arrays and
 * pictures, bit for bit (tests/test_gpu_predict_tiled_c_host.py; examples/host_tiled.cpp).  Tiled intrinsic images, member-parallel
 * pipelines and sequences of tiled pictures are not covered. */
typedef struct mg_tiled_opts {
  int guide_config, tile_config;   /* indices of mg_model_find_config */
  int overlap_y, overlap_x;        /* minimum overlap of neighbouring tiles, multiples of 8 */
  int tail_config;                 /* -1 | the configuration of n mod K pictures per call for the short last group */
} mg_tiled_opts;
int mg_model_predict_tiled(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                           const mg_tiled_opts* tiled, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                           float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                           double* info4_or_null, int* degenerate_or_null, void* stream);

/* Shader clock under matrix-core load, for bench.py's calibration block (the sysfs sensors do not answer on every box): one
 * workgroup per CU (one wave per SIMD) runs a fixed chain of v_mfma_f32_32x32x16_bf16 on random (zero_operands = 0) or zero
 * operands for ~2 ms and times it with s_memtime (shader cycles) against s_memrealtime (100 MHz).  mhz = mean over the
 * workgroups; tflops = the chain's rate (the clock-limited MFMA roof of this box on this data).  Synchronises the stream. */
int mg_clock_probe(void* stream, int zero_operands, double* mhz, double* tflops);

/* Tuning only (MARIGOLD_TUNING=1 MARIGOLD_IGEMM_STAMPS=1): the per-workgroup phase stamps of the last forced-tile MG_OP_IGEMM
 * launch (8 x uint64 of the 100 MHz s_memrealtime per workgroup, in the split-K workspace) -> host.  tools/igemm_phases.py. */
int mg_debug_read_workspace(void* host_dst, long long bytes);

/* HIP-event timing helpers for bench.py (the kernels run on the caller's stream). */
void* mg_event_create(void);
int mg_event_record(void* ev, void* stream);
int mg_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
void mg_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* MARIGOLD_HIP_H */
