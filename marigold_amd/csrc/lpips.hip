// LPIPS (AlexNet features) of one intrinsic-image target on the device, fp32 throughout: the third score of the reference's
// script/iid/eval.py:112-131 beside PSNR and SSIM (evalscore.hip).  The definition is the docstring of evaluation/metrics.py:lpips;
// the constants below restate it and are the only place the device path names them.
//
// Activations are channels-last, both images stacked along the rows: a map is fp32 [2 * Ho * Wo][C] (row = image, y, x), so one
// weight tile serves both images, the K gather of the next convolution and the channel norm of the distance are contiguous.
//  lpips_conv_kernel   implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fma chain): M = 2 * Ho * Wo, N = Cout,
//                      K = k * k * Cin in (ky, kx, ci) order; a 128 x 128 x 32 LDS-staged tile per workgroup of four waves, 2 x 2 MFMA tiles
//                      of 32 x 32 per wave; bias + ReLU in the epilogue.  One workgroup owns its K range whole: no split-K, no
//                      floating-point atomics, the bits do not depend on scheduling.  The first layer's staging reads the two images as
//                      the scores see them (IidImages: gamma, (s, q), mask -> 0), then 2x - 1 and the scaling layer; zero padding is
//                      of the scaled tensor.
//  lpips_pool_kernel   3 x 3 / 2 max-pool (floor, no padding) of a tap into the next convolution's input.
//  lpips_range_kernel  elements of either image outside [0, 1] (NaN counts) among the valid ones: every element once, which the first
//                      convolution's staging cannot give (its windows overlap, and the last rows / columns of some sizes lie in no window);
//                      an integer atomic.
//  lpips_dist_kernel   per position, one wave: both channel norms, then the weighted squared difference of the unit vectors, in fp32;
//                      the spatial sum in fp64, wave -> block -> a partial table that lpips_final_kernel adds; the order is reduce.h's.
#include <math.h>
#include <string.h>

#include "common.h"
#include "iid_images.h"
#include "reduce.h"

namespace {

// ---- the definition's constants -------------------------------------------------------------------------------------------
constexpr float LPIPS_SHIFT[3] = {-0.030f, -0.088f, -0.188f};   // scaling layer: (x - shift) / scale per channel
constexpr float LPIPS_SCALE[3] = {0.458f, 0.448f, 0.450f};
constexpr float LPIPS_NORM_EPS = 1e-8f;
constexpr int LPIPS_MIN_SIZE = 31;                              // the smallest image whose last map is 1 x 1
constexpr int LP_TAPS = 5;
constexpr int LP_CIN[LP_TAPS] = {3, 64, 192, 384, 256};
constexpr int LP_COUT[LP_TAPS] = {64, 192, 384, 256, 256};
constexpr int LP_KS[LP_TAPS] = {11, 5, 3, 3, 3};
constexpr int LP_STRIDE[LP_TAPS] = {4, 1, 1, 1, 1};
constexpr int LP_PAD[LP_TAPS] = {2, 2, 1, 1, 1};
constexpr bool LP_POOL_BEFORE[LP_TAPS] = {false, true, true, false, false};   // max-pool 3 / 2 (floor, no padding)

// the unit vector of a position's features is f * (1 / lpips_norm(sum_c f_c^2)) taken as f / lpips_norm(...): eps inside the root
// (the lpips package adds 1e-10 after it); an all-zero position gives 0
__device__ __forceinline__ float lpips_norm(float sumsq) { return sqrtf(LPIPS_NORM_EPS + sumsq); }

constexpr int BM = 128, BN = 128, BK = 32;   // the workgroup's tile
constexpr int LP_THREADS = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---- where a convolution reads its input ------------------------------------------------------------------------------------

// a channels-last map [2][Hi][Wi][C]
struct ActSrc {
  const float* x;
  int Hi, Wi, C;
  __device__ __forceinline__ float value(int img, int iy, int ix, int ci) const {
    return x[(((size_t)img * Hi + iy) * Wi + ix) * C + ci];
  }
};

// the two images (img 0: the prediction, 1: the ground truth), planar [3][H][W], as the scores see them, then scaled
struct ImgSrc {
  IidImages im;
  int H, W;
  __device__ __forceinline__ float value(int img, int iy, int ix, int ci) const {
    float s = 1.f, q = 1.f;
    if (im.map) { s = im.map->s; q = im.map->q; }
    const long long e = ((long long)ci * H + iy) * W + ix;
    const float v = im.valid(e) ? im.load_one(e, s, q, img) : 0.f;
    const float shift = ci == 0 ? LPIPS_SHIFT[0] : ci == 1 ? LPIPS_SHIFT[1] : LPIPS_SHIFT[2];
    const float scale = ci == 0 ? LPIPS_SCALE[0] : ci == 1 ? LPIPS_SCALE[1] : LPIPS_SCALE[2];
    return ((2.0f * v - 1.0f) - shift) / scale;
  }
};

// out[m][n] = relu(bias[n] + sum_k A[m][k] * wt[k][n]); A[m][k] = src at (image, oy * STRIDE - PAD + ky, ox * STRIDE - PAD + kx, ci),
// 0 outside the map; m = (image, oy, ox), k = (ky * KS + kx) * Cin + ci.  grid (ceil(M / BM), ceil(N / BN)).
// LDS: A tile [128][33] (the pad: a wave reads a column of 32 rows, row stride 33 words -> 32 different banks; the upper half of the
// wave reads the next column, 33 * d = 1 mod 64 only at d = 33: no conflict) + B tile [32][128] (a wave reads 32 consecutive words of
// two rows) + the rows' coordinates = 16 896 + 16 384 + 1 536 B.  Every global and LDS index is guarded by m < M, n < N, k < K and
// the map's bounds.
template <int KS, int STRIDE, int PAD, class Src>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_kernel(Src src, const float* __restrict__ wt, const float* __restrict__ bias,
                                                                float* __restrict__ out, int Hi, int Wi, int Cin, int Ho, int Wo, int N) {
  __shared__ float As[BM][BK + 1];
  __shared__ float Bs[BK][BN];
  __shared__ int r_img[BM], r_iy[BM], r_ix[BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = 2 * Ho * Wo, K = KS * KS * Cin;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  if (tid < BM) {
    const int m = m0 + tid;
    int img = 0, iy = -(1 << 28), ix = 0;   // a row past M: every tap is out of bounds
    if (m < M) {
      img = m / (Ho * Wo);
      const int r = m - img * (Ho * Wo), oy = r / Wo, ox = r - oy * Wo;
      iy = oy * STRIDE - PAD;
      ix = ox * STRIDE - PAD;
    }
    r_img[tid] = img;
    r_iy[tid] = iy;
    r_ix[tid] = ix;
  }
  __syncthreads();
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;   // the wave's 64 x 64 corner of the tile
  const bool wave_has_work = m0 + wm < M && n0 + wn < N;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += BK) {
    {   // A: thread = one k of the tile, 16 rows
      const int kk = tid & 31, k = k0 + kk;
      const bool kin = k < K;
      const int tap = kin ? k / Cin : 0, ci = kin ? k - tap * Cin : 0;
      const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll 4
      for (int j = 0; j < BM / 8; ++j) {
        const int r = (tid >> 5) + 8 * j;
        const int iy = r_iy[r] + ky, ix = r_ix[r] + kx;
        float v = 0.f;
        if (kin && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) v = src.value(r_img[r], iy, ix, ci);
        As[r][kk] = v;
      }
    }
    {   // B: thread = one column of the tile, 16 k
      const int n = tid & (BN - 1);
      const bool nin = n0 + n < N;
#pragma unroll 4
      for (int j = 0; j < BK / 2; ++j) {
        const int kk = (tid >> 7) + 2 * j, k = k0 + kk;
        Bs[kk][n] = (nin && k < K) ? wt[(size_t)k * N + n0 + n] : 0.f;
      }
    }
    __syncthreads();
    if (wave_has_work) {
#pragma unroll
      for (int kk = 0; kk < BK; kk += 2) {
        const int k = kk + (lane >> 5), c = lane & 31;   // lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
        const float a0 = As[wm + c][k], a1 = As[wm + 32 + c][k];
        const float b0 = Bs[k][wn + c], b1 = Bs[k][wn + 32 + c];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __syncthreads();   // the next K tile overwrites both tiles
  }
  if (!wave_has_work) return;
  // C / D of the 32 x 32 form: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 32 * j + (lane & 31);
    if (n >= N) continue;
    const float b = bias[n];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M) out[(size_t)m * N + n] = max_keep_nan(acc[i][j][r] + b, 0.f);   // torch.relu: a NaN stays
      }
  }
}

// (a NaN in the window stays, like torch's max_pool2d)
// y [2][Ho][Wo][C] = max over the 3 x 3 window at (2 oy, 2 ox) of x [2][Hi][Wi][C]; Ho = (Hi - 3) / 2 + 1, so 2 oy + 2 <= Hi - 1
__global__ __launch_bounds__(LP_THREADS) void lpips_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int Hi, int Wi, int C,
                                                                int Ho, int Wo) {
  const long long total = 2ll * Ho * Wo * C;
  for (long long idx = (long long)blockIdx.x * LP_THREADS + threadIdx.x; idx < total; idx += (long long)gridDim.x * LP_THREADS) {
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int ox = (int)(p % Wo);
    const long long t = p / Wo;
    const int oy = (int)(t % Ho), img = (int)(t / Ho);
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = max_keep_nan(m, x[(((size_t)img * Hi + 2 * oy + dy) * Wi + 2 * ox + dx) * C + c]);
    y[idx] = m;
  }
}

// valid elements of either image that are not within [0, 1] (a NaN is not) -> *count += their number
__global__ __launch_bounds__(EV_THREADS) void lpips_range_kernel(IidImages im, unsigned long long* __restrict__ count, long long N) {
  float s = 1.f, q = 1.f;
  if (im.map) { s = im.map->s; q = im.map->q; }
  unsigned bad = 0;
  for (long long e = (long long)blockIdx.x * EV_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * EV_THREADS) {
    if (!im.valid(e)) continue;
    float p, g;
    im.load(e, s, q, p, g);
    bad += !(p >= 0.f && p <= 1.f);
    bad += !(g >= 0.f && g <= 1.f);
  }
  bad = wave_sum_xor(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, (unsigned long long)bad);
}

// one tap: f [2][P][C] (the prediction's rows, then the ground truth's), lin [C] -> part[block] = the block's sum over its positions
// of sum_c lin_c * (fp_c / |fp| - fg_c / |fg|)^2.  A wave owns a position at a time (positions wave, wave + waves, ...: one order).
__global__ __launch_bounds__(LP_THREADS) void lpips_dist_kernel(const float* __restrict__ f, const float* __restrict__ lin,
                                                                double* __restrict__ part, int P, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[1] = {0.0};
  for (long long p = (long long)blockIdx.x * (LP_THREADS / 64) + wave; p < P; p += (long long)gridDim.x * (LP_THREADS / 64)) {
    const float* __restrict__ fp = f + (size_t)p * C;
    const float* __restrict__ fg = f + ((size_t)P + p) * C;
    float sp = 0.f, sg = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float a = fp[c], b = fg[c];
      sp += a * a;
      sg += b * b;
    }
    sp = wave_sum_xor(sp);
    sg = wave_sum_xor(sg);
    const float np = lpips_norm(sp), ng = lpips_norm(sg);
    float d = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float t = fp[c] / np - fg[c] / ng;
      d += lin[c] * (t * t);
    }
    acc[0] += (double)wave_sum_xor(d);
  }
  waves_sum_store<1, LP_THREADS>(acc, part + blockIdx.x);   // (acc is wave-uniform already: the waves' half of the block sum alone)
}

struct LpipsTail {
  int nblk[LP_TAPS];   // rows of each tap's partial table
  int P[LP_TAPS];      // positions of each tap
};

// the five tables in row order -> the terms (spatial means), their sum and the out-of-range count: out8 of mg_eval_iid_lpips
__global__ __launch_bounds__(64) void lpips_final_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ count,
                                                         double* __restrict__ out, LpipsTail t) {
  __shared__ double T[LP_TAPS];
  rows_sum<LP_TAPS>(part, threadIdx.x < LP_TAPS ? t.nblk[threadIdx.x] : 0, 1, EV_BLOCKS, T);   // [tap][EV_BLOCKS]: a tap is a column
  if (threadIdx.x != 0) return;
  for (int k = 0; k < LP_TAPS; ++k) T[k] = T[k] / (double)t.P[k];
  out[0] = (((T[0] + T[1]) + T[2]) + T[3]) + T[4];
  out[1] = (double)*count;
  for (int k = 0; k < LP_TAPS; ++k) out[2 + k] = T[k];
  out[7] = (double)__builtin_nanf("");
}

// ---- the call's plan: map sizes and the activation workspace's layout -------------------------------------------------------

constexpr size_t LP_ALIGN = 256;
size_t align_up(size_t b) { return (b + LP_ALIGN - 1) / LP_ALIGN * LP_ALIGN; }

struct LpipsPlan {
  int h[LP_TAPS], w[LP_TAPS];     // the taps' maps
  int hin[LP_TAPS], win[LP_TAPS];  // each convolution's input map
  size_t act[LP_TAPS];            // byte offsets: the taps, fp32 [2 * h * w][Cout]
  size_t pool[LP_TAPS];           // the pooled input of a layer with LP_POOL_BEFORE
  size_t part, count, total;      // f64 [LP_TAPS][EV_BLOCKS]; one u64
};

LpipsPlan lpips_plan(int H, int W) {
  LpipsPlan p;
  memset(&p, 0, sizeof(p));
  size_t off = 0;
  p.part = off;
  off = align_up(off + (size_t)LP_TAPS * EV_BLOCKS * 8);
  p.count = off;
  off = align_up(off + 8);
  int hi = H, wi = W;
  for (int l = 0; l < LP_TAPS; ++l) {
    if (LP_POOL_BEFORE[l]) {
      hi = (hi - 3) / 2 + 1;
      wi = (wi - 3) / 2 + 1;
      p.pool[l] = off;
      off = align_up(off + 2 * (size_t)hi * wi * LP_CIN[l] * 4);
    }
    p.hin[l] = hi;
    p.win[l] = wi;
    hi = (hi + 2 * LP_PAD[l] - LP_KS[l]) / LP_STRIDE[l] + 1;
    wi = (wi + 2 * LP_PAD[l] - LP_KS[l]) / LP_STRIDE[l] + 1;
    p.h[l] = hi;
    p.w[l] = wi;
    p.act[l] = off;
    off = align_up(off + 2 * (size_t)hi * wi * LP_COUT[l] * 4);
  }
  p.total = off;
  return p;
}

bool lpips_size_ok(int H, int W) { return H >= LPIPS_MIN_SIZE && W >= LPIPS_MIN_SIZE && 3ll * H * W < (1ll << 31); }

template <int KS, int STRIDE, int PAD, class Src>
void launch_conv(const Src& src, const float* wt, const float* bias, float* out, const LpipsPlan& p, int l, hipStream_t s) {
  const int M = 2 * p.h[l] * p.w[l], N = LP_COUT[l];
  MG_LAUNCH((lpips_conv_kernel<KS, STRIDE, PAD, Src>), dim3((M + BM - 1) / BM, (N + BN - 1) / BN), dim3(LP_THREADS), 0, s, src, wt, bias,
            out, p.hin[l], p.win[l], LP_CIN[l], p.h[l], p.w[l], N);
}

}  // namespace

extern "C" {

long long mg_lpips_workspace_bytes(int H, int W) {
  if (!lpips_size_ok(H, W)) {
    mg_set_error("mg_lpips_workspace_bytes: H, W >= %d and 3 H W < 2^31 required, got %d x %d", LPIPS_MIN_SIZE, H, W);
    return -1;
  }
  return (long long)lpips_plan(H, W).total;
}

int mg_eval_iid_lpips(const mg_lpips_net* net, const float* pred, const float* gt, const uint8_t* mask_or_null, int H, int W,
                      int up_to_scale, int gamma_mode, double* out8, void* eval_ws, void* act_ws, long long act_ws_bytes, void* stream) {
  MG_REQUIRE(net && pred && gt && out8 && eval_ws && act_ws, "mg_eval_iid_lpips: null pointer");
  for (int l = 0; l < LP_TAPS; ++l) {
    MG_REQUIRE(net->conv_w[l] && net->conv_b[l] && net->lin_w[l], "mg_eval_iid_lpips: null pointer in the network (layer %d)", l);
    MG_REQUIRE(((uintptr_t)net->conv_w[l] | (uintptr_t)net->conv_b[l] | (uintptr_t)net->lin_w[l]) % 4 == 0,
               "mg_eval_iid_lpips: network weights not 4-byte aligned (layer %d)", l);
  }
  MG_REQUIRE(lpips_size_ok(H, W), "mg_eval_iid_lpips: H, W >= %d required (the last feature map must be at least 1 x 1) and 3 H W < 2^31, got %d x %d",
             LPIPS_MIN_SIZE, H, W);
  MG_REQUIRE(gamma_mode >= MG_IID_GAMMA_NONE && gamma_mode <= MG_IID_GAMMA_BOTH, "mg_eval_iid_lpips: unknown gamma mode %d", gamma_mode);
  MG_REQUIRE(((uintptr_t)pred | (uintptr_t)gt) % 4 == 0, "mg_eval_iid_lpips: pred / gt not 4-byte aligned");
  MG_REQUIRE(((uintptr_t)out8 | (uintptr_t)eval_ws) % 8 == 0, "mg_eval_iid_lpips: out / workspace not 8-byte aligned");
  MG_REQUIRE((uintptr_t)act_ws % 16 == 0, "mg_eval_iid_lpips: activation workspace not 16-byte aligned");
  const LpipsPlan plan = lpips_plan(H, W);
  MG_REQUIRE(act_ws_bytes >= (long long)plan.total, "mg_eval_iid_lpips: activation workspace too small: %lld bytes, %d x %d needs %lld",
             act_ws_bytes, H, W, (long long)plan.total);
  hipStream_t s = (hipStream_t)stream;
  char* const ws = (char*)act_ws;
  if (up_to_scale) {   // (s, q) into the evaluation workspace: bit-reproducible, so they are those of mg_eval_iid
    mg_op op;
    memset(&op, 0, sizeof(op));
    op.kind = MG_OP_IIDSCORE_PREP;
    op.p[MG_IIDSCORE_PREP_P_PRED] = (void*)pred;
    op.p[MG_IIDSCORE_PREP_P_GT] = (void*)gt;
    op.p[MG_IIDSCORE_PREP_P_MASK] = (void*)mask_or_null;
    op.p[MG_IIDSCORE_PREP_P_OUT] = out8;   // PREP's slots are overwritten by the last kernel below
    op.p[MG_IIDSCORE_PREP_P_WS] = eval_ws;
    op.i[MG_IIDSCORE_PREP_I_H] = H;
    op.i[MG_IIDSCORE_PREP_I_W] = W;
    op.i[MG_IIDSCORE_PREP_I_GAMMA] = gamma_mode;
    if (const int rc = mg_launch_evalscore(&op, s)) return rc;
  }
  const IidImages im{pred, gt, mask_or_null, up_to_scale ? (const IidMap*)((char*)eval_ws + WS_II_MAP) : nullptr, gamma_mode};
  unsigned long long* const count = (unsigned long long*)(ws + plan.count);
  double* const part = (double*)(ws + plan.part);
  if (!g_dry_run) MG_CHECK_HIP(hipMemsetAsync(count, 0, 8, s));
  const long long N3 = 3ll * H * W;
  MG_LAUNCH(lpips_range_kernel, dim3((int)max(1ll, min((N3 + EV_THREADS - 1) / EV_THREADS, (long long)EV_BLOCKS))), dim3(EV_THREADS), 0, s,
            im, count, N3);
  LpipsTail tail;
  for (int l = 0; l < LP_TAPS; ++l) {
    float* const out = (float*)(ws + plan.act[l]);
    const float* in = l ? (const float*)(ws + plan.act[l - 1]) : nullptr;
    if (LP_POOL_BEFORE[l]) {
      float* const pooled = (float*)(ws + plan.pool[l]);
      const long long total = 2ll * plan.hin[l] * plan.win[l] * LP_CIN[l];
      MG_LAUNCH(lpips_pool_kernel, dim3((int)min((total + LP_THREADS - 1) / LP_THREADS, 4096ll)), dim3(LP_THREADS), 0, s, in, pooled,
                plan.h[l - 1], plan.w[l - 1], LP_CIN[l], plan.hin[l], plan.win[l]);
      in = pooled;
    }
    const ActSrc act{in, plan.hin[l], plan.win[l], LP_CIN[l]};
    static_assert(LP_KS[0] == 11 && LP_STRIDE[0] == 4 && LP_PAD[0] == 2 && LP_KS[1] == 5 && LP_STRIDE[1] == 1 && LP_PAD[1] == 2, "conv1 / conv2");
    static_assert(LP_KS[2] == 3 && LP_KS[3] == 3 && LP_KS[4] == 3 && LP_STRIDE[4] == 1 && LP_PAD[2] == 1 && LP_PAD[4] == 1, "conv3-5");
    switch (l) {
      case 0: launch_conv<11, 4, 2>(ImgSrc{im, H, W}, net->conv_w[l], net->conv_b[l], out, plan, l, s); break;
      case 1: launch_conv<5, 1, 2>(act, net->conv_w[l], net->conv_b[l], out, plan, l, s); break;
      default: launch_conv<3, 1, 1>(act, net->conv_w[l], net->conv_b[l], out, plan, l, s); break;
    }
    const int P = plan.h[l] * plan.w[l];
    tail.P[l] = P;
    tail.nblk[l] = min((P + LP_THREADS / 64 - 1) / (LP_THREADS / 64), EV_BLOCKS);
    MG_LAUNCH(lpips_dist_kernel, dim3(tail.nblk[l]), dim3(LP_THREADS), 0, s, (const float*)out, net->lin_w[l], part + (size_t)l * EV_BLOCKS,
              P, LP_COUT[l]);
  }
  MG_LAUNCH(lpips_final_kernel, dim3(1), dim3(64), 0, s, (const double*)part, (const unsigned long long*)count, out8, tail);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
