// On-device scoring of one prediction against its ground truth: the per-image body of the reference's validation loop
// (src/trainer/marigold_depth_trainer.py:510-601) and of script/{depth,normals}/eval.py - least-squares alignment
// (src/util/alignment.py:35-82), the clips of script/depth/eval.py:176-212, the ten depth scores (src/util/metric.py:64-199) and the
// angular-error statistics of the normals protocol (:206-279).
//
// Element arithmetic is fp32 with IEEE division, sqrt and the library's accurate logf / log10f / acosf (this file is built with
// -ffp-contract=off and no fast-math, so an expression rounds like the numpy / torch element ops it restates); every sum is fp64.
// Reductions: thread -> wave -> block -> one row of a per-block partial table; a one-block launch then adds the rows.  The order of
// every step is reduce.h's.  No floating-point atomics: two launches on the same input give the same bits.
// The median of the angles is exact: they are non-negative, so their bit patterns order as unsigned integers, and three histogram
// passes over 11 / 11 / 10 bits (integer atomics in LDS, merged into a global histogram) select the two middle order statistics.
// The same selection finds the brightness quantile of the intrinsic-image scores (compute_iid_metric, src/util/metric.py:263-338;
// PSNR and a tiled fp64 SSIM) in the last part of this file.
//
// The maps are 0.3-0.6 M pixels: every kernel here is a few microseconds of streaming, the cost of a call is its launches.
#include <math.h>
#include <string.h>

#include "common.h"
#include "iid_images.h"   // EV_BLOCKS, EV_THREADS, IidMap, iid_gamma, IidImages and the head of the IID workspace layout
#include "reduce.h"

namespace {

constexpr int LS_N = 5;           // n, Sx, Sy, Sxx, Sxy
constexpr int DM_N = 11;          // the eleven sums of the depth scores (below)
constexpr int NM_N = 9;           // Se, See, five counts, n, NaN count

// workspace layout of mg_eval_depth / MG_OP_EVAL_NORMALS (bytes)
constexpr size_t WS_LS_PART = 0;
constexpr size_t WS_LS_SUMS = WS_LS_PART + (size_t)EV_BLOCKS * LS_N * 8;
constexpr size_t WS_DM_PART = WS_LS_SUMS + 64;
constexpr size_t WS_DEPTH_END = WS_DM_PART + (size_t)EV_BLOCKS * DM_N * 8;
constexpr size_t WS_NM_PART = 0;
constexpr size_t WS_NM_STATE = WS_NM_PART + (size_t)EV_BLOCKS * NM_N * 8;
constexpr size_t WS_NM_HIST0 = WS_NM_STATE + 64;              // [2048]       bits 31..21
constexpr size_t WS_NM_HIST1 = WS_NM_HIST0 + 2048 * 4;        // [2][2048]    bits 20..10 under each rank's prefix
constexpr size_t WS_NM_HIST2 = WS_NM_HIST1 + 2 * 2048 * 4;    // [2][1024]    bits 9..0
constexpr size_t WS_NORMALS_END = WS_NM_HIST2 + 2 * 1024 * 4;
static_assert(WS_DEPTH_END <= MG_EVAL_WS_BYTES && WS_NORMALS_END <= MG_EVAL_WS_BYTES, "MG_EVAL_WS_BYTES too small");

// the selection's state between the passes: per rank (lower / upper middle) the bits fixed so far and the rank inside them
struct SelState {
  unsigned prefix[2];
  unsigned long long rem[2];
  unsigned long long n, nan;
};
static_assert(sizeof(SelState) <= 64, "SelState");

// rows [0, nblk) of a partial table added in row order -> out[N]; one block
__global__ __launch_bounds__(64) void sum_rows_kernel(const double* __restrict__ part, double* __restrict__ out, int nblk, int N) {
  const int k = threadIdx.x;
  if (k < N) out[k] = column_sum(part + k, nblk, N);
}

// ---- depth ----------------------------------------------------------------------------------------------------------

// alignment._nearest_downscale / torch.nn.Upsample(mode="nearest") on a [1, H, W] tensor: the width alone is sub-sampled
__device__ __forceinline__ int fit_pixel(int idx, int W, int OW, float inv) {
  if (OW <= 0) return idx;
  const int row = idx / OW, col = idx - row * OW;
  const int sc = (int)fminf(floorf((float)col * inv), (float)(W - 1));
  return row * W + sc;
}

__global__ __launch_bounds__(EV_THREADS) void depth_ls_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                              const uint8_t* __restrict__ mask, double* __restrict__ part,
                                                              int H, int W, int OW, float inv, int disparity) {
  double acc[LS_N];
#pragma unroll
  for (int k = 0; k < LS_N; ++k) acc[k] = 0.0;
  const int total = H * (OW > 0 ? OW : W);
  for (int idx = blockIdx.x * EV_THREADS + threadIdx.x; idx < total; idx += gridDim.x * EV_THREADS) {
    const int src = fit_pixel(idx, W, OW, inv);
    if (!mask[src]) continue;
    const float p = pred[src], g = gt[src];
    float y = g;
    if (disparity) {
      if (!(g > 0.f && p > 0.f)) continue;
      y = 1.0f / g;
    }
    const double x = (double)p, yd = (double)y;
    acc[0] += 1.0;
    acc[1] += x;
    acc[2] += yd;
    acc[3] += x * x;
    acc[4] += x * yd;
  }
  block_sum_store<LS_N, EV_THREADS>(acc, part + (size_t)blockIdx.x * LS_N);
}

// scale, shift of the 2 x 2 normal equations (evaluation/alignment.py), cast to fp32 like the fit of fp32 arrays
__device__ __forceinline__ void ls_solve(const double* __restrict__ sums, float& s, float& t) {
  if (!sums) { s = 1.f; t = 0.f; return; }
  const scale_shift f = scale_shift_solve(sums[0], sums[1], sums[2], sums[3], sums[4]);   // unguarded, like the host's
  s = (float)f.s;
  t = (float)f.t;
}

// sums: 0 |a-g|/g  1 (a-g)^2/g  2 (a-g)^2  3 (ln a - ln g)^2  4 ln a - ln g  5 |log10 a - log10 g|  6..8 max(a/g, g/a) < 1.25^k
// 9 (1/a - 1/g)^2  10 n
__global__ __launch_bounds__(EV_THREADS) void depth_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                   const uint8_t* __restrict__ mask, const double* __restrict__ sums,
                                                                   double* __restrict__ part, int HW, int disparity, int has_lo,
                                                                   int has_hi, float lo, float hi) {
  float s, t;
  ls_solve(sums, s, t);
  const bool aligned = sums != nullptr;
  double acc[DM_N];
#pragma unroll
  for (int k = 0; k < DM_N; ++k) acc[k] = 0.0;
  for (int idx = blockIdx.x * EV_THREADS + threadIdx.x; idx < HW; idx += gridDim.x * EV_THREADS) {
    if (!mask[idx]) continue;
    const float g = gt[idx];
    float a = pred[idx];
    if (aligned) {
      a = a * s + t;
      if (disparity) {   // np.clip(disp, 1e-3, None), then disparity2depth: 1 / d where d > 0, else 0
        a = floor_keep_nan(a, 1e-3f);
        a = a > 0.f ? 1.0f / a : 0.f;
      }
    }
    if (has_lo) a = floor_keep_nan(a, lo);
    if (has_hi) a = a != a ? a : fminf(a, hi);
    a = floor_keep_nan(a, 1e-6f);
    const float d = a - g, ad = fabsf(d);
    const float ld = logf(a) - logf(g);
    const float worst = max_keep_nan(a / g, g / a);
    const float id = 1.0f / a - 1.0f / g;
    acc[0] += (double)(ad / g);
    acc[1] += (double)((ad * ad) / g);
    acc[2] += (double)(d * d);
    acc[3] += (double)(ld * ld);
    acc[4] += (double)ld;
    acc[5] += (double)fabsf(log10f(a) - log10f(g));
    acc[6] += worst < 1.25f ? 1.0 : 0.0;
    acc[7] += worst < 1.5625f ? 1.0 : 0.0;
    acc[8] += worst < 1.953125f ? 1.0 : 0.0;
    acc[9] += (double)(id * id);
    acc[10] += 1.0;
  }
  block_sum_store<DM_N, EV_THREADS>(acc, part + (size_t)blockIdx.x * DM_N);
}

__global__ __launch_bounds__(64) void depth_metrics_final_kernel(const double* __restrict__ part, const double* __restrict__ sums,
                                                                 double* __restrict__ out, int nblk) {
  __shared__ double S[DM_N];
  rows_sum<DM_N>(part, nblk, DM_N, 1, S);
  if (threadIdx.x != 0) return;
  const double n = S[10];
  float s, t;
  ls_solve(sums, s, t);
  const double mlog = S[4] / n;
  out[0] = S[0] / n;
  out[1] = S[1] / n;
  out[2] = sqrt(S[2] / n);
  out[3] = sqrt(S[3] / n);
  out[4] = S[5] / n;
  out[5] = S[6] / n;
  out[6] = S[7] / n;
  out[7] = S[8] / n;
  out[8] = sqrt(S[9] / n);
  out[9] = sqrt(S[3] / n - mlog * mlog) * 100.0;
  out[10] = (double)s;
  out[11] = (double)t;
  out[12] = n;
}

// ---- normals --------------------------------------------------------------------------------------------------------

// metrics.compute_cosine_error for pixel i; false = the pixel is dropped (masked and a ground-truth vector of zero norm)
__device__ __forceinline__ bool normals_angle(const float* __restrict__ pred, const float* __restrict__ gt, long long HW, long long i,
                                              int masked, float& e) {
  const float gx = gt[i], gy = gt[HW + i], gz = gt[2 * HW + i];
  float gn = sqrtf((gx * gx + gy * gy) + gz * gz);
  if (masked && !(gn > 0.f)) return false;
  const float px = pred[i], py = pred[HW + i], pz = pred[2 * HW + i];
  const float pn = max_keep_nan(sqrtf((px * px + py * py) + pz * pz), 1e-8f);
  gn = max_keep_nan(gn, 1e-8f);
  float c = ((px / pn) * (gx / gn) + (py / pn) * (gy / gn)) + (pz / pn) * (gz / gn);
  c = clip_keep_nan(c, -1.0f, 1.0f);
  e = acosf(c) * 57.29577951308232f;
  return true;
}

// the angle of pixel i for the selection passes: from the error map when the caller gave one, else recomputed (the same code, the
// same bits)
__device__ __forceinline__ bool angle_of(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ err,
                                         long long HW, long long i, int masked, float& e) {
  if (err) {
    e = err[i];
    return !(e == -1.0f);
  }
  return normals_angle(pred, gt, HW, i, masked, e);
}

__global__ __launch_bounds__(EV_THREADS) void normals_stats_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                   float* __restrict__ err, double* __restrict__ part,
                                                                   unsigned* __restrict__ ghist, long long HW, int masked) {
  __shared__ unsigned hist[2048];
  for (int b = threadIdx.x; b < 2048; b += EV_THREADS) hist[b] = 0u;
  __syncthreads();
  double acc[NM_N];
#pragma unroll
  for (int k = 0; k < NM_N; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < HW; i += (long long)gridDim.x * EV_THREADS) {
    float e;
    const bool keep = normals_angle(pred, gt, HW, i, masked, e);
    if (err) err[i] = keep ? e : -1.0f;
    if (!keep) continue;
    acc[0] += (double)e;
    acc[1] += (double)(e * e);
    acc[2] += e < 5.0f ? 1.0 : 0.0;
    acc[3] += e < 7.5f ? 1.0 : 0.0;
    acc[4] += e < 11.25f ? 1.0 : 0.0;
    acc[5] += e < 22.5f ? 1.0 : 0.0;
    acc[6] += e < 30.0f ? 1.0 : 0.0;
    acc[7] += 1.0;
    acc[8] += e != e ? 1.0 : 0.0;
    atomicAdd(&hist[__float_as_uint(e) >> 21], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 2048; b += EV_THREADS)
    if (hist[b]) atomicAdd(&ghist[b], hist[b]);
  block_sum_store<NM_N, EV_THREADS>(acc, part + (size_t)blockIdx.x * NM_N);
}

// the bin that holds rank st->rem[r] of a histogram, for both ranks (lane 0 of waves 0 and 1); the bin joins the prefix
__device__ __forceinline__ void select_bin(SelState* __restrict__ st, const unsigned* __restrict__ hist, int bins, int stride, int bits) {
  const int r = threadIdx.x >> 6;
  if ((threadIdx.x & 63) != 0 || r >= 2) return;
  const unsigned* __restrict__ h = hist + (size_t)r * stride;
  unsigned long long rem = st->rem[r];
  int b = 0;
  for (; b < bins - 1; ++b) {
    const unsigned long long c = h[b];
    if (rem < c) break;
    rem -= c;
  }
  st->prefix[r] = (st->prefix[r] << bits) | (unsigned)b;
  st->rem[r] = rem;
}

// one block: the table's rows in order -> every output but the median; the ranks of the two middle angles; the first selection step
__global__ __launch_bounds__(128) void normals_reduce_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                             SelState* __restrict__ st, const unsigned* __restrict__ hist0, int nblk) {
  __shared__ double S[NM_N];
  rows_sum<NM_N>(part, nblk, NM_N, 1, S);
  if (threadIdx.x == 0) {
    const double n = S[7];
    out[0] = S[0] / n;
    for (int k = 0; k < 5; ++k) out[2 + k] = 100.0 * (S[2 + k] / n);
    out[7] = sqrt(S[1] / n);
    out[8] = n;
    const unsigned long long cnt = (unsigned long long)n;
    st->n = cnt;
    st->nan = (unsigned long long)S[8];
    st->prefix[0] = st->prefix[1] = 0u;
    st->rem[0] = cnt ? (cnt - 1) / 2 : 0;
    st->rem[1] = cnt / 2;
  }
  __syncthreads();
  select_bin(st, hist0, 2048, 0, 11);
}

// the values a selection runs over, as unsigned keys that order like the values: the angles of the normals protocol (non-negative,
// so their bit patterns order as they stand); the IID brightness is IidBrightness below
struct NormalsAngles {
  const float *pred, *gt, *err;
  long long HW;
  int masked;
  __device__ __forceinline__ bool key(long long i, unsigned& u) const {
    float e;
    if (!angle_of(pred, gt, err, HW, i, masked, e)) return false;
    u = __float_as_uint(e);
    return true;
  }
};

// passes 2 and 3: the histogram of the next `bits` bits of the keys that carry a rank's prefix; ghist [2][1 << bits]
template <class Src>
__global__ __launch_bounds__(EV_THREADS) void select_hist_kernel(Src src, const SelState* __restrict__ st, unsigned* __restrict__ ghist,
                                                                 long long N, int shift, int bits) {
  __shared__ unsigned hist[2 * 2048];
  const int bins = 1 << bits;
  for (int b = threadIdx.x; b < 2 * bins; b += EV_THREADS) hist[b] = 0u;
  __syncthreads();
  const unsigned p0 = st->prefix[0], p1 = st->prefix[1];
  for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * EV_THREADS) {
    unsigned u;
    if (!src.key(i, u)) continue;
    const unsigned hi = u >> (shift + bits), bin = (u >> shift) & (unsigned)(bins - 1);
    if (hi == p0) atomicAdd(&hist[bin], 1u);
    if (hi == p1) atomicAdd(&hist[bins + bin], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 2 * bins; b += EV_THREADS)
    if (hist[b]) atomicAdd(&ghist[b], hist[b]);
}

__global__ __launch_bounds__(128) void select_step_kernel(SelState* __restrict__ st, const unsigned* __restrict__ hist, int bins,
                                                             int bits, double* __restrict__ out_median) {
  select_bin(st, hist, bins, bins, bits);
  if (!out_median) return;
  __syncthreads();
  if (threadIdx.x != 0) return;
  // np.median: the mean of the two middle order statistics, in the array's own fp32 (odd n: both ranks are the same element)
  const float lo = __uint_as_float(st->prefix[0]), hi = __uint_as_float(st->prefix[1]);
  const float med = (lo + hi) / 2.0f;
  *out_median = (st->n == 0 || st->nan != 0) ? (double)__builtin_nanf("") : (double)med;
}

// ---- intrinsic image decomposition ----------------------------------------------------------------------------------

constexpr int SS_T = 32;          // the SSIM kernel's output tile is SS_T x SS_T
constexpr int SS_R = 5;           // radius of the 11-tap window
constexpr int SS_K = 2 * SS_R + 1;
constexpr int SS_S = SS_T + 2 * SS_R;   // the staged tile: output tile + halo

// workspace layout of the MG_OP_IIDSCORE_* ops (bytes), after the head in iid_images.h
constexpr size_t WS_II_HIST0 = WS_II_MAP + 64;
constexpr size_t WS_II_HIST1 = WS_II_HIST0 + 2048 * 4;
constexpr size_t WS_II_HIST2 = WS_II_HIST1 + 2 * 2048 * 4;
constexpr size_t WS_II_PSNR_PART = WS_II_HIST2 + 2 * 1024 * 4;
constexpr size_t WS_II_SSIM_PART = WS_II_PSNR_PART + (size_t)EV_BLOCKS * 2 * 8;
constexpr size_t WS_IID_END = WS_II_SSIM_PART + (size_t)EV_BLOCKS * 2 * 8;
static_assert(WS_IID_END <= MG_EVAL_WS_BYTES, "MG_EVAL_WS_BYTES too small");

// brightness of the ground truth over the pixels of mask channel 0 (quantile_map, metric.py:337-375).  Its sign is not known, so
// the key flips the pattern into an order-preserving one: negative values complemented, the others with the sign bit set.
struct IidBrightness {
  const float* gt;
  const uint8_t* mask;
  long long HW;
  int gamma;
  __device__ __forceinline__ bool value(long long i, float& b) const {
    if (mask && !mask[i]) return false;
    const float g0 = iid_gamma(gt[i], gamma), g1 = iid_gamma(gt[HW + i], gamma), g2 = iid_gamma(gt[2 * HW + i], gamma);
    b = (0.3f * g0 + 0.59f * g1) + 0.11f * g2;
    return true;
  }
  static __device__ __forceinline__ unsigned to_key(float b) {
    const unsigned u = __float_as_uint(b);
    return (u >> 31) ? ~u : (u | 0x80000000u);
  }
  static __device__ __forceinline__ float from_key(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
  __device__ __forceinline__ bool key(long long i, unsigned& u) const {
    float b;
    if (!value(i, b)) return false;
    u = to_key(b);
    return true;
  }
};

// the sums of compute_alignment_scale (metric.py:319-334) over the valid elements and the first histogram of the brightness
__global__ __launch_bounds__(EV_THREADS) void iid_prep_kernel(IidImages im, IidBrightness br, double* __restrict__ part,
                                                              unsigned* __restrict__ ghist, long long HW) {
  __shared__ unsigned hist[2048];
  for (int b = threadIdx.x; b < 2048; b += EV_THREADS) hist[b] = 0u;
  __syncthreads();
  double acc[II_N];
#pragma unroll
  for (int k = 0; k < II_N; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < HW; i += (long long)gridDim.x * EV_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long e = c * HW + i;
      if (!im.valid(e)) continue;
      const double p = (double)iid_gamma(im.pred[e], im.gamma), g = (double)iid_gamma(im.gt[e], im.gamma);
      acc[0] += p * g;
      acc[1] += p * p;
      acc[2] += 1.0;
    }
    float b;
    if (!br.value(i, b)) continue;
    acc[3] += 1.0;
    acc[4] += b != b ? 1.0 : 0.0;
    atomicAdd(&hist[IidBrightness::to_key(b) >> 21], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 2048; b += EV_THREADS)
    if (hist[b]) atomicAdd(&ghist[b], hist[b]);
  block_sum_store<II_N, EV_THREADS>(acc, part + (size_t)blockIdx.x * II_N);
}

// one block: the alignment scale; the ranks of the two order statistics around 0.9 (n - 1); the first selection step.
// The position is np.quantile's / torch.quantile's on fp32 input: (n - 1) * 0.9 evaluated in fp32.
__global__ __launch_bounds__(128) void iid_prep_reduce_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                              SelState* __restrict__ st, IidMap* __restrict__ map,
                                                              const unsigned* __restrict__ hist0, int nblk) {
  __shared__ double S[II_N];
  rows_sum<II_N>(part, nblk, II_N, 1, S);
  if (threadIdx.x == 0) {
    const double s = S[0] / S[1];
    out[2] = s;
    map->s = (float)s;
    const unsigned long long cnt = (unsigned long long)S[3];
    st->n = cnt;
    st->nan = (unsigned long long)S[4];
    st->prefix[0] = st->prefix[1] = 0u;
    unsigned long long lo = 0, hi = 0;
    if (cnt) {
      const float v = (float)(cnt - 1) * 0.9f;
      lo = (unsigned long long)floorf(v);
      hi = lo + 1;
      if (lo >= cnt - 1) lo = hi = cnt - 1;
    }
    st->rem[0] = lo;
    st->rem[1] = hi;
  }
  __syncthreads();
  select_bin(st, hist0, 2048, 0, 11);
}

// the last selection step, then numpy's _lerp between the two order statistics in fp32 and the scale of quantile_map
__global__ __launch_bounds__(128) void iid_quantile_kernel(SelState* __restrict__ st, const unsigned* __restrict__ hist,
                                                           IidMap* __restrict__ map, double* __restrict__ out) {
  select_bin(st, hist, 1024, 1024, 10);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float a = IidBrightness::from_key(st->prefix[0]), b = IidBrightness::from_key(st->prefix[1]);
  float q = __builtin_nanf(""), lo = q, hi = q;
  if (st->n != 0 && st->nan == 0) {
    const float v = (float)(st->n - 1) * 0.9f;
    const float t = v - floorf(v);   // (both ranks the last element: a == b, whatever t)
    const float d = b - a;
    q = t >= 0.5f ? b - d * (1.0f - t) : a + d * t;
    lo = a;
    hi = b;
  }
  const float scale = (double)q < 1e-4 ? 0.f : (float)(0.8 / (double)q);   // (the host compares and divides q as a Python float)
  map->q = scale;
  out[3] = (double)q;
  out[4] = (double)scale;
  out[6] = (double)lo;
  out[7] = (double)hi;
}

// squared error over the valid elements (metrics.psnr: the difference of the fp32 images is taken in fp64)
__global__ __launch_bounds__(EV_THREADS) void iid_psnr_kernel(IidImages im, double* __restrict__ part, long long N) {
  float s = 1.f, q = 1.f;
  if (im.map) { s = im.map->s; q = im.map->q; }
  double acc[2] = {0.0, 0.0};
  for (long long e = (long long)blockIdx.x * EV_THREADS + threadIdx.x; e < N; e += (long long)gridDim.x * EV_THREADS) {
    if (!im.valid(e)) continue;
    float p, g;
    im.load(e, s, q, p, g);
    const double d = (double)p - (double)g;
    acc[0] += d * d;
    acc[1] += 1.0;
  }
  block_sum_store<2, EV_THREADS>(acc, part + (size_t)blockIdx.x * 2);
}

__global__ __launch_bounds__(64) void iid_psnr_final_kernel(const double* __restrict__ part, double* __restrict__ out, int nblk,
                                                            int mapped, int want_psnr) {
  __shared__ double S[2];
  rows_sum<2>(part, nblk, 2, 1, S);
  if (threadIdx.x != 0) return;
  const double n = S[1];
  if (want_psnr) out[0] = 10.0 * log10(1.0 / (S[0] / n));   // identical images: 1 / 0 = +inf, like the host; n = 0: NaN
  out[5] = n;
  if (!mapped) out[2] = out[4] = n > 0.0 ? 1.0 : (double)__builtin_nanf("");
}

struct SsimWindow {
  double w[SS_K];
};

// SSIM (metrics.ssim: 11 x 11 Gaussian window, sigma 1.5, reflect padding, the padded border cropped - so no kept value ever sees
// a padded pixel and the kept values are those of image rows / columns [5, H - 5) x [5, W - 5)).  One workgroup owns a 32 x 32 tile
// of kept values of one channel at a time (tiles blockIdx.x, blockIdx.x + gridDim.x, ... in that order, so a block's sum has one
// order).  Per tile: the 42 x 42 patch (tile + halo of 5) of both images goes to LDS once, masked / mapped / gamma'd in staging;
// the five moments x, y, xx, yy, xy - exact fp64 products of the fp32 values - are blurred along the rows into an fp64 LDS
// intermediate [5][42][32] and then along the columns out of it; the per-pixel SSIM is formed in fp64 and summed.
// fp64 throughout: sigma = E[x^2] - mu^2 cancels against c2 = 9e-4, and the host function is fp64.
// LDS per workgroup: 2 x 42 x 42 x 4 = 14 112 B patches + 5 x 42 x 32 x 8 = 53 760 B intermediate + 64 B of the block sum = 67 936 B
// of the CU's 160 KiB (163 840 B): 2 workgroups = 8 waves per CU, 2 per SIMD (130 VGPRs would allow 3: LDS is the limit).  Row pass: a wave reads 32 consecutive floats of two
// patch rows (ds_read_b32, the halves of the wave on different rows: no conflict); column pass: 32 consecutive doubles of one
// intermediate row per half wave (ds_read_b64, one 256 B bank row: no conflict).
__global__ __launch_bounds__(EV_THREADS) void iid_ssim_kernel(IidImages im, SsimWindow win, double* __restrict__ part, int H, int W,
                                                              int nty, int ntx) {
  __shared__ float sx[SS_S][SS_S], sy[SS_S][SS_S];
  __shared__ double rows[5][SS_S][SS_T];
  float s = 1.f, q = 1.f;
  if (im.map) { s = im.map->s; q = im.map->q; }
  const long long HW = (long long)H * W;
  const int OH = H - 2 * SS_R, OW = W - 2 * SS_R;
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  double acc[2] = {0.0, 0.0};   // the SSIM values; the valid elements staged (> 0: there is something to score)
  for (int t = blockIdx.x; t < 3 * nty * ntx; t += gridDim.x) {
    const int c = t / (nty * ntx), ty = (t / ntx) % nty, tx = t % ntx;
    const int y0 = ty * SS_T, x0 = tx * SS_T;   // the patch's origin in the image = the tile's origin among the kept values
    for (int idx = threadIdx.x; idx < SS_S * SS_S; idx += EV_THREADS) {
      const int r = idx / SS_S, cc = idx - r * SS_S;
      const int iy = y0 + r, ix = x0 + cc;
      float p = 0.f, g = 0.f;
      if (iy < H && ix < W) {
        const long long e = c * HW + (long long)iy * W + ix;
        if (im.valid(e)) {
          im.load(e, s, q, p, g);
          acc[1] += 1.0;
        }
      }
      sx[r][cc] = p;
      sy[r][cc] = g;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < SS_S * SS_T; idx += EV_THREADS) {
      const int r = idx / SS_T, cc = idx - r * SS_T;
      double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
      for (int k = 0; k < SS_K; ++k) {
        const double x = (double)sx[r][cc + k], y = (double)sy[r][cc + k], w = win.w[k];
        mx = fma(w, x, mx);
        my = fma(w, y, my);
        mxx = fma(w, x * x, mxx);
        myy = fma(w, y * y, myy);
        mxy = fma(w, x * y, mxy);
      }
      rows[0][r][cc] = mx;
      rows[1][r][cc] = my;
      rows[2][r][cc] = mxx;
      rows[3][r][cc] = myy;
      rows[4][r][cc] = mxy;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < SS_T * SS_T; idx += EV_THREADS) {
      const int r = idx / SS_T, cc = idx - r * SS_T;
      if (y0 + r >= OH || x0 + cc >= OW) continue;
      double m[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < SS_K; ++k) v = fma(win.w[k], rows[j][r + k][cc], v);
        m[j] = v;
      }
      const double mx = m[0], my = m[1];
      const double sxx = m[2] - mx * mx, syy = m[3] - my * my, sxy = m[4] - mx * my;
      acc[0] += ((2.0 * mx * my + c1) * (2.0 * sxy + c2)) / (((mx * mx + my * my) + c1) * ((sxx + syy) + c2));
    }
    __syncthreads();   // the next tile overwrites the patches and the intermediate
  }
  block_sum_store<2, EV_THREADS>(acc, part + (size_t)blockIdx.x * 2);
}

__global__ __launch_bounds__(64) void iid_ssim_final_kernel(const double* __restrict__ part, double* __restrict__ out, int nblk,
                                                            double count) {
  __shared__ double S[2];
  rows_sum<2>(part, nblk, 2, 1, S);
  if (threadIdx.x == 0) out[1] = S[1] > 0.0 ? S[0] / count : (double)__builtin_nanf("");
}

int grid_for(long long n) { return (int)max(1ll, min((n + EV_THREADS - 1) / EV_THREADS, (long long)EV_BLOCKS)); }

}  // namespace

// MG_OP_IIDSCORE_PREP / _PSNR / _SSIM share their slots: the launcher and mg_eval_iid read and write all three by PSNR's names
#define IID_SAME_SLOT(ARR_NAME) \
  static_assert((int)MG_IIDSCORE_PREP_##ARR_NAME == (int)MG_IIDSCORE_PSNR_##ARR_NAME && (int)MG_IIDSCORE_SSIM_##ARR_NAME == (int)MG_IIDSCORE_PSNR_##ARR_NAME, #ARR_NAME)
IID_SAME_SLOT(I_H); IID_SAME_SLOT(I_W); IID_SAME_SLOT(I_GAMMA); IID_SAME_SLOT(P_PRED); IID_SAME_SLOT(P_GT); IID_SAME_SLOT(P_MASK);
IID_SAME_SLOT(P_OUT); IID_SAME_SLOT(P_WS);
static_assert((int)MG_IIDSCORE_SSIM_I_UP_TO_SCALE == (int)MG_IIDSCORE_PSNR_I_UP_TO_SCALE, "I_UP_TO_SCALE");
#undef IID_SAME_SLOT

int mg_launch_evalscore(const mg_op* op, hipStream_t s) {
  switch (op->kind) {
    case MG_OP_EVAL_DEPTH_LS: {
      const int H = op->i[MG_EVAL_DEPTH_LS_I_H], W = op->i[MG_EVAL_DEPTH_LS_I_W], OW = op->i[MG_EVAL_DEPTH_LS_I_FIT_W];
      const float inv_factor = op->f[MG_EVAL_DEPTH_LS_F_INV_FACTOR];
      const float *pred = (const float*)op->p[MG_EVAL_DEPTH_LS_P_PRED], *gt = (const float*)op->p[MG_EVAL_DEPTH_LS_P_GT];
      const uint8_t* mask = (const uint8_t*)op->p[MG_EVAL_DEPTH_LS_P_MASK];
      double *out = (double*)op->p[MG_EVAL_DEPTH_LS_P_OUT], *scratch = (double*)op->p[MG_EVAL_DEPTH_LS_P_SCRATCH];
      MG_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "eval_depth_ls: bad size %d x %d", H, W);
      MG_REQUIRE(OW >= 0 && OW <= W, "eval_depth_ls: sub-sampled width %d outside [0, %d]", OW, W);
      MG_REQUIRE(OW == 0 || inv_factor >= 1.0f, "eval_depth_ls: inverse factor %g must be >= 1", (double)inv_factor);
      MG_REQUIRE(pred && gt && mask && out && scratch, "eval_depth_ls: null pointer");
      MG_REQUIRE(((uintptr_t)out | (uintptr_t)scratch) % 8 == 0, "eval_depth_ls: out / scratch not 8-byte aligned");
      const int nblk = grid_for((long long)H * (OW > 0 ? OW : W));
      MG_LAUNCH(depth_ls_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, pred, gt, mask, scratch, H, W, OW, inv_factor,
                op->i[MG_EVAL_DEPTH_LS_I_DISPARITY] != 0);
      MG_LAUNCH(sum_rows_kernel, dim3(1), dim3(64), 0, s, (const double*)scratch, out, nblk, LS_N);
      break;
    }
    case MG_OP_EVAL_DEPTH_METRICS: {
      const int H = op->i[MG_EVAL_DEPTH_METRICS_I_H], W = op->i[MG_EVAL_DEPTH_METRICS_I_W];
      const float *pred = (const float*)op->p[MG_EVAL_DEPTH_METRICS_P_PRED], *gt = (const float*)op->p[MG_EVAL_DEPTH_METRICS_P_GT];
      const uint8_t* mask = (const uint8_t*)op->p[MG_EVAL_DEPTH_METRICS_P_MASK];
      const double* sums = (const double*)op->p[MG_EVAL_DEPTH_METRICS_P_SUMS];
      double *out = (double*)op->p[MG_EVAL_DEPTH_METRICS_P_OUT], *scratch = (double*)op->p[MG_EVAL_DEPTH_METRICS_P_SCRATCH];
      MG_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "eval_depth_metrics: bad size %d x %d", H, W);
      MG_REQUIRE(pred && gt && mask && out && scratch, "eval_depth_metrics: null pointer");
      MG_REQUIRE(((uintptr_t)sums | (uintptr_t)out | (uintptr_t)scratch) % 8 == 0,
                 "eval_depth_metrics: sums / out / scratch not 8-byte aligned");
      const int nblk = grid_for((long long)H * W);
      MG_LAUNCH(depth_metrics_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, pred, gt, mask, sums, scratch, H * W,
                op->i[MG_EVAL_DEPTH_METRICS_I_DISPARITY] != 0, op->i[MG_EVAL_DEPTH_METRICS_I_CLIP_MIN] != 0,
                op->i[MG_EVAL_DEPTH_METRICS_I_CLIP_MAX] != 0, op->f[MG_EVAL_DEPTH_METRICS_F_MIN_DEPTH], op->f[MG_EVAL_DEPTH_METRICS_F_MAX_DEPTH]);
      MG_LAUNCH(depth_metrics_final_kernel, dim3(1), dim3(64), 0, s, (const double*)scratch, sums, out, nblk);
      break;
    }
    case MG_OP_EVAL_NORMALS: {
      const long long HW = op->l[MG_EVAL_NORMALS_L_HW];
      MG_REQUIRE(HW >= 0, "eval_normals: HW %lld < 0", HW);
      char* const ws = (char*)op->p[MG_EVAL_NORMALS_P_WS];
      const float *pred = (const float*)op->p[MG_EVAL_NORMALS_P_PRED], *gt = (const float*)op->p[MG_EVAL_NORMALS_P_GT];
      float* const err = (float*)op->p[MG_EVAL_NORMALS_P_ERR];
      double* const out = (double*)op->p[MG_EVAL_NORMALS_P_OUT];
      MG_REQUIRE(out && ws && (HW == 0 || (pred && gt)), "eval_normals: null pointer");
      MG_REQUIRE(((uintptr_t)out | (uintptr_t)ws) % 8 == 0, "eval_normals: out / workspace not 8-byte aligned");
      SelState* const st = (SelState*)(ws + WS_NM_STATE);
      unsigned *h0 = (unsigned*)(ws + WS_NM_HIST0), *h1 = (unsigned*)(ws + WS_NM_HIST1), *h2 = (unsigned*)(ws + WS_NM_HIST2);
      const int masked = op->i[MG_EVAL_NORMALS_I_MASKED] != 0, nblk = grid_for(HW);
      const NormalsAngles angles{pred, gt, err, HW, masked};
      if (!g_dry_run) MG_CHECK_HIP(hipMemsetAsync(ws + WS_NM_STATE, 0, WS_NORMALS_END - WS_NM_STATE, s));
      MG_LAUNCH(normals_stats_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, pred, gt, err, (double*)(ws + WS_NM_PART), h0, HW, masked);
      MG_LAUNCH(normals_reduce_kernel, dim3(1), dim3(128), 0, s, (const double*)(ws + WS_NM_PART), out, st, (const unsigned*)h0, nblk);
      MG_LAUNCH(select_hist_kernel<NormalsAngles>, dim3(nblk), dim3(EV_THREADS), 0, s, angles, (const SelState*)st, h1, HW, 10, 11);
      MG_LAUNCH(select_step_kernel, dim3(1), dim3(128), 0, s, st, (const unsigned*)h1, 2048, 11, (double*)nullptr);
      MG_LAUNCH(select_hist_kernel<NormalsAngles>, dim3(nblk), dim3(EV_THREADS), 0, s, angles, (const SelState*)st, h2, HW, 0, 10);
      MG_LAUNCH(select_step_kernel, dim3(1), dim3(128), 0, s, st, (const unsigned*)h2, 1024, 10, out + 1);
      break;
    }
    case MG_OP_IIDSCORE_PREP:
    case MG_OP_IIDSCORE_PSNR:
    case MG_OP_IIDSCORE_SSIM: {
      const char* const name = op->kind == MG_OP_IIDSCORE_PREP ? "iidscore_prep" : op->kind == MG_OP_IIDSCORE_PSNR ? "iidscore_psnr" : "iidscore_ssim";
      // (the three kinds share their slots: read by PSNR's names, which hold every field of the other two)
      const int H = op->i[MG_IIDSCORE_PSNR_I_H], W = op->i[MG_IIDSCORE_PSNR_I_W], gamma = op->i[MG_IIDSCORE_PSNR_I_GAMMA];
      const int mapped = op->i[MG_IIDSCORE_PSNR_I_UP_TO_SCALE] != 0;
      const float *pred = (const float*)op->p[MG_IIDSCORE_PSNR_P_PRED], *gt = (const float*)op->p[MG_IIDSCORE_PSNR_P_GT];
      char* const ws = (char*)op->p[MG_IIDSCORE_PSNR_P_WS];
      double* const out = (double*)op->p[MG_IIDSCORE_PSNR_P_OUT];
      MG_REQUIRE(H >= 1 && W >= 1 && 3ll * H * W < (1ll << 31), "%s: bad size %d x %d", name, H, W);
      MG_REQUIRE(op->kind != MG_OP_IIDSCORE_SSIM || (H >= SS_K && W >= SS_K),
                 "%s: H, W >= %d required (an 11 x 11 window, reflect padding by 5 and a non-empty crop), got %d x %d", name, SS_K, H, W);
      MG_REQUIRE(gamma >= MG_IID_GAMMA_NONE && gamma <= MG_IID_GAMMA_BOTH, "%s: unknown gamma mode %d", name, gamma);
      MG_REQUIRE(pred && gt && out && ws, "%s: null pointer", name);
      MG_REQUIRE(((uintptr_t)pred | (uintptr_t)gt) % 4 == 0, "%s: pred / gt not 4-byte aligned", name);
      MG_REQUIRE(((uintptr_t)out | (uintptr_t)ws) % 8 == 0, "%s: out / workspace not 8-byte aligned", name);
      const long long HW = (long long)H * W;
      IidMap* const map = (IidMap*)(ws + WS_II_MAP);
      const IidImages im{pred, gt, (const uint8_t*)op->p[MG_IIDSCORE_PSNR_P_MASK],
                         op->kind != MG_OP_IIDSCORE_PREP && mapped ? map : nullptr, gamma};
      if (op->kind == MG_OP_IIDSCORE_PREP) {
        const IidBrightness br{im.gt, im.mask, HW, gamma};
        SelState* const st = (SelState*)(ws + WS_II_STATE);
        unsigned *h0 = (unsigned*)(ws + WS_II_HIST0), *h1 = (unsigned*)(ws + WS_II_HIST1), *h2 = (unsigned*)(ws + WS_II_HIST2);
        const int nblk = grid_for(HW);
        if (!g_dry_run) MG_CHECK_HIP(hipMemsetAsync(ws + WS_II_STATE, 0, WS_II_PSNR_PART - WS_II_STATE, s));
        MG_LAUNCH(iid_prep_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, im, br, (double*)(ws + WS_II_PART), h0, HW);
        MG_LAUNCH(iid_prep_reduce_kernel, dim3(1), dim3(128), 0, s, (const double*)(ws + WS_II_PART), out, st, map, (const unsigned*)h0, nblk);
        MG_LAUNCH(select_hist_kernel<IidBrightness>, dim3(nblk), dim3(EV_THREADS), 0, s, br, (const SelState*)st, h1, HW, 10, 11);
        MG_LAUNCH(select_step_kernel, dim3(1), dim3(128), 0, s, st, (const unsigned*)h1, 2048, 11, (double*)nullptr);
        MG_LAUNCH(select_hist_kernel<IidBrightness>, dim3(nblk), dim3(EV_THREADS), 0, s, br, (const SelState*)st, h2, HW, 0, 10);
        MG_LAUNCH(iid_quantile_kernel, dim3(1), dim3(128), 0, s, st, (const unsigned*)h2, map, out);
      } else if (op->kind == MG_OP_IIDSCORE_PSNR) {
        const int nblk = grid_for(3 * HW);
        MG_LAUNCH(iid_psnr_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, im, (double*)(ws + WS_II_PSNR_PART), 3 * HW);
        MG_LAUNCH(iid_psnr_final_kernel, dim3(1), dim3(64), 0, s, (const double*)(ws + WS_II_PSNR_PART), out, nblk, mapped,
                  op->i[MG_IIDSCORE_PSNR_I_WRITE_PSNR] != 0);
      } else {
        const int OH = H - 2 * SS_R, OW = W - 2 * SS_R;
        const int nty = (OH + SS_T - 1) / SS_T, ntx = (OW + SS_T - 1) / SS_T;
        const int nblk = min(3 * nty * ntx, EV_BLOCKS);
        SsimWindow win;   // metrics.ssim: exp(-(d / sigma)^2 / 2), normalised
        double sum = 0.0;
        for (int k = 0; k < SS_K; ++k) {
          const double d = (double)(k - SS_R) / 1.5;
          sum += win.w[k] = exp(-(d * d) / 2.0);
        }
        for (int k = 0; k < SS_K; ++k) win.w[k] /= sum;
        MG_LAUNCH(iid_ssim_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, im, win, (double*)(ws + WS_II_SSIM_PART), H, W, nty, ntx);
        MG_LAUNCH(iid_ssim_final_kernel, dim3(1), dim3(64), 0, s, (const double*)(ws + WS_II_SSIM_PART), out, nblk,
                  3.0 * (double)OH * (double)OW);
      }
      break;
    }
    default: MG_REQUIRE(false, "evalscore: bad op kind %d", op->kind);
  }
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int mg_eval_depth(const float* pred, const float* gt, const uint8_t* mask, int H, int W, int alignment, int align_max_res,
                  double min_depth, double max_depth, double* out13, void* workspace, void* stream) {
  MG_REQUIRE(pred && gt && mask && out13 && workspace, "mg_eval_depth: null pointer");
  MG_REQUIRE(alignment >= MG_EVAL_ALIGN_NONE && alignment <= MG_EVAL_ALIGN_LS_DISPARITY, "mg_eval_depth: unknown alignment %d", alignment);
  MG_REQUIRE((uintptr_t)workspace % 8 == 0, "mg_eval_depth: workspace not 8-byte aligned");
  char* const ws = (char*)workspace;
  mg_op op;
  if (alignment != MG_EVAL_ALIGN_NONE) {
    memset(&op, 0, sizeof(op));
    op.kind = MG_OP_EVAL_DEPTH_LS;
    op.p[MG_EVAL_DEPTH_LS_P_PRED] = (void*)pred;
    op.p[MG_EVAL_DEPTH_LS_P_GT] = (void*)gt;
    op.p[MG_EVAL_DEPTH_LS_P_MASK] = (void*)mask;
    op.p[MG_EVAL_DEPTH_LS_P_OUT] = ws + WS_LS_SUMS;
    op.p[MG_EVAL_DEPTH_LS_P_SCRATCH] = ws + WS_LS_PART;
    op.i[MG_EVAL_DEPTH_LS_I_H] = H;
    op.i[MG_EVAL_DEPTH_LS_I_W] = W;
    op.i[MG_EVAL_DEPTH_LS_I_DISPARITY] = alignment == MG_EVAL_ALIGN_LS_DISPARITY;
    if (align_max_res > 0 && H >= 1 && W >= 1) {   // align_depth_least_square: factor = min(max_res / (H, W)), applied when < 1
      const double fh = (double)align_max_res / (double)H, fw = (double)align_max_res / (double)W;
      const double factor = fh < fw ? fh : fw;
      if (factor < 1.0) {
        op.i[MG_EVAL_DEPTH_LS_I_FIT_W] = (int)floor((double)W * factor);
        op.f[MG_EVAL_DEPTH_LS_F_INV_FACTOR] = (float)(1.0 / factor);
        MG_REQUIRE(op.i[MG_EVAL_DEPTH_LS_I_FIT_W] >= 1, "mg_eval_depth: alignment_max_res %d leaves no column of a %d x %d map", align_max_res, H, W);
      }
    }
    const int rc = mg_launch_evalscore(&op, (hipStream_t)stream);
    if (rc) return rc;
  }
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_EVAL_DEPTH_METRICS;
  const bool clip_min = min_depth == min_depth, clip_max = max_depth == max_depth;   // (NaN = no limit)
  op.p[MG_EVAL_DEPTH_METRICS_P_PRED] = (void*)pred;
  op.p[MG_EVAL_DEPTH_METRICS_P_GT] = (void*)gt;
  op.p[MG_EVAL_DEPTH_METRICS_P_MASK] = (void*)mask;
  op.p[MG_EVAL_DEPTH_METRICS_P_SUMS] = alignment != MG_EVAL_ALIGN_NONE ? ws + WS_LS_SUMS : nullptr;
  op.p[MG_EVAL_DEPTH_METRICS_P_OUT] = out13;
  op.p[MG_EVAL_DEPTH_METRICS_P_SCRATCH] = ws + WS_DM_PART;
  op.i[MG_EVAL_DEPTH_METRICS_I_H] = H;
  op.i[MG_EVAL_DEPTH_METRICS_I_W] = W;
  op.i[MG_EVAL_DEPTH_METRICS_I_DISPARITY] = alignment == MG_EVAL_ALIGN_LS_DISPARITY;
  op.i[MG_EVAL_DEPTH_METRICS_I_CLIP_MIN] = clip_min;
  op.i[MG_EVAL_DEPTH_METRICS_I_CLIP_MAX] = clip_max;
  op.f[MG_EVAL_DEPTH_METRICS_F_MIN_DEPTH] = clip_min ? (float)min_depth : 0.f;
  op.f[MG_EVAL_DEPTH_METRICS_F_MAX_DEPTH] = clip_max ? (float)max_depth : 0.f;
  return mg_launch_evalscore(&op, (hipStream_t)stream);
}

int mg_eval_normals(const float* pred, const float* gt, int64_t HW, int masked, double* out9, float* err_map_or_null,
                    void* workspace, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_EVAL_NORMALS;
  op.p[MG_EVAL_NORMALS_P_PRED] = (void*)pred;
  op.p[MG_EVAL_NORMALS_P_GT] = (void*)gt;
  op.p[MG_EVAL_NORMALS_P_OUT] = out9;
  op.p[MG_EVAL_NORMALS_P_ERR] = err_map_or_null;
  op.p[MG_EVAL_NORMALS_P_WS] = workspace;
  op.i[MG_EVAL_NORMALS_I_MASKED] = masked;
  op.l[MG_EVAL_NORMALS_L_HW] = HW;
  return mg_launch_evalscore(&op, (hipStream_t)stream);
}

int mg_eval_iid(const float* pred, const float* gt, const uint8_t* mask_or_null, int H, int W, int up_to_scale, int gamma_mode,
                int metrics_mask, double* out8, void* workspace, void* stream) {
  MG_REQUIRE(pred && gt && out8 && workspace, "mg_eval_iid: null pointer");
  MG_REQUIRE(H >= SS_K && W >= SS_K, "mg_eval_iid: H, W >= %d required (an 11 x 11 window, reflect padding by 5 and a non-empty crop), got %d x %d",
             SS_K, H, W);
  MG_REQUIRE(metrics_mask >= 0 && metrics_mask <= (MG_IID_PSNR | MG_IID_SSIM), "mg_eval_iid: unknown metrics mask %d", metrics_mask);
  MG_REQUIRE(((uintptr_t)out8 | (uintptr_t)workspace) % 8 == 0, "mg_eval_iid: out / workspace not 8-byte aligned");
  if (!g_dry_run) MG_CHECK_HIP(hipMemsetAsync(out8, 0xff, 8 * sizeof(double), (hipStream_t)stream));   // every slot NaN until an op fills it
  mg_op op;
  memset(&op, 0, sizeof(op));
  // one op, launched as each kind in turn: the three share their slots (PSNR's names hold every field of the other two)
  op.p[MG_IIDSCORE_PSNR_P_PRED] = (void*)pred;
  op.p[MG_IIDSCORE_PSNR_P_GT] = (void*)gt;
  op.p[MG_IIDSCORE_PSNR_P_MASK] = (void*)mask_or_null;
  op.p[MG_IIDSCORE_PSNR_P_OUT] = out8;
  op.p[MG_IIDSCORE_PSNR_P_WS] = workspace;
  op.i[MG_IIDSCORE_PSNR_I_H] = H;
  op.i[MG_IIDSCORE_PSNR_I_W] = W;
  op.i[MG_IIDSCORE_PSNR_I_GAMMA] = gamma_mode;
  op.i[MG_IIDSCORE_PSNR_I_UP_TO_SCALE] = up_to_scale != 0;
  int rc = 0;
  if (up_to_scale) {
    op.kind = MG_OP_IIDSCORE_PREP;
    if ((rc = mg_launch_evalscore(&op, (hipStream_t)stream))) return rc;
  }
  op.kind = MG_OP_IIDSCORE_PSNR;   // always: it counts the valid elements
  op.i[MG_IIDSCORE_PSNR_I_WRITE_PSNR] = (metrics_mask & MG_IID_PSNR) != 0;
  if ((rc = mg_launch_evalscore(&op, (hipStream_t)stream))) return rc;
  if (metrics_mask & MG_IID_SSIM) {
    op.kind = MG_OP_IIDSCORE_SSIM;
    rc = mg_launch_evalscore(&op, (hipStream_t)stream);
  }
  return rc;
}

}  // extern "C"
