// Edge-guided (joint bilateral) upsampling of a prediction to the input picture's size: the low-resolution prediction
// is enlarged with tent weights, and every tap is weighted once more by how closely the picture at the tap - the picture resampled to
// the prediction's size - resembles the full-size picture at the output pixel.  The definition is in include/marigold_hip.h.
// One workgroup makes a tile of 32 x 8 output pixels, one pixel per lane.  The low-resolution taps of the whole tile - the footprint -
// are staged once in LDS: the guide as three fp32 planes already divided by 255, the prediction as C fp32 planes.  A lane reads its
// three bytes of the full-size picture once, keeps its (2R)^2 weights in registers, and writes one float per channel: a wave stores two
// row segments of 128 bytes per channel.  A tile whose footprint exceeds the LDS given to the launch (strong reductions only) reads
// its taps from global memory with the same arithmetic, so the bits do not depend on the route.  No atomics; fp32; expf; built with
// -ffp-contract=off: the roundings are the ones written.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace {

constexpr int GU_TX = 32, GU_TY = 8, GU_THREADS = GU_TX * GU_TY;
constexpr int GU_MAX_STAGE = 704;   // footprint pixels a launch stages at most: 12 + 4 C bytes each, 53.6 KiB at C = 16

struct gu_args {
  const float* __restrict__ pred;
  const uint8_t* __restrict__ lo;
  const uint8_t* __restrict__ hi;
  float* __restrict__ out;
  int C, h, w, H, W, hwc, tiles_x, cap;
  float sy, sx, two_sigma2;
};

__device__ __forceinline__ float gu_src(int dst, float scale) { return scale * ((float)dst + 0.5f) - 0.5f; }
__device__ __forceinline__ int gu_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float gu_unit(unsigned byte) { return __fdiv_rn((float)byte, 255.0f); }

// the footprint of a tile along one axis: the clamped taps of its first and last pixel (the source coordinate is monotonic in the pixel)
__device__ __forceinline__ void gu_span(int first, int last, float scale, int R, int len, int& lo, int& hi) {
  lo = gu_clamp((int)floorf(gu_src(first, scale)) - R + 1, len - 1);
  hi = gu_clamp((int)floorf(gu_src(last, scale)) + R, len - 1);
}

// One output pixel.  STAGED: guide and prediction of tap (i, j) at LDS slot (i - i_lo) ncols + (j - j_lo), planes `cap` apart.
template <int R, int CMAX, bool STAGED>
__device__ __forceinline__ void gu_pixel(const gu_args& a, int Y, int X, const float* __restrict__ sg, const float* __restrict__ sp, int i_lo,
                                         int j_lo, int ncols) {
  constexpr int T = 2 * R;
  const long long hw = (long long)a.h * a.w, HW = (long long)a.H * a.W, P = (long long)Y * a.W + X;
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = gu_unit(a.hwc ? a.hi[P * 3 + c] : a.hi[c * HW + P]);
  const float sy = gu_src(Y, a.sy), sx = gu_src(X, a.sx);
  const int fy = (int)floorf(sy), fx = (int)floorf(sx);
  float wy[T], wx[T];
  std::conditional_t<STAGED, int, long long> ro[T];   // the tap's row: the LDS slot (STAGED) or the plane element where it starts
  int co[T];                                          // its column within that row
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int i = fy - R + 1 + t, j = fx - R + 1 + t;
    wy[t] = fmaxf(0.0f, 1.0f - __fdiv_rn(fabsf(sy - (float)i), (float)R));
    wx[t] = fmaxf(0.0f, 1.0f - __fdiv_rn(fabsf(sx - (float)j), (float)R));
    const int ic = gu_clamp(i, a.h - 1), jc = gu_clamp(j, a.w - 1);
    ro[t] = STAGED ? (ic - i_lo) * ncols : (long long)ic * a.w;
    co[t] = STAGED ? jc - j_lo : jc;
  }
  float wt[T * T], den = 0.0f;
#pragma unroll
  for (int ty = 0; ty < T; ++ty)
#pragma unroll
    for (int tx = 0; tx < T; ++tx) {
      float d2 = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float l = STAGED ? sg[c * a.cap + ro[ty] + co[tx]] : gu_unit(a.lo[c * hw + ro[ty] + co[tx]]);
        const float d = g[c] - l;
        d2 = d2 + d * d;
      }
      const float range = expf(__fdiv_rn(-d2, a.two_sigma2)) + 1e-4f;
      wt[ty * T + tx] = (wy[ty] * wx[tx]) * range;
      den = den + wt[ty * T + tx];
    }
  // out = sum (weight / sum of weights) pred: with one tap of non-zero weight its quotient is exactly 1 and the value passes unchanged
  float acc[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int ty = 0; ty < T; ++ty)
#pragma unroll
    for (int tx = 0; tx < T; ++tx) {
      const float wn = __fdiv_rn(wt[ty * T + tx], den);
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < a.C) {   // (uniform over the grid)
          const float v = STAGED ? sp[c * a.cap + ro[ty] + co[tx]] : a.pred[c * hw + ro[ty] + co[tx]];
          acc[c] = acc[c] + wn * v;
        }
    }
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < a.C) a.out[c * HW + P] = acc[c];
}

// grid: tiles_x * tiles_y workgroups, tile = blockIdx.x row-major; dynamic LDS: fp32 [3 + C][cap] (no static LDS: the base stays aligned)
template <int R, int CMAX>
__global__ __launch_bounds__(GU_THREADS) void guided_upsample_kernel(const gu_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gu_lds[];
  float* __restrict__ sg = (float*)gu_lds;
  float* __restrict__ sp = sg + 3 * a.cap;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x % a.tiles_x;
  const int Y0 = tile_y * GU_TY, X0 = tile_x * GU_TX;
  const int Y1 = min(Y0 + GU_TY, a.H) - 1, X1 = min(X0 + GU_TX, a.W) - 1;
  int i_lo, i_hi, j_lo, j_hi;
  gu_span(Y0, Y1, a.sy, R, a.h, i_lo, i_hi);
  gu_span(X0, X1, a.sx, R, a.w, j_lo, j_hi);
  const int ncols = j_hi - j_lo + 1;
  const long long npix = (long long)(i_hi - i_lo + 1) * ncols;
  const bool staged = npix <= a.cap;   // (uniform over the workgroup)
  if (staged) {
    const long long hw = (long long)a.h * a.w;
    for (int p = threadIdx.x; p < (int)npix; p += GU_THREADS) {
      const long long q = (long long)(i_lo + p / ncols) * a.w + j_lo + p % ncols;
#pragma unroll
      for (int c = 0; c < 3; ++c) sg[c * a.cap + p] = gu_unit(a.lo[c * hw + q]);
      for (int c = 0; c < a.C; ++c) sp[c * a.cap + p] = a.pred[c * hw + q];
    }
  }
  __syncthreads();
  const int Y = Y0 + threadIdx.x / GU_TX, X = X0 + threadIdx.x % GU_TX;
  if (Y >= a.H || X >= a.W) return;
  if (staged) gu_pixel<R, CMAX, true>(a, Y, X, sg, sp, i_lo, j_lo, ncols);
  else gu_pixel<R, CMAX, false>(a, Y, X, sg, sp, i_lo, j_lo, ncols);
}

template <int R>
void gu_launch_r(const gu_args& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.C == 1) MG_LAUNCH((guided_upsample_kernel<R, 1>), grid, dim3(GU_THREADS), lds, s, a);
  else if (a.C <= 3) MG_LAUNCH((guided_upsample_kernel<R, 3>), grid, dim3(GU_THREADS), lds, s, a);
  else if (a.C <= 6) MG_LAUNCH((guided_upsample_kernel<R, 6>), grid, dim3(GU_THREADS), lds, s, a);
  else MG_LAUNCH((guided_upsample_kernel<R, 16>), grid, dim3(GU_THREADS), lds, s, a);
}

// an upper bound of a tile's footprint along one axis: the taps of `n` consecutive pixels, at most the axis itself
long long gu_span_bound(int n, float scale, int R, int len) {
  const double reach = (double)(n - 1) * (double)scale + 2.0 * R + 2.0;
  return reach < (double)len ? (long long)reach : (long long)len;
}

}  // namespace

extern "C" int mg_guided_upsample(const float* pred, int C, int h, int w, const uint8_t* guide_lo, const uint8_t* guide_hi, int hwc, int H,
                                  int W, int radius, float sigma, float* out, void* stream) {
  const char* fn = "mg_guided_upsample";
  MG_REQUIRE(pred && guide_lo && guide_hi && out, "%s: null pointer", fn);
  MG_REQUIRE(C >= 1 && C <= 16, "%s: %d channels, 1 to 16 are supported", fn, C);
  MG_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, "%s: bad size %d x %d -> %d x %d", fn, h, w, H, W);
  MG_REQUIRE((long long)h * w <= (1ll << 30) && (long long)H * W <= (1ll << 30), "%s: a size above 2^30 pixels (%d x %d -> %d x %d) is not supported", fn,
             h, w, H, W);
  MG_REQUIRE(radius >= 1 && radius <= 4, "%s: radius %d, 1 to 4 are supported", fn, radius);
  const float two_sigma2 = 2.0f * sigma * sigma;
  MG_REQUIRE(sigma > 0.0f && isfinite(sigma) && two_sigma2 > 0.0f && isfinite(two_sigma2),
             "%s: sigma must be finite and > 0, with 2 sigma^2 inside the fp32 range (got %g)", fn, (double)sigma);
  MG_REQUIRE((uintptr_t)pred % 4 == 0 && (uintptr_t)out % 4 == 0, "%s: pred and out must be 4-byte aligned", fn);
  gu_args a;
  a.pred = pred; a.lo = guide_lo; a.hi = guide_hi; a.out = out;
  a.C = C; a.h = h; a.w = w; a.H = H; a.W = W; a.hwc = hwc != 0;
  a.sy = (float)h / (float)H; a.sx = (float)w / (float)W; a.two_sigma2 = two_sigma2;
  a.tiles_x = (W + GU_TX - 1) / GU_TX;
  const long long tiles = (long long)a.tiles_x * ((H + GU_TY - 1) / GU_TY);   // <= 2^30 / 8 + ...: fits the grid's x
  // LDS for the largest footprint a tile of this launch can have, GU_MAX_STAGE pixels at most; the kernel checks each tile against it
  const long long bound = gu_span_bound(GU_TY, a.sy, radius, h) * gu_span_bound(GU_TX, a.sx, radius, w);
  a.cap = (int)(bound < GU_MAX_STAGE ? bound : GU_MAX_STAGE);
  a.cap = (a.cap + 3) / 4 * 4;   // planes start on 16 bytes
  const size_t lds = (size_t)(3 + C) * a.cap * sizeof(float);
  const dim3 grid((unsigned)tiles);
  hipStream_t s = (hipStream_t)stream;
  switch (radius) {
    case 1: gu_launch_r<1>(a, grid, lds, s); break;
    case 2: gu_launch_r<2>(a, grid, lds, s); break;
    case 3: gu_launch_r<3>(a, grid, lds, s); break;
    default: gu_launch_r<4>(a, grid, lds, s); break;
  }
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
