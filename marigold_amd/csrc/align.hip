// Depth alignment: the robust scale and shift that carry one depth map into the range of another - a reference with
// trusted values, or the frame before - and their application.  The contract of every entry point is in include/marigold_hip.h.
// A fit is 1 + iters (+ 1 under MG_ALIGN_START_LS) pairs of launches: the partial sums of fixed chunks of pixels, then one wave that
// adds the partials and solves; the order of every sum is reduce.h's.  The coefficients stay on the device: the solve writes them to
// `coef`, the next partial launch reads its weights' coefficients from there.  Bound by memory where it is bound by anything: 8 n bytes per solve,
// tens of microseconds at 768 x 768 - the launches themselves cost as much.  fp64 throughout, as in the tile fit (tiles.hip), the price
// of a result that can be checked to 1e-9.  Built with -ffp-contract=off: every product and sum below is rounded on its own.
#include <cmath>

#include "common.h"
#include "reduce.h"

namespace {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_CHUNK = 4096;                            // pixels per workgroup: 16 per lane, all loads in flight together
constexpr int ALIGN_PER_THREAD = ALIGN_CHUNK / ALIGN_THREADS;
constexpr int ALIGN_SUMS = 6;                                // count, N, Sd, Sg, Sdd, Sdg
constexpr long long ALIGN_MAX_N = 1ll << 30;

enum { WEIGHTS_ONE = 0, WEIGHTS_FROM_ARGS = 1, WEIGHTS_FROM_COEF = 2 };

// grid (chunks): block c sums pixels [c ALIGN_CHUNK, (c + 1) ALIGN_CHUNK) -> part[c * 6 + {count, N, Sd, Sg, Sdd, Sdg}].  Element loads
// (consecutive lanes, consecutive pixels): no alignment beyond the element's is asked of d and ref, and the lane that takes a pixel - hence
// the order of every sum - does not depend on where the buffers lie.
__global__ __launch_bounds__(ALIGN_THREADS) void align_partial_kernel(const float* __restrict__ d, const float* __restrict__ ref,
                                                                      const unsigned char* __restrict__ mask, long long n, int weights,
                                                                      double s_arg, double t_arg, double delta,
                                                                      const double* __restrict__ coef, double* __restrict__ part) {
  const long long base = (long long)blockIdx.x * ALIGN_CHUNK + threadIdx.x;
  const float nan = __builtin_nanf("");
  float dv[ALIGN_PER_THREAD], gv[ALIGN_PER_THREAD];
#pragma unroll
  for (int j = 0; j < ALIGN_PER_THREAD; ++j) {
    const long long i = base + (long long)j * ALIGN_THREADS;
    const bool in = i < n && (mask == nullptr || mask[i] != 0);   // beyond the map or masked out: a NaN, which no sum takes
    dv[j] = in ? d[i] : nan;
    gv[j] = in ? ref[i] : nan;
  }
  double s = s_arg, t = t_arg;
  if (weights == WEIGHTS_FROM_COEF) {
    s = coef[0];
    t = coef[1];
  }
  double acc[ALIGN_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < ALIGN_PER_THREAD; ++j) {
    if (isfinite(dv[j]) && isfinite(gv[j])) {
      const double x = (double)dv[j], g = (double)gv[j];
      double w = 1.0;
      if (weights != WEIGHTS_ONE) {
        const double r = ((s * x + t) - g) / delta;
        w = 1.0 / (1.0 + r * r);
      }
      const double wd = w * x;
      acc[0] += 1.0;
      acc[1] += w;
      acc[2] += wd;
      acc[3] += w * g;
      acc[4] += wd * x;
      acc[5] += wd * g;
    }
  }
  block_sum_store<ALIGN_SUMS, ALIGN_THREADS>(acc, part + (long long)blockIdx.x * ALIGN_SUMS);
}

// one wave: the partials of the chunks, lane-strided (reduce.h), then lane 0 solves.  `first`: the fit's first solve, which sets the
// flag; a later one leaves a fit that is already degenerate alone.
__global__ __launch_bounds__(64) void align_solve_kernel(const double* __restrict__ part, long long chunks, int fit_shift, int first,
                                                         double* __restrict__ coef, int* __restrict__ flag) {
  double a[ALIGN_SUMS];
  lane_rows_sum<ALIGN_SUMS>(part, chunks, a);
  if (threadIdx.x != 0) return;
  if (!first && flag[0] != 0) return;
  const double count = a[0], N = a[1], Sd = a[2], Sg = a[3], Sdd = a[4], Sdg = a[5];
  double s = 1.0, t = 0.0;
  int bad = 1;
  if (count >= 2.0) {
    if (fit_shift) {
      const scale_shift f = scale_shift_solve(N, Sd, Sg, Sdd, Sdg);
      if (f.det > 1e-12 * N * N) {
        s = f.s;
        t = f.t;
        bad = 0;
      }
    } else if (Sdd > 1e-12 * N) {
      s = Sdg / Sdd;
      bad = 0;
    }
  }
  if (bad || !(s > 0.0) || !isfinite(s) || !isfinite(t)) {
    s = 1.0;
    t = 0.0;
    bad = 1;
  }
  coef[0] = s;
  coef[1] = t;
  flag[0] = bad;
}

__device__ __forceinline__ float apply_one(float x, double s, double t, int clip, float lo, float hi) {
  const float v = (float)((double)x * s + t);
  return clip ? (v < lo ? lo : (v > hi ? hi : v)) : v;   // (a NaN fails both comparisons and stays)
}

// vec: both pointers are 16-byte aligned - lanes take float4s, then the n % 4 tail element by element; else element by element.  out may
// be x: a lane reads what it writes, nothing else.
__global__ __launch_bounds__(256) void align_apply_kernel(const float* x, long long n, const double* __restrict__ coef, int use_shift, int clip,
                                                          float lo, float hi, float* out, int vec) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const double s = coef[0], t = use_shift ? coef[1] : 0.0;
  const long long nv = vec ? n >> 2 : 0;
  for (long long i = tid; i < nv; i += stride) {
    float4 v = ((const float4*)x)[i];
    v.x = apply_one(v.x, s, t, clip, lo, hi);
    v.y = apply_one(v.y, s, t, clip, lo, hi);
    v.z = apply_one(v.z, s, t, clip, lo, hi);
    v.w = apply_one(v.w, s, t, clip, lo, hi);
    ((float4*)out)[i] = v;
  }
  for (long long i = nv * 4 + tid; i < n; i += stride) out[i] = apply_one(x[i], s, t, clip, lo, hi);
}

long long chunks_of(long long n) { return (n + ALIGN_CHUNK - 1) / ALIGN_CHUNK; }

}  // namespace

extern "C" long long mg_depth_align_workspace_bytes(long long n) {
  if (n < 1 || n > ALIGN_MAX_N) {
    mg_set_error("mg_depth_align_workspace_bytes: %lld pixels, 1 to 2^30 are supported", n);
    return -1;
  }
  return chunks_of(n) * ALIGN_SUMS * (long long)sizeof(double);
}

extern "C" int mg_depth_align_fit(const float* d, const float* ref, const unsigned char* mask_or_null, long long n, int fit_shift, int iters,
                                  int start_mode, double s_start, double t_start, double delta, double* coef, int* flag, void* ws,
                                  long long ws_bytes, void* stream) {
  const char* fn = "mg_depth_align_fit";
  MG_REQUIRE(n >= 1 && n <= ALIGN_MAX_N, "%s: %lld pixels, 1 to 2^30 are supported", fn, n);
  MG_REQUIRE(d && ref && coef && flag && ws, "%s: null pointer", fn);
  MG_REQUIRE((uintptr_t)d % 4 == 0 && (uintptr_t)ref % 4 == 0 && (uintptr_t)coef % 8 == 0 && (uintptr_t)flag % 4 == 0,
             "%s: d, ref, coef and flag must be aligned to their elements", fn);
  MG_REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
  const long long need = mg_depth_align_workspace_bytes(n);
  MG_REQUIRE(ws_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (mg_depth_align_workspace_bytes)", fn, ws_bytes, need);
  MG_REQUIRE(iters >= 0 && iters <= MG_ALIGN_MAX_ITERS, "%s: %d iterations, 0 to %d are supported", fn, iters, MG_ALIGN_MAX_ITERS);
  if (iters >= 1) {
    MG_REQUIRE(start_mode == MG_ALIGN_START_GIVEN || start_mode == MG_ALIGN_START_LS, "%s: unknown start mode %d", fn, start_mode);
    MG_REQUIRE(std::isfinite(delta) && delta > 0.0, "%s: delta %g is not finite and > 0", fn, delta);
    MG_REQUIRE(start_mode != MG_ALIGN_START_GIVEN || (std::isfinite(s_start) && std::isfinite(t_start)), "%s: the start values (%g, %g) are not finite", fn,
               s_start, t_start);
  }
  const long long chunks = chunks_of(n);   // (<= 2^18: a grid's x extent)
  const hipStream_t st = (hipStream_t)stream;
  int first = 1;
  const auto solve = [&](int weights) {
    MG_LAUNCH(align_partial_kernel, dim3((unsigned)chunks), dim3(ALIGN_THREADS), 0, st, d, ref, mask_or_null, n, weights, s_start, t_start, delta,
              (const double*)coef, (double*)ws);
    MG_LAUNCH(align_solve_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, chunks, fit_shift, first, coef, flag);
    first = 0;
  };
  if (iters == 0 || start_mode == MG_ALIGN_START_LS) solve(WEIGHTS_ONE);
  for (int k = 0; k < iters; ++k) solve(k == 0 && start_mode == MG_ALIGN_START_GIVEN ? WEIGHTS_FROM_ARGS : WEIGHTS_FROM_COEF);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mg_depth_align_apply(const float* x, long long n, const double* coef, int use_shift, float clip_lo, float clip_hi, float* out,
                                    void* stream) {
  const char* fn = "mg_depth_align_apply";
  MG_REQUIRE(n >= 1 && n <= ALIGN_MAX_N, "%s: %lld elements, 1 to 2^30 are supported", fn, n);
  MG_REQUIRE(x && coef && out, "%s: null pointer", fn);
  MG_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)coef % 8 == 0, "%s: x, out and coef must be aligned to their elements",
             fn);
  const int clip = clip_lo <= clip_hi;   // (false with a NaN bound: no clamp)
  const int vec = (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0;
  const long long nv = vec ? n >> 2 : 0, work = nv > n - 4 * nv ? nv : n - 4 * nv;
  const int grid = (int)min((work + 255) / 256, (long long)2048);
  MG_LAUNCH(align_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, coef, use_shift, clip, clip_lo, clip_hi, out, vec);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
