// Image sequences: the blend that carries frame k - 1's denoised latent into frame k's initial noise,
//     x <- (1 - strength) x + strength prev,
// rounded like the three separate torch ops (x * a) + (prev * b) with a, b as fp32: two products, one sum, no FMA (the
// file is built with -ffp-contract=off and the kernel spells the roundings out).  HBM-bound: two reads and one write per element.
#include "common.h"

namespace {

// vec: both pointers are 16-byte aligned - lanes take float4s, then the n % 4 tail element by element; else element by element
__global__ __launch_bounds__(256) void latent_carry_kernel(float* x, const float* prev, long long n, float a, float b, int vec) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const long long nv = vec ? n >> 2 : 0;
  for (long long i = tid; i < nv; i += stride) {
    float4 v = ((const float4*)x)[i];
    const float4 p = ((const float4*)prev)[i];
    v.x = __fadd_rn(__fmul_rn(a, v.x), __fmul_rn(b, p.x));
    v.y = __fadd_rn(__fmul_rn(a, v.y), __fmul_rn(b, p.y));
    v.z = __fadd_rn(__fmul_rn(a, v.z), __fmul_rn(b, p.z));
    v.w = __fadd_rn(__fmul_rn(a, v.w), __fmul_rn(b, p.w));
    ((float4*)x)[i] = v;
  }
  for (long long i = nv * 4 + tid; i < n; i += stride) x[i] = __fadd_rn(__fmul_rn(a, x[i]), __fmul_rn(b, prev[i]));
}

}  // namespace

extern "C" int mg_latent_carry(float* x, const float* prev, int64_t n, float strength, void* stream) {
  MG_REQUIRE(n >= 0, "mg_latent_carry: bad element count %lld", (long long)n);
  MG_REQUIRE(strength >= 0.f && strength <= 1.f, "mg_latent_carry: strength %g is not in [0, 1]", (double)strength);   // (a NaN fails both)
  if (n == 0) return 0;
  MG_REQUIRE(x && prev, "mg_latent_carry: null pointer");
  MG_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)prev % 4 == 0, "mg_latent_carry: the pointers must be aligned to their elements");
  const float b = strength, a = (float)(1.0 - (double)strength);
  const int vec = (uintptr_t)x % 16 == 0 && (uintptr_t)prev % 16 == 0;
  const long long nv = vec ? n >> 2 : 0, work = nv > n - 4 * nv ? nv : n - 4 * nv;
  const int grid = (int)min((work + 255) / 256, (long long)2048);
  MG_LAUNCH(latent_carry_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, prev, (long long)n, a, b, vec);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
