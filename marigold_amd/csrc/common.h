// Shared device helpers for libmarigold_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include "../../include/marigold_hip.h"

// The 16-bit operand type of the build: bf16 (the product library, libmarigold_hip.so) or IEEE fp16 (libmarigold_hip_f16.so, built
// from the same sources with -DMG_OPERAND_F16_BUILD=1: what the reference computes with `--fp16` / torch_dtype=torch.float16,
// script/depth/run.py:203-211).  Same MFMA rate (v_mfma_f32_32x32x16_f16), three more mantissa bits, five fewer exponent bits:
// every conversion, unpack and matrix instruction of the kernels goes through the helpers below, so the kernels are written once.
// The names keep "bf16" (the product type); in the fp16 build they hold fp16 bits.
constexpr bool MG_F16 = MG_OPERAND_F16_BUILD != 0;
typedef uint16_t bf16_t;  // raw operand bits
typedef std::conditional_t<MG_F16, _Float16, __bf16> mg_op16_t;
typedef __attribute__((ext_vector_type(8))) mg_op16_t bf16x8;
typedef __attribute__((ext_vector_type(2))) mg_op16_t mg_bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float mg_f32x2_t;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

// mnemonics for the hand-placed instruction streams (csrc/gen_*.py emit them as adjacent string literals)
#if MG_OPERAND_F16_BUILD
#define MG_MFMA32_ASM "v_mfma_f32_32x32x16_f16"
#define MG_MFMA16_ASM "v_mfma_f32_16x16x32_f16"
#define MG_CVT_PK_ASM "v_cvt_pk_f16_f32"
#else
#define MG_MFMA32_ASM "v_mfma_f32_32x32x16_bf16"
#define MG_MFMA16_ASM "v_mfma_f32_16x16x32_bf16"
#define MG_CVT_PK_ASM "v_cvt_pk_bf16_f32"
#endif
constexpr float MG_OP16_MAX = MG_F16 ? 65504.0f : 3.3895314e38f;   // largest finite operand value

// Clamps, minima and maxima that KEEP NaN, as torch.clip / clamp(min=) / .min() / .max() do: fminf / fmaxf return the other operand
// (fmaxf(NaN, -1) = -1; v_med3_f32 returns min3 on a NaN), and everything after the decoder's last convolution must hand a
// non-finite value on as the reference does, never turn it into a plausible finite one.  Finite operands: the same bits.
__device__ __forceinline__ float clip_keep_nan(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float floor_keep_nan(float x, float lo) { return x != x ? x : fmaxf(x, lo); }
// IEEE 754-2019 minimum / maximum: one instruction each on gfx950 (v_minimum3_f32 / v_maximum3_f32), the price of fminf / fmaxf
__device__ __forceinline__ float min_keep_nan(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float max_keep_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// the running (value, pixel) extremum of the ensembling passes: does candidate (o, op) replace (m, p)?  A NaN beats every number
// (torch's .min() / .max() / argmin / argmax), equal values - and NaN among themselves - go to the lowest pixel
__device__ __forceinline__ bool takes_min(float o, long long op, float m, long long p) {
  return o < m || (o != o && m == m) || ((o == m || (o != o && m != m)) && op < p);
}
__device__ __forceinline__ bool takes_max(float o, long long op, float m, long long p) {
  return o > m || (o != o && m == m) || ((o == m || (o != o && m != m)) && op < p);
}

typedef __attribute__((ext_vector_type(8))) _Float16 mg_f16x8_t;
typedef __attribute__((ext_vector_type(8))) __bf16 mg_bf16x8_t;
__device__ __forceinline__ f32x16 mg_mfma32(bf16x8 a, bf16x8 b, f32x16 c) {   // D = A (32 x 16) B (16 x 32) + C
  if constexpr (MG_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(mg_f16x8_t, a), __builtin_bit_cast(mg_f16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mg_bf16x8_t, a), __builtin_bit_cast(mg_bf16x8_t, b), c, 0, 0, 0);
}

__device__ __forceinline__ float bf2f(bf16_t v) {
  if constexpr (MG_F16) return (float)__builtin_bit_cast(_Float16, v);
  else return __uint_as_float(((uint32_t)v) << 16);
}
// two fp32 -> packed operands (round to nearest even) in one instruction: v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32; the fp16 form
// saturates at +-65504 (a bf16 value of 1e5 is a number, an fp16 inf poisons every sum it enters) and keeps NaN: the pair is
// converted first (|x| >= 65520 rounds to inf) and then clamped with IEEE maximum / minimum (v_pk_maximum3_f16 / v_pk_minimum3_f16),
// which propagate NaN - a clamp by v_med3_f32 / v_max_f32 turns a NaN into -65504.  Two VALU ops per pair as before, but the dependent
// packed pair needs an s_nop between them and the constants take moves: the fp16 objects grow by about 1 %.
__device__ __forceinline__ uint32_t cvt_pk_bf16_f32(float lo, float hi) {
  mg_f32x2_t v = {lo, hi};
  mg_bf16x2_t h = __builtin_convertvector(v, mg_bf16x2_t);
  if constexpr (MG_F16) {
    const mg_bf16x2_t m = {(mg_op16_t)MG_OP16_MAX, (mg_op16_t)MG_OP16_MAX};
    h = __builtin_elementwise_minimum(__builtin_elementwise_maximum(h, -m), m);
  }
  return __builtin_bit_cast(uint32_t, h);
}
__device__ __forceinline__ bf16_t f2bf(float f) {  // round-to-nearest-even, NaN preserved
  if constexpr (MG_F16) return (bf16_t)(cvt_pk_bf16_f32(f, 0.f) & 0xffffu);
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  if constexpr (MG_F16) return cvt_pk_bf16_f32(lo, hi);
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}
__device__ __forceinline__ float bflo(uint32_t w) {
  if constexpr (MG_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
  else return __uint_as_float(w << 16);
}
__device__ __forceinline__ float bfhi(uint32_t w) {
  if constexpr (MG_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
  else return __uint_as_float(w & 0xffff0000u);
}
constexpr uint32_t MG_OP16_ONE_X2 = MG_F16 ? 0x3c003c00u : 0x3f803f80u;   // (1.0, 1.0) as packed operands
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }
// GELU (diffusers GEGLU: F.gelu, exact-erf form) with the Gaussian CDF as an odd polynomial, Phi(x) = 1/2 + x P(x^2) on |x| <= 4 (degree 6 in x^2,
// |error| <= 1.1e-4 on Phi, <= 4e-4 on x Phi(x) inside the interval - an eighth of a bf16 rounding step of the result -
// and <= 1e-4 relative beyond it, where x is clamped): 11 full-rate VALU operations, no transcendental.  The GEGLU
// epilogue of the K = 320 projection issues more VALU than its K loop issues MFMAs; this is its cheapest form.
__device__ __forceinline__ float gelu_poly_f(float x) {
  const float xc = __builtin_amdgcn_fmed3f(x, -4.0f, 4.0f);
  const float t = xc * xc;
  float p = __builtin_fmaf(2.816104822e-08f, t, -1.891892127e-06f);
  p = __builtin_fmaf(p, t, 5.419045219e-05f);
  p = __builtin_fmaf(p, t, -8.789814671e-04f);
  p = __builtin_fmaf(p, t, 9.112954036e-03f);
  p = __builtin_fmaf(p, t, -6.538836045e-02f);
  p = __builtin_fmaf(p, t, 3.985269148e-01f);
  const float phi = fmaxf(__builtin_fmaf(xc, p, 0.5f), 0.0f);
  return x * phi;
}

// lane^32 regroup used by the MFMA epilogues: every lane holds two values g0, g1 (accumulator
// groups g and g+1 of its 32-lane half); afterwards `lo` = what the lower-half lane of the pair owns
// first, i.e. for lanes 0-31: (own g0, partner's g0), for lanes 32-63: (partner's g1, own g1).
// One v_permlane32_swap_b32 (VALU, no LDS traffic).
__device__ __forceinline__ void half_swap(float g0, float g1, float& first, float& second) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(g0), __float_as_uint(g1), false, false);
  first = __uint_as_float(r[0]);
  second = __uint_as_float(r[1]);
}

// ---- the steps the GEMM, convolution and attention epilogues share: 8 consecutive channels of one row per lane ----
// eight fp32 -> the 16 bytes of one store (cvt_pk_bf16_f32's rounding and fp16 saturation), and back
__device__ __forceinline__ uint4 mg_pack8(const float (&v)[8]) {
  uint4 pk;
  pk.x = cvt_pk_bf16_f32(v[0], v[1]); pk.y = cvt_pk_bf16_f32(v[2], v[3]);
  pk.z = cvt_pk_bf16_f32(v[4], v[5]); pk.w = cvt_pk_bf16_f32(v[6], v[7]);
  return pk;
}
__device__ __forceinline__ void mg_unpack8(const uint4 w, float (&v)[8]) {
  v[0] = bflo(w.x); v[1] = bfhi(w.x); v[2] = bflo(w.y); v[3] = bfhi(w.y);
  v[4] = bflo(w.z); v[5] = bfhi(w.z); v[6] = bflo(w.w); v[7] = bfhi(w.w);
}
// two vectors of four fp32 (float4 from memory, f32x4 from an LDS read) as one array
template <class V4>
__device__ __forceinline__ void mg_join8(const V4 lo, const V4 hi, float (&v)[8]) {
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
  v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}
__device__ __forceinline__ void mg_load8(const float* p, float (&v)[8]) {   // p: 16-byte aligned
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  mg_join8(lo, hi, v);
}
// v += eight values: two fp32 vectors (bias, time-embedding row, split-K partials) or eight packed operands (the residual).  Each
// word is unpacked next to its add, as the epilogues were written by hand: hipcc's schedule follows the source order.
template <class V4>
__device__ __forceinline__ void mg_add8(float (&v)[8], const V4 lo, const V4 hi) {
  v[0] += lo.x; v[1] += lo.y; v[2] += lo.z; v[3] += lo.w;
  v[4] += hi.x; v[5] += hi.y; v[6] += hi.z; v[7] += hi.w;
}
__device__ __forceinline__ void mg_add8(float (&v)[8], const float* p) {   // p: 16-byte aligned
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  mg_add8(v, lo, hi);
}
__device__ __forceinline__ void mg_add8(float (&v)[8], const uint4 w) {
  v[0] += bflo(w.x); v[1] += bfhi(w.x); v[2] += bflo(w.y); v[3] += bfhi(w.y);
  v[4] += bflo(w.z); v[5] += bfhi(w.z); v[6] += bflo(w.w); v[7] += bfhi(w.w);
}
// (sum, sum of squares) of a row in fp64 -> (mean, rstd): fp64 for the cancellation E[x^2] - mean^2 only, 1/sqrt in fp32
// (v_rsq_f32, ~1 ulp).  The row-resident kernels and the tile GEMM's cross-attention epilogue call this; the slot reducer of
// igemm2_body.h (ln_out_finish) spells the same three lines out, because the call changed that kernel family's register
// allocation (docs/history/epilogue_steps.md) - the tables must agree bit for bit whichever kernel wrote them, so the two copies
// change together.  (GroupNorm's finalize in norm.hip is other arithmetic - fp64 1 / sqrt - and not one of these.)
__device__ __forceinline__ float2 mg_row_mean_rstd(double s, double q, double inv_n, float eps) {
  const double mean = s * inv_n;
  const float var = fmaxf((float)__builtin_fma(q, inv_n, -mean * mean), 0.f);
  return make_float2((float)mean, __builtin_amdgcn_rsqf(var + eps));
}
// The softmax of the collapsed cross-attention (2 keys per head): eight scaled scores = 4 (key 0, key 1) pairs of the score
// columns c0 .. c0 + 7 -> four words of packed probabilities; pairs at or beyond sm_cols (padding heads) give zero.
__device__ __forceinline__ uint4 mg_pair_softmax4(const float (&s)[8], int c0, int sm_cols) {
  uint32_t w4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float mx = fmaxf(s[2 * k], s[2 * k + 1]);
    const float e0 = __expf(s[2 * k] - mx), e1 = __expf(s[2 * k + 1] - mx);
    const float inv = 1.0f / (e0 + e1);
    w4[k] = (c0 + 2 * k < sm_cols) ? pack2bf(e0 * inv, e1 * inv) : 0u;
  }
  return make_uint4(w4[0], w4[1], w4[2], w4[3]);
}

__device__ __forceinline__ float silu_fast_f(float x) {  // x * sigmoid(x): one v_exp, one v_rcp
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

// Sum over the 64 lanes of a wave with DPP moves (VALU speed; __shfl_xor goes through the LDS crossbar
// - six dependent ds_bpermute round trips per reduction).  Result is wave-uniform.
__device__ __forceinline__ float wave_sum_f(float v) {
  auto dpp = [](float x, auto ctrl_tag, auto row_mask_tag) {
    constexpr int ctrl = decltype(ctrl_tag)::value, rm = decltype(row_mask_tag)::value;
    return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), ctrl, rm, 0xF, false));
  };
  v += dpp(v, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xF>{});   // quad_perm [1,0,3,2]
  v += dpp(v, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xF>{});   // quad_perm [2,3,0,1]
  v += dpp(v, std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xF>{});  // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xF>{});  // row_mirror: 16-lane row sums
  v += dpp(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});  // row_bcast15 -> rows 1, 3
  v += dpp(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});  // row_bcast31 -> rows 2, 3
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}

// 16-byte async global -> LDS copy.  LDS destination = wave-uniform base + lane*16.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gsrc, (LDS_AS void*)lds_wave_base, 16, 0,
                                   0);
}

// Bijective XCD-aware remap of a linear workgroup id: consecutive remapped ids live on the
// same XCD (hardware places block b on XCD b % 8), so neighbouring tiles share that XCD's L2.
__device__ __forceinline__ int xcd_remap(unsigned bid, unsigned nwg) {
  const unsigned NX = 8;
  const unsigned xcd = bid % NX, idx = bid / NX;
  const unsigned q = nwg / NX, r = nwg % NX;
  const unsigned start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return (int)(start + idx);
}

// Division of x < 2^31 by a launch-time constant d >= 1 in three integer instructions (the compiler's generic 32-bit
// division is ~25, and the GEMM prologue / epilogue run a dozen of them per thread - measured: half of the instructions a
// short-K tile executes).  L = ceil(log2 d), m = ceil(2^(31+L) / d) < 2^32: floor(x / d) = (x * m) >> (31 + L) exactly,
// since the error term x * (m d - 2^(31+L)) < 2^31 * d <= 2^(31+L).  Written as umulhi(2x, m) >> L so that d = 1 needs no case.
struct mg_fastdiv {
  uint32_t m, l;
};
inline mg_fastdiv mg_make_fastdiv(long long d) {
  mg_fastdiv f;
  uint32_t l = 0;
  while ((1ull << l) < (unsigned long long)d) ++l;
  f.l = l;
  f.m = (uint32_t)(((1ull << (31 + l)) + (unsigned long long)d - 1) / (unsigned long long)d);   // d < 2^31: l <= 31
  return f;
}
__device__ __forceinline__ int fdiv(int x, const mg_fastdiv f) { return (int)(__umulhi((uint32_t)x << 1, f.m) >> f.l); }

// Cross-workgroup hand-offs inside one launch (the row-statistics tickets of igemm2_body.h, GroupNorm's last-block finalize in
// norm.hip, the key pieces of flash4w.hip).  The product form is the write-through one of cdna_hip_programming.md Guideline 16 /
// MI355X_MICROARCH.md "valid forms": 16-byte / 8-byte sc1 stores of the payload -> every storing wave drains vmcnt ->
// __syncthreads -> ONE relaxed agent-scope ticket; the last arriver reads the payload with sc1 loads ("sc1 loads may replace the
// acquire only when the producer stored sc1").  MG_HANDOFF_FENCES (Makefile: HANDOFF_FENCES=1) adds the C++-memory-model form on
// top - an agent-scope release fence in front of the ticket, an acquire fence in the last arriver - for same-box A/B runs of what
// that costs (profiles/r6_ab_handoff_fences.log).
constexpr bool MG_HANDOFF_FENCES = MG_HANDOFF_FENCES_BUILD != 0;
__device__ __forceinline__ void mg_handoff_release() {   // lane 0, behind the workgroup barrier that follows the drained stores
  if constexpr (MG_HANDOFF_FENCES) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (ROCm 7.2 may drop the wait behind buffer_wbl2: restated where it cannot)
  }
}
__device__ __forceinline__ void mg_handoff_acquire() {   // the last arriver's lane 0, in front of the barrier that releases its readers
  if constexpr (MG_HANDOFF_FENCES) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// The ticket itself, drawn by ONE lane of the workgroup behind that barrier: true for the last of `total` arrivers, which has
// then also put the counter back to zero for the next launch (stream-ordered).  The caller keeps what surrounds it: the vmcnt
// drain and barrier in front, the LDS broadcast of the answer and the barrier behind.
__device__ __forceinline__ bool mg_draw_last_ticket(unsigned* counter, unsigned total) {
  mg_handoff_release();
  const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = ticket == total - 1;
  if (last) {
    mg_handoff_acquire();
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return last;
}

#define MG_ZERO_BYTES (128 * 1024)
extern void* g_zero_page;  // MG_ZERO_BYTES zero bytes in device memory (mg_init): padding source
// Dry run (mg_program_validate): every launcher checks its op's shape / alignment contract and
// returns before touching the device - the CPU test-suite validates full-size programs with it.
extern thread_local bool g_dry_run;
#define MG_SPLITK_WS_BYTES (64ll * 1024 * 1024)
#define MG_LN_COUNTERS 65536
extern unsigned* g_ln_counters;  // MG_LN_COUNTERS zeroed tickets (mg_init): one per row block of a GEMM launch that writes row
                                 // statistics (the last column tile of a row block reduces them); self-resetting, stream-ordered
extern void* g_splitk_ws;  // fp32 partial sums of split-K GEMM launches (mg_init); stream-ordered reuse
#define MG_LAUNCH(...)                                   \
  do {                                                   \
    if (!g_dry_run) hipLaunchKernelGGL(__VA_ARGS__);     \
  } while (0)
void mg_set_error(const char* fmt, ...);
// Tuning switch `name` (an environment variable) if MARIGOLD_TUNING=1, else `dflt`: the library's only access to the
// environment (runtime.hip).  Deployments run the compiled-in defaults.
int mg_tuning_int(const char* name, int dflt);
#define MG_CHECK_HIP(expr)                                                         \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) {                                                        \
      mg_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return 1;                                                                    \
    }                                                                              \
  } while (0)
// Once per kernel, before its launch: raise `kern`'s hipFuncAttributeMaxDynamicSharedMemorySize to `bytes` (runtime.hip, over
// kernel_once.h).  Safe when several host threads make the first launch of the same or different kernels at once; the attribute is
// set at most once per size, a larger request raises it; a failure is reported (mg_set_error, -> 1) and tried again by the next
// launch; under g_dry_run nothing is set or recorded.  `no_static_lds`: refuse (-> 2), in the same once-only step, a kernel whose
// static LDS is not empty - its dynamic LDS must start at address 0.
int mg_kernel_max_lds(const void* kern, int bytes, bool no_static_lds = false);
#define MG_KERNEL_MAX_LDS(...)                                   \
  do {                                                           \
    if (const int _rc = mg_kernel_max_lds(__VA_ARGS__)) return _rc; \
  } while (0)
int mg_cu_count();   // compute units of the device mg_init bound; 256 (MI355X) before mg_init
#define MG_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      mg_set_error(__VA_ARGS__);   \
      return 2;                    \
    }                              \
  } while (0)

// launchers (one per .hip file)
int mg_launch_igemm(const mg_op* op, hipStream_t s);
int mg_launch_igemm2(const mg_op* op, hipStream_t s, int variant);  // -1: shape outside the kernel's contract
int mg_launch_conv_patch(const mg_op* op, hipStream_t s);
int mg_conv3x3_gn_slots_of(const mg_op* op);
int mg_launch_rowgemm(const mg_op* op, hipStream_t s);
int mg_launch_norm(const mg_op* op, hipStream_t s);
int mg_launch_attention(const mg_op* op, hipStream_t s);
int mg_launch_flash512(const mg_op* op, hipStream_t s);
int mg_launch_misc(const mg_op* op, hipStream_t s);
int mg_launch_head_conv(const mg_op* op, hipStream_t s);
int mg_launch_ensemble(const mg_op* op, hipStream_t s);
int mg_launch_resize(const mg_op* op, hipStream_t s);
int mg_launch_evalscore(const mg_op* op, hipStream_t s);
int mg_launch_randn(const mg_op* op, hipStream_t s);
