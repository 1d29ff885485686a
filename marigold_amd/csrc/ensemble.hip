// On-device test-time ensembling (reference: marigold/util/ensemble.py).
//
// Depth (ensemble_depth :39-196).  The reference evaluates, per BFGS cost call, E(E-1)/2
// pairwise RMSE reductions with one .item() sync each (:142-144) plus a median (:147-150).
// Here:
//   * DEPTH_STATS makes ONE pass set over the members and produces per-member min/max/mean
//     and the centred second-moment matrix C (E x E, fp64).  With a_i = s_i d_i + t_i,
//       mean((a_i - a_j)^2) = s_i^2 C_ii + s_j^2 C_jj - 2 s_i s_j C_ij + (s_i m_i + t_i - s_j m_j - t_j)^2
//     so the pairwise term of the cost - and its exact gradient - is O(E^2) host arithmetic.
//   * DEPTH_MEDIAN is the only per-evaluation pixel work: align -> lower-middle median over E
//     (torch.median semantics, :129) -> global min/max (regulariser, :146-150); the same kernel
//     writes the final median / MAD maps (:178-182).
//   * DEPTH_NORM applies the final min/max normalisation (:184-194) from device-resident
//     scalars (no host sync).
// Normals (ensemble_normals :199-249): one fused per-pixel kernel (mean -> normalise -> cosine
// -> arccos mean / pi -> argmax -> gather).
// Intrinsic images (ensemble_iid :252-270): IID is DEPTH_MEDIAN's reduction over the members alone, per element.
// All HBM-bound streaming kernels: E*HW*4 B read per pass, coalesced over pixels.
// What the kernels share is written once: the reduction over the members of one element (reduce_members for members in registers,
// reduce_members_mem - rank count, bitwise selection, mean / std - for members in LDS or memory), the block's extrema
// (store_block_extrema), the wave's (wave_extrema, under either order) and the ladder of register bounds (with_member_bound).
// tests/golden/ensemble_bits.json holds a digest of every output of every kernel form.
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "common.h"

namespace {

constexpr int EMAX = 32;        // members a thread keeps in registers (selection kernels) / columns per second-moment block
constexpr int EMAX_LDS = 128;   // members of the LDS-resident selection (33 ... 128: any size the reference's users ask for in
                                // practice - it warns above 15, script/depth/run.py:143-144); beyond: depth_median_big_kernel
                                // (bitwise selection straight from memory - the reference accepts ANY ensemble size)
constexpr int ENS_BLOCKS = 512;

// grid (nblk, E, column chunks of 32): block (x, i, jc) accumulates columns [32 jc, 32 jc + 32) of row i of the raw
// second-moment matrix; partial layout [block x][row i][3 + E] (min, max, sum, row of the matrix)
__global__ __launch_bounds__(256) void depth_stats_kernel(const float* __restrict__ d0, double* __restrict__ part,
                                                          int Etot, long long HW) {
  __shared__ double red[4][EMAX + 3];
  const int i = blockIdx.y;
  const int j0 = blockIdx.z * EMAX;
  const int E = min(EMAX, Etot - j0);            // columns of this block
  const float* __restrict__ d = d0 + (long long)j0 * HW;
  const float* __restrict__ di_row = d0 + (long long)i * HW;
  float acc[EMAX];
#pragma unroll
  for (int j = 0; j < EMAX; ++j) acc[j] = 0.f;
  float mn = __builtin_inff(), mx = -__builtin_inff();   // (min / max keep NaN, like the reference's flat.min() / .max())
  double sum = 0.0;
  // fp32 partials over short strides, promoted to fp64 every 64 pixels per thread
  double accd[EMAX];
#pragma unroll
  for (int j = 0; j < EMAX; ++j) accd[j] = 0.0;
  int cnt = 0;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
    const float di = di_row[p];
    mn = min_keep_nan(mn, di);
    mx = max_keep_nan(mx, di);
    sum += (double)di;
#pragma unroll
    for (int j = 0; j < EMAX; ++j)
      if (j < E) acc[j] += di * d[(long long)j * HW + p];
    if (++cnt == 64) {
#pragma unroll
      for (int j = 0; j < EMAX; ++j) { accd[j] += (double)acc[j]; acc[j] = 0.f; }
      cnt = 0;
    }
  }
#pragma unroll
  for (int j = 0; j < EMAX; ++j) accd[j] += (double)acc[j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min_keep_nan(mn, __shfl_xor(mn, o));
    mx = max_keep_nan(mx, __shfl_xor(mx, o));
    sum += __shfl_xor(sum, o);
#pragma unroll
    for (int j = 0; j < EMAX; ++j)
      if (j < E) accd[j] += __shfl_xor(accd[j], o);
  }
  if (lane == 0) {
    red[wave][0] = (double)mn; red[wave][1] = (double)mx; red[wave][2] = sum;
#pragma unroll
    for (int j = 0; j < EMAX; ++j)
      if (j < E) red[wave][3 + j] = accd[j];
  }
  __syncthreads();
  double* o = part + ((long long)blockIdx.x * Etot + i) * (Etot + 3);
  for (int k = threadIdx.x; k < E + 3; k += 256) {
    double v;
    if (k == 0) v = (double)min_keep_nan(min_keep_nan((float)red[0][0], (float)red[1][0]), min_keep_nan((float)red[2][0], (float)red[3][0]));   // (floats, held as doubles: exact)
    else if (k == 1) v = (double)max_keep_nan(max_keep_nan((float)red[0][1], (float)red[1][1]), max_keep_nan((float)red[2][1], (float)red[3][1]));
    else v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    if (k < 3) { if (j0 == 0) o[k] = v; }       // min / max / sum of row i: once
    else o[3 + j0 + (k - 3)] = v;
  }
}

// one block; out = [min[E], max[E], mean[E], C[E][E]] (C centred)
__global__ __launch_bounds__(256) void depth_stats_final_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                                int E, int nblk, long long HW) {
  // the member means: out[2E ..), written by this (single) block below and read back after the barrier
  double* const mean_s = out + 2 * E;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < E * 3; idx += 256) {
    const int i = idx / 3, k = idx % 3;
    double v = (k == 0) ? (double)__builtin_inff() : (k == 1 ? -(double)__builtin_inff() : 0.0);
    for (int b = 0; b < nblk; ++b) {
      const double x = part[((long long)b * E + i) * (E + 3) + k];
      if (k == 0) v = (double)min_keep_nan((float)v, (float)x);   // (the members' own floats: exact)
      else if (k == 1) v = (double)max_keep_nan((float)v, (float)x);
      else v += x;
    }
    if (k == 0) out[i] = v;
    else if (k == 1) out[E + i] = v;
    else mean_s[i] = v / (double)HW;
  }
  __threadfence_block();
  __syncthreads();
  for (int idx = tid; idx < E * E; idx += 256) {
    const int i = idx / E, j = idx % E;
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += part[((long long)b * E + i) * (E + 3) + 3 + j];   // same order as before: b ascending
    out[3 * E + idx] = v / (double)HW - mean_s[i] * mean_s[j];
  }
}

template <int E_>
__device__ __forceinline__ float select_rank(const float (&a)[E_], int E, int k) {
  float res = a[0];
#pragma unroll
  for (int e = 0; e < E_; ++e) {
    if (e < E) {
      int rank = 0;
#pragma unroll
      for (int j = 0; j < E_; ++j)
        if (j < E) rank += (a[j] < a[e]) || (a[j] == a[e] && j < e);
      if (rank == k) res = a[e];
    }
  }
  return res;
}

// The benchmark's ensemble size: k-th smallest of <= 10 values through the 29-comparator sorting network (Knuth, TAOCP 3, n = 10;
// 58 min / max against ~300 compare / add of the rank count above).  Entries past E are +inf; the VALUE of rank k under
// (value, index) order is the k-th order statistic, whichever way ties are broken.  torch.median propagates NaN and so does the
// network: its comparators are IEEE minimum / maximum (v_minimum3_f32 / v_maximum3_f32, the price of v_min_f32 / v_max_f32), which
// return NaN on both wires when either input is one - and every output of a sorting network is reached from every input.
__device__ __forceinline__ float select_kth10(const float (&v)[10], int E, int k) {
  float a[10];
#pragma unroll
  for (int e = 0; e < 10; ++e) a[e] = e < E ? v[e] : __builtin_inff();
#define MG_CE(i, j) { const float lo = min_keep_nan(a[i], a[j]), hi = max_keep_nan(a[i], a[j]); a[i] = lo; a[j] = hi; }
  MG_CE(4, 9) MG_CE(3, 8) MG_CE(2, 7) MG_CE(1, 6) MG_CE(0, 5) MG_CE(1, 4) MG_CE(6, 9) MG_CE(0, 3) MG_CE(5, 8) MG_CE(0, 2)
  MG_CE(3, 6) MG_CE(7, 9) MG_CE(0, 1) MG_CE(2, 4) MG_CE(5, 7) MG_CE(8, 9) MG_CE(1, 2) MG_CE(4, 6) MG_CE(7, 8) MG_CE(3, 5)
  MG_CE(2, 5) MG_CE(6, 8) MG_CE(1, 3) MG_CE(4, 7) MG_CE(2, 3) MG_CE(6, 7) MG_CE(3, 4) MG_CE(5, 6) MG_CE(4, 5)
#undef MG_CE
  float r = a[0];
#pragma unroll
  for (int e = 1; e < 10; ++e)
    if (e == k) r = a[e];
  return r;
}
// torch.median propagates NaN: a NaN among the members makes the order statistic NaN.  The rank count would not (its < and == are
// false on a NaN), so a NaN test stands beside it: one unordered compare per PAIR of values (entries past E are numbers),
// branch-free, the count itself unchanged.
template <int E_>
__device__ __forceinline__ bool any_nan(const float (&a)[E_]) {
  static_assert(E_ % 2 == 0, "any_nan: pairs");
  bool r = false;
#pragma unroll
  for (int e = 0; e < E_; e += 2) r |= __builtin_isunordered(a[e], a[e + 1]);
  return r;
}
template <int E_>
__device__ __forceinline__ float select_kth(const float (&a)[E_], int E, int k) {
  if constexpr (E_ == 10) return select_kth10(a, E, k);
  else return any_nan<E_>(a) ? __builtin_nanf("") : select_rank<E_>(a, E, k);
}

// ---- the reduction over the members of one element (a pixel of the depth map, an element of an intrinsic-image target), written
// once per place the members live in.  reduction 0: the lower-middle median (torch.median) and, where asked for, the median
// absolute deviation about it; 1: the mean and the unbiased standard deviation (torch.std).  The members are added in index order,
// every operation is rounded on its own (this file is built without FMA contraction), and a NaN member makes every statistic NaN.
// Every kernel below that reduces over members calls one of the two functions, so a correction is made here and nowhere else.

// The members in registers: a[0 .. E) of E_ (entries past E are numbers: the callers store 0).
template <int E_>
__device__ __forceinline__ void reduce_members(const float (&a)[E_], int E, int reduction, bool want_unc, float& pred, float& unc) {
  const int k = (E - 1) >> 1;   // torch.median: lower middle
  unc = 0.f;
  if (reduction == 0) {
    pred = select_kth<E_>(a, E, k);
    if (want_unc) {
      float dv[E_];
#pragma unroll
      for (int e = 0; e < E_; ++e) dv[e] = fabsf(__fsub_rn(a[e], pred));
      unc = select_kth<E_>(dv, E, k);
    }
  } else {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E_; ++e)
      if (e < E) s += a[e];
    pred = s / (float)E;
    if (want_unc) {
      float q = 0.f;
#pragma unroll
      for (int e = 0; e < E_; ++e)
        if (e < E) { const float dd = a[e] - pred; q += dd * dd; }
      unc = sqrtf(q / (float)(E > 1 ? E - 1 : 1));   // torch.std: unbiased
    }
  }
}

// The members behind an accessor - more of them than a thread keeps in registers: member(e) reads member e of the element from LDS
// or from memory (cache-resident after the first pass), as often as the selection asks for it.  The deviations |member - centre| of
// the second selection are formed on the fly (a second array would fit neither place).
// Element of rank k by counting ranks, ties broken by the member index (as select_rank): O(E^2).  torch.median: a NaN member makes
// the statistic NaN, and the count would not (its < and == are false on a NaN), so a flag stands beside it.
template <class Member>
__device__ __forceinline__ float select_by_rank(const Member& member, int E, int k, bool dev, float centre) {
  auto val = [&](int e) { const float x = member(e); return dev ? fabsf(__fsub_rn(x, centre)) : x; };
  float res = val(0);
  bool nan = false;
  for (int e = 0; e < E; ++e) {
    const float ve = val(e);
    nan |= ve != ve;
    int rank = 0;
    for (int j = 0; j < E; ++j) {
      const float vj = val(j);
      rank += (vj < ve) || (vj == ve && j < e);
    }
    if (rank == k) res = ve;
  }
  return nan ? __builtin_nanf("") : res;
}
// The same element by a bitwise selection: 32 counting passes over the E values (monotone float -> uint32 key, most significant bit
// first), O(32 E) instead of O(E^2).  The VALUE of rank k does not depend on how ties are broken, and its sign comes out of the key
// (where the statistic falls among zeros of both signs: -0 sorts before +0).  A NaN would sort past +-inf as a key: a pass of its
// own looks for one first.
template <class Member>
__device__ __forceinline__ float select_by_bits(const Member& member, int E, int k, bool dev, float centre) {
  auto val = [&](int e) { const float x = member(e); return dev ? fabsf(__fsub_rn(x, centre)) : x; };
  auto key_of = [](float x) { const unsigned b = __float_as_uint(x); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); };
  auto val_of = [](unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); };
  bool nan = false;
  for (int e = 0; e < E; ++e) {
    const float v = val(e);
    nan |= v != v;
  }
  unsigned prefix = 0;
  int kk = k;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned hi_mask = bit == 31 ? 0u : ~((2u << bit) - 1u);   // the bits already decided
    int cnt0 = 0;
    for (int e = 0; e < E; ++e) {
      const unsigned key = key_of(val(e));
      cnt0 += ((key & hi_mask) == prefix && !((key >> bit) & 1u)) ? 1 : 0;
    }
    if (kk >= cnt0) { kk -= cnt0; prefix |= 1u << bit; }
  }
  return nan ? __builtin_nanf("") : val_of(prefix);
}
// by_rank: which of the two selections (the callers' choice by E; both give the same value)
template <class Member>
__device__ __forceinline__ void reduce_members_mem(const Member& member, int E, bool by_rank, int reduction, bool want_unc, float& pred,
                                                   float& unc) {
  const int k = (E - 1) >> 1;   // torch.median: lower middle
  auto select = [&](bool dev, float centre) {
    return by_rank ? select_by_rank(member, E, k, dev, centre) : select_by_bits(member, E, k, dev, centre);
  };
  unc = 0.f;
  if (reduction == 0) {
    pred = select(false, 0.f);
    if (want_unc) unc = select(true, pred);
  } else {
    float s = 0.f;
    for (int e = 0; e < E; ++e) s += member(e);
    pred = s / (float)E;
    if (want_unc) {
      float q = 0.f;
      for (int e = 0; e < E; ++e) { const float dd = member(e) - pred; q += dd * dd; }
      unc = sqrtf(q / (float)(E > 1 ? E - 1 : 1));   // torch.std: unbiased
    }
  }
}

// ---- the running (value, pixel) extrema of a map: (min, its pixel, max, its pixel), merged under one of two orders
struct NumberOrder {   // numbers only (no NaN among the candidates): ties go to the lowest pixel
  static __device__ __forceinline__ bool min(float o, long long op, float m, long long p) { return o < m || (o == m && op < p); }
  static __device__ __forceinline__ bool max(float o, long long op, float m, long long p) { return o > m || (o == m && op < p); }
};
struct NanFirstOrder {   // a NaN beats every number (common.h: takes_min / takes_max)
  static __device__ __forceinline__ bool min(float o, long long op, float m, long long p) { return takes_min(o, op, m, p); }
  static __device__ __forceinline__ bool max(float o, long long op, float m, long long p) { return takes_max(o, op, m, p); }
};
// the extrema of a wave's 64 lanes, in every lane
template <class Order>
__device__ __forceinline__ void wave_extrema(float& mn_io, float& mx_io, long long& pmn_io, long long& pmx_io) {
  // (on copies: the conditional assignments below are selects on registers, not branches around stores through a reference)
  float mn = mn_io, mx = mx_io;
  long long pmn = pmn_io, pmx = pmx_io;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float omn = __shfl_xor(mn, o), omx = __shfl_xor(mx, o);
    const long long opmn = __shfl_xor(pmn, o), opmx = __shfl_xor(pmx, o);
    if (Order::min(omn, opmn, mn, pmn)) { mn = omn; pmn = opmn; }
    if (Order::max(omx, opmx, mx, pmx)) { mx = omx; pmx = opmx; }
  }
  mn_io = mn; mx_io = mx; pmn_io = pmn; pmx_io = pmx;
}
// The tail of the three median kernels (256 threads; every thread calls it): the block's extrema - wave shuffle, four-wave merge in
// LDS - into its row of the per-block tables that minmax_final_kernel scans.
__device__ __forceinline__ void store_block_extrema(float mn, float mx, long long pmn, long long pmx, float* __restrict__ blockmm,
                                                    long long* __restrict__ blockpx) {
  __shared__ float red[8];
  __shared__ long long redp[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_extrema<NanFirstOrder>(mn, mx, pmn, pmx);
  if (lane == 0) { red[wave] = mn; red[4 + wave] = mx; redp[wave] = pmn; redp[4 + wave] = pmx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      if (takes_min(red[w], redp[w], red[0], redp[0])) { red[0] = red[w]; redp[0] = redp[w]; }
      if (takes_max(red[4 + w], redp[4 + w], red[4], redp[4])) { red[4] = red[4 + w]; redp[4] = redp[4 + w]; }
    }
    blockmm[2 * blockIdx.x] = red[0];
    blockmm[2 * blockIdx.x + 1] = red[4];
    blockpx[2 * blockIdx.x] = redp[0];
    blockpx[2 * blockIdx.x + 1] = redp[4];
  }
}

// E_ = compile-time upper bound of E (registers); st = [s[E], t[E]] fp32; reduction 0 median 1 mean
template <int E_>
__global__ __launch_bounds__(256) void depth_median_kernel(const float* __restrict__ d, const float* __restrict__ st,
                                                           float* __restrict__ med, float* __restrict__ mad,
                                                           float* __restrict__ blockmm, long long* __restrict__ blockpx,
                                                           int E, long long HW,
                                                           int reduction, int has_shift, int aligned) {
  long long pmn = 0, pmx = 0;
  float sc[E_], sh[E_];
#pragma unroll
  for (int e = 0; e < E_; ++e) {
    sc[e] = (aligned && e < E) ? st[e] : 1.f;
    sh[e] = (aligned && has_shift && e < E) ? st[E + e] : 0.f;
    // keep the 2 E_ parameters in vector registers: as scalars they compete with the loops' condition masks, and once they no
    // longer fit the compiler parks them in VGPR lanes and reads each back (v_readlane + wait states) before every use
    asm volatile("" : "+v"(sc[e]), "+v"(sh[e]));
  }
  float mn = __builtin_inff(), mx = -__builtin_inff();
  auto pixel = [&](const float (&raw)[E_], long long p, float& pred, float& unc) {
    float a[E_];
#pragma unroll
    for (int e = 0; e < E_; ++e)   // reference: depth * s + t as two separately rounded fp32 ops (ensemble.py:112)
      a[e] = e < E ? (aligned ? __fadd_rn(__fmul_rn(raw[e], sc[e]), sh[e]) : raw[e]) : 0.f;
    reduce_members<E_>(a, E, reduction, mad != nullptr, pred, unc);
    if (pred < mn) { mn = pred; pmn = p; }
    if (pred > mx) { mx = pred; pmx = p; }
  };
  // a NaN prediction makes min and max NaN (torch's .min() / .max()): both comparisons above are false on it, so the loops only
  // note that one occurred - an IEEE minimum over the predictions, which a NaN poisons: vector operations on one register, no
  // condition mask held across the loop (this pass runs ~100 times per map and is short of scalar registers) - and the thread's
  // extrema become NaN after them.  The members reported beside NaN extrema are those of pixel 0: the regulariser's sub-gradient
  // means nothing on a NaN cost.
  float nan_acc = 0.f;
  // four consecutive pixels per thread and pass (16-byte loads, E of them in flight): the optimiser calls this pass ~100 times
  // per map and as one pixel per thread it was 4-5 dependent HBM round trips long (19 us for 23.6 MB; round 3)
  const long long HW4 = (HW & 3) == 0 && (((uintptr_t)d | (uintptr_t)med | (uintptr_t)mad) & 15) == 0 ? HW : 0;
  for (long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; p < HW4; p += (long long)gridDim.x * 1024) {
    float4 v[E_];
#pragma unroll
    for (int e = 0; e < E_; ++e) v[e] = e < E ? *(const float4*)(d + (long long)e * HW + p) : make_float4(0.f, 0.f, 0.f, 0.f);
    float pr[4], un[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float raw[E_];
#pragma unroll
      for (int e = 0; e < E_; ++e) raw[e] = i == 0 ? v[e].x : (i == 1 ? v[e].y : (i == 2 ? v[e].z : v[e].w));
      pixel(raw, p + i, pr[i], un[i]);
    }
    nan_acc = min_keep_nan(min_keep_nan(nan_acc, pr[0]), min_keep_nan(min_keep_nan(pr[1], pr[2]), pr[3]));
    if (med) *(float4*)(med + p) = make_float4(pr[0], pr[1], pr[2], pr[3]);
    if (mad) *(float4*)(mad + p) = make_float4(un[0], un[1], un[2], un[3]);
  }
  for (long long p = HW4 + (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
    float raw[E_];
#pragma unroll
    for (int e = 0; e < E_; ++e) raw[e] = e < E ? d[(long long)e * HW + p] : 0.f;
    float pred, unc;
    pixel(raw, p, pred, unc);
    nan_acc = min_keep_nan(nan_acc, pred);
    if (med) med[p] = pred;
    if (mad) mad[p] = unc;
  }
  if (nan_acc != nan_acc) { mn = mx = nan_acc; pmn = pmx = 0; }
  store_block_extrema(mn, mx, pmn, pmx, blockmm, blockpx);
}

// 33 ... 128 members: the aligned values of a pixel live in LDS ([member][thread]: conflict-free), the lower-middle order
// statistic is found by counting ranks (O(E^2) per pixel - large ensembles are rare and the pass stays HBM-light).
// Same semantics, same outputs as depth_median_kernel.
__global__ __launch_bounds__(256) void depth_median_lds_kernel(const float* __restrict__ d, const float* __restrict__ st,
                                                               float* __restrict__ med, float* __restrict__ mad,
                                                               float* __restrict__ blockmm, long long* __restrict__ blockpx,
                                                               int E, long long HW, int reduction, int has_shift, int aligned) {
  extern __shared__ float lds_a[];   // [E][256] aligned values (128 KB at E = 128), then [2 E] scale / shift
  const int tid = threadIdx.x;
  float* a = lds_a + tid;
  float* sc = lds_a + (long long)E * 256;
  for (int e = tid; e < E; e += 256) {
    sc[e] = aligned ? st[e] : 1.f;
    sc[E + e] = (aligned && has_shift) ? st[E + e] : 0.f;
  }
  __syncthreads();
  long long pmn = 0, pmx = 0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  bool saw_nan = false;
  auto member = [&](int e) { return a[e * 256]; };
  for (long long p = (long long)blockIdx.x * 256 + tid; p < HW; p += (long long)gridDim.x * 256) {
    for (int e = 0; e < E; ++e) {
      const float v = d[(long long)e * HW + p];
      a[e * 256] = aligned ? __fadd_rn(__fmul_rn(v, sc[e]), sc[E + e]) : v;
    }
    float pred, unc;
    reduce_members_mem(member, E, true, reduction, mad != nullptr, pred, unc);
    if (med) med[p] = pred;
    if (mad) mad[p] = unc;
    if (pred < mn) { mn = pred; pmn = p; }
    if (pred > mx) { mx = pred; pmx = p; }
    saw_nan |= pred != pred;   // NaN extrema, pixel 0: as depth_median_kernel
  }
  if (saw_nan) { mn = mx = __builtin_nanf(""); pmn = pmx = 0; }
  store_block_extrema(mn, mx, pmn, pmx, blockmm, blockpx);
}

// More than 128 members (the reference takes any ensemble size, marigold/util/ensemble.py:39-49): the members' values are read
// straight from memory and aligned at every read, the order statistic is found by the bitwise selection - no per-pixel storage.
// Same semantics and outputs as depth_median_kernel.
__global__ __launch_bounds__(256) void depth_median_big_kernel(const float* __restrict__ d, const float* __restrict__ st,
                                                               float* __restrict__ med, float* __restrict__ mad,
                                                               float* __restrict__ blockmm, long long* __restrict__ blockpx,
                                                               int E, long long HW, int reduction, int has_shift, int aligned) {
  const int tid = threadIdx.x;
  long long pmn = 0, pmx = 0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  bool saw_nan = false;
  for (long long p = (long long)blockIdx.x * 256 + tid; p < HW; p += (long long)gridDim.x * 256) {
    auto member = [&](int e) {   // reference: depth * s + t as two separately rounded fp32 ops (ensemble.py:112)
      const float v = d[(long long)e * HW + p];
      return aligned ? __fadd_rn(__fmul_rn(v, st[e]), has_shift ? st[E + e] : 0.f) : v;
    };
    float pred, unc;
    reduce_members_mem(member, E, false, reduction, mad != nullptr, pred, unc);
    if (med) med[p] = pred;
    if (mad) mad[p] = unc;
    if (pred < mn) { mn = pred; pmn = p; }
    if (pred > mx) { mx = pred; pmx = p; }
    saw_nan |= pred != pred;   // NaN extrema, pixel 0: as depth_median_kernel
  }
  if (saw_nan) { mn = mx = __builtin_nanf(""); pmn = pmx = 0; }
  store_block_extrema(mn, mx, pmn, pmx, blockmm, blockpx);
}

// out = [min, max, d[0..E)[argmin px], d[0..E)[argmax px]]  (raw member values at the extremal
// pixels of the prediction: the host derives the exact sub-gradient of the regulariser from them)
__global__ __launch_bounds__(64) void minmax_final_kernel(const float* __restrict__ blockmm,
                                                          const long long* __restrict__ blockpx,
                                                          const float* __restrict__ d, float* __restrict__ out,
                                                          int nblk, int E, long long HW) {
  __shared__ long long px[2];
  // one wave: strided scan of the per-block results, then a lane reduction (ties -> lowest pixel)
  const int lane = threadIdx.x;
  float mn, mx;
  long long pmn, pmx;
  auto scan = [&](auto order) {   // -> whether a block reported a NaN
    mn = __builtin_inff(); mx = -__builtin_inff();
    pmn = pmx = 0x7fffffffffffffffll;
    bool nan = false;
    for (int i = lane; i < nblk; i += 64) {
      const float a = blockmm[2 * i], b = blockmm[2 * i + 1];
      const long long pa = blockpx[2 * i], pb = blockpx[2 * i + 1];
      nan |= __builtin_isunordered(a, b);
      if (order.min(a, pa, mn, pmn)) { mn = a; pmn = pa; }
      if (order.max(b, pb, mx, pmx)) { mx = b; pmx = pb; }
    }
    return nan;
  };
  if (__any(scan(NumberOrder()))) {   // a block saw a NaN prediction: the scan again in the order that puts a NaN first (wave-uniform, rarely taken)
    scan(NanFirstOrder());
    wave_extrema<NanFirstOrder>(mn, mx, pmn, pmx);
  } else {
    wave_extrema<NumberOrder>(mn, mx, pmn, pmx);
  }
  if (lane == 0) {
    out[0] = mn; out[1] = mx;
    px[0] = pmn < HW ? pmn : 0; px[1] = pmx < HW ? pmx : 0;   // (every block reports a pixel of the map; never read past it)
  }
  __syncthreads();
  for (int e = lane; e < E; e += 64) {
    out[2 + e] = d[(long long)e * HW + px[0]];
    out[2 + E + e] = d[(long long)e * HW + px[1]];
  }
}

__global__ __launch_bounds__(256) void depth_norm_kernel(float* __restrict__ med, float* __restrict__ unc,
                                                         const float* __restrict__ mm, long long HW, int shift_inv) {
  const float hi = mm[1];
  const float lo = shift_inv ? mm[0] : 0.f;
  const float rng = floor_keep_nan(hi - lo, 1e-6f);   // (hi - lo).clamp(min=1e-6): NaN extrema make a NaN map, as in the reference
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
    med[p] = (med[p] - lo) / rng;
    if (unc) unc[p] = unc[p] / rng;
  }
}

__global__ __launch_bounds__(256) void normals_kernel(const float* __restrict__ n, float* __restrict__ out,
                                                      float* __restrict__ unc, int E, long long HW, int reduction) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int e = 0; e < E; ++e) {
      const float* q = n + (long long)e * 3 * HW + p;
      sx += q[0]; sy += q[HW]; sz += q[2 * HW];
    }
    float mx_ = sx / (float)E, my = sy / (float)E, mz = sz / (float)E;
    const float nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(mx_, mx_), __fmul_rn(my, my)), __fmul_rn(mz, mz)));
    const float den = floor_keep_nan(nrm, 1e-6f);
    mx_ = mx_ / den; my = my / den; mz = mz / den;
    float best = -2.f, ua = 0.f;
    int bi = 0;
    for (int e = 0; e < E; ++e) {
      const float* q = n + (long long)e * 3 * HW + p;
      float c = __fadd_rn(__fadd_rn(__fmul_rn(mx_, q[0]), __fmul_rn(my, q[HW])), __fmul_rn(mz, q[2 * HW]));
      c = clip_keep_nan(c, -1.f, 1.f);   // NaN cosines: no member is closer than member 0 (torch's argmax), the uncertainty is NaN
      if (c > best) { best = c; bi = e; }
      ua += acosf(c);
    }
    if (unc) unc[p] = ua / (float)E / 3.14159265358979323846f;
    if (reduction == 1) {
      out[p] = mx_; out[HW + p] = my; out[2 * HW + p] = mz;
    } else {
      const float* q = n + (long long)bi * 3 * HW + p;
      out[p] = q[0]; out[HW + p] = q[HW]; out[2 * HW + p] = q[2 * HW];
    }
  }
}

// ---- MG_OP_ENS_IID: ensemble_iid (marigold/util/ensemble.py:252-270) - the reduction over the members of every element on its own.
// It is depth_median_kernel's `pixel` without the alignment and without the extrema: no min / max table, no scratch, nothing shared
// between lanes - and the same reduce_members / reduce_members_mem on the same padded arrays, so the two ops cannot drift apart.

// E <= E_ <= EMAX members in registers (the bound of depth_median_kernel's register-resident selection).  vec: a lane owns four
// neighbouring elements - one 16-byte load per member, one 16-byte store per output (n % 4 == 0 and all pointers 16-byte aligned:
// the launcher decides); else one element.
template <int E_>
__global__ __launch_bounds__(256) void iid_kernel(const float* __restrict__ d, float* __restrict__ pred, float* __restrict__ unc, int E,
                                                  long long n, int reduction, int vec) {
  if (vec) {
    for (long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; p < n; p += (long long)gridDim.x * 1024) {
      float4 v[E_];
#pragma unroll
      for (int e = 0; e < E_; ++e) v[e] = e < E ? *(const float4*)(d + (long long)e * n + p) : make_float4(0.f, 0.f, 0.f, 0.f);
      float pr[4], un[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float a[E_];
#pragma unroll
        for (int e = 0; e < E_; ++e) a[e] = i == 0 ? v[e].x : (i == 1 ? v[e].y : (i == 2 ? v[e].z : v[e].w));
        reduce_members<E_>(a, E, reduction, unc != nullptr, pr[i], un[i]);
      }
      *(float4*)(pred + p) = make_float4(pr[0], pr[1], pr[2], pr[3]);
      if (unc) *(float4*)(unc + p) = make_float4(un[0], un[1], un[2], un[3]);
    }
  } else {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
      float a[E_];
#pragma unroll
      for (int e = 0; e < E_; ++e) a[e] = e < E ? d[(long long)e * n + p] : 0.f;
      float pr, un;
      reduce_members<E_>(a, E, reduction, unc != nullptr, pr, un);
      pred[p] = pr;
      if (unc) unc[p] = un;
    }
  }
}

// More than EMAX members: one element per lane, the members read from memory wherever the register-resident kernel reads its
// array.  The order statistic as the kernels the depth op runs at these sizes find it: up to EMAX_LDS members by counting ranks
// (depth_median_lds_kernel), beyond by the bitwise selection (depth_median_big_kernel).
__global__ __launch_bounds__(256) void iid_mem_kernel(const float* __restrict__ d, float* __restrict__ pred, float* __restrict__ unc, int E,
                                                      long long n, int reduction) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
    auto member = [&](int e) { return d[(long long)e * n + p]; };
    float pr, un;
    reduce_members_mem(member, E, E <= EMAX_LDS, reduction, unc != nullptr, pr, un);
    pred[p] = pr;
    if (unc) unc[p] = un;
  }
}

// The member bounds the register-resident kernels are instantiated at, for both ops: f(std::integral_constant<int, E_>) with the
// smallest E_ >= E (E <= EMAX).  At E <= 10 the selection is the sorting network.
template <class F>
void with_member_bound(int E, F f) {
  if (E <= 4) f(std::integral_constant<int, 4>());
  else if (E <= 8) f(std::integral_constant<int, 8>());
  else if (E <= 10) f(std::integral_constant<int, 10>());
  else if (E <= 16) f(std::integral_constant<int, 16>());
  else f(std::integral_constant<int, EMAX>());
}

template <int E_>
void launch_iid(const float* d, float* pred, float* unc, int E, long long n, int reduction, hipStream_t s) {
  const int vec = (n & 3) == 0 && (((uintptr_t)d | (uintptr_t)pred | (uintptr_t)unc) & 15) == 0;
  const long long per = vec ? 1024 : 256;
  const int nblk = (int)min((n + per - 1) / per, (long long)2048);
  MG_LAUNCH(iid_kernel<E_>, dim3(nblk), dim3(256), 0, s, d, pred, unc, E, n, reduction, vec);
}

// MG_OP_ENS_DEPTH_MEDIAN decoded once: the argument list its three selection kernels share.  The scratch holds the per-block
// (min, max) table and, behind it, the pixels they were found at.
struct MedianOp {
  const float *d, *st;
  float *med, *mad, *minmax, *blockmm;
  long long* blockpx;
  int E;
  long long HW;
  int reduction, has_shift;
  explicit MedianOp(const mg_op* op)
      : d((const float*)op->p[MG_ENS_DEPTH_MEDIAN_P_D]), st((const float*)op->p[MG_ENS_DEPTH_MEDIAN_P_ST]),
        med((float*)op->p[MG_ENS_DEPTH_MEDIAN_P_MED]), mad((float*)op->p[MG_ENS_DEPTH_MEDIAN_P_MAD]),
        minmax((float*)op->p[MG_ENS_DEPTH_MEDIAN_P_MINMAX]), blockmm((float*)op->p[MG_ENS_DEPTH_MEDIAN_P_SCRATCH]),
        blockpx((long long*)((char*)op->p[MG_ENS_DEPTH_MEDIAN_P_SCRATCH] + 8 * ENS_BLOCKS)), E(op->i[MG_ENS_DEPTH_MEDIAN_I_E]),
        HW(op->l[MG_ENS_DEPTH_MEDIAN_L_HW]), reduction(op->i[MG_ENS_DEPTH_MEDIAN_I_REDUCTION]),
        has_shift(op->i[MG_ENS_DEPTH_MEDIAN_I_HAS_SHIFT]) {}
};
#define MEDIAN_KERNEL_ARGS(m) m.d, m.st, m.med, m.mad, m.blockmm, m.blockpx, m.E, m.HW, m.reduction, m.has_shift, m.st != nullptr

template <int E_>
void launch_median(const MedianOp& m, int nblk, hipStream_t s) {
  MG_LAUNCH(depth_median_kernel<E_>, dim3(nblk), dim3(256), 0, s, MEDIAN_KERNEL_ARGS(m));
}

}  // namespace

int mg_launch_ensemble(const mg_op* op, hipStream_t s) {
  switch (op->kind) {
    case MG_OP_ENS_DEPTH_STATS: {
      const int E = op->i[MG_ENS_DEPTH_STATS_I_E];
      const long long HW = op->l[MG_ENS_DEPTH_STATS_L_HW];
      MG_REQUIRE(E >= 1 && E <= 65535, "ens_depth_stats: E %d out of range [1,65535]", E);
      // (the partial table is nblk x E x (E + 3) doubles: fewer pixel blocks for the ensembles beyond the kernels' usual range)
      const int nblk = (int)min((HW + 255) / 256, (long long)(E > 256 ? 32 : 128));
      MG_LAUNCH(depth_stats_kernel, dim3(nblk, E, (E + EMAX - 1) / EMAX), dim3(256), 0, s, (const float*)op->p[MG_ENS_DEPTH_STATS_P_D],
                         (double*)op->p[MG_ENS_DEPTH_STATS_P_SCRATCH], E, HW);
      MG_LAUNCH(depth_stats_final_kernel, dim3(1), dim3(256), 0, s, (const double*)op->p[MG_ENS_DEPTH_STATS_P_SCRATCH],
                         (double*)op->p[MG_ENS_DEPTH_STATS_P_OUT], E, nblk, HW);
      break;
    }
    case MG_OP_ENS_DEPTH_MEDIAN: {
      const MedianOp m(op);
      const int E = m.E;
      MG_REQUIRE(E >= 1, "ens_depth_median: E %d must be >= 1", E);
      MG_REQUIRE(m.minmax && m.blockmm, "ens_depth_median: minmax / scratch missing");
      const int nblk = (int)min((m.HW + 255) / 256, (long long)ENS_BLOCKS);
      if (E > EMAX_LDS) {
        MG_LAUNCH(depth_median_big_kernel, dim3(nblk), dim3(256), 0, s, MEDIAN_KERNEL_ARGS(m));
      } else if (E > EMAX) {
        const size_t lds = ((size_t)E * 256 + 2 * E) * sizeof(float);
        MG_KERNEL_MAX_LDS((const void*)depth_median_lds_kernel, (int)(((size_t)EMAX_LDS * 256 + 2 * EMAX_LDS) * sizeof(float)));
        MG_LAUNCH(depth_median_lds_kernel, dim3(nblk), dim3(256), lds, s, MEDIAN_KERNEL_ARGS(m));
      } else {
        with_member_bound(E, [&](auto bound) { launch_median<decltype(bound)::value>(m, nblk, s); });
      }
      // (round 3: finishing the reduction in the median kernel's last-arriving block instead - fence + ticket per block - measured
      // SLOWER than this 5 us launch: 40-41 vs 34-36 us per pass, profiles/r3_ab_native_bfgs_alignment.log)
      MG_LAUNCH(minmax_final_kernel, dim3(1), dim3(64), 0, s, (const float*)m.blockmm, (const long long*)m.blockpx, m.d, m.minmax, nblk, E,
                m.HW);
      break;
    }
    case MG_OP_ENS_DEPTH_NORM: {
      const long long HW = op->l[MG_ENS_DEPTH_NORM_L_HW];
      const int nblk = (int)min((HW + 255) / 256, (long long)2048);
      MG_LAUNCH(depth_norm_kernel, dim3(nblk), dim3(256), 0, s, (float*)op->p[MG_ENS_DEPTH_NORM_P_MED], (float*)op->p[MG_ENS_DEPTH_NORM_P_MAD],
                         (const float*)op->p[MG_ENS_DEPTH_NORM_P_MINMAX], HW, op->i[MG_ENS_DEPTH_NORM_I_SHIFT_INVARIANT]);
      break;
    }
    case MG_OP_ENS_NORMALS: {
      const int E = op->i[MG_ENS_NORMALS_I_E];
      const long long HW = op->l[MG_ENS_NORMALS_L_HW];
      MG_REQUIRE(E >= 1, "ens_normals: E must be >= 1");
      const int nblk = (int)min((HW + 255) / 256, (long long)2048);
      MG_LAUNCH(normals_kernel, dim3(nblk), dim3(256), 0, s, (const float*)op->p[MG_ENS_NORMALS_P_NORMALS],
                         (float*)op->p[MG_ENS_NORMALS_P_OUT], (float*)op->p[MG_ENS_NORMALS_P_UNC], E, HW, op->i[MG_ENS_NORMALS_I_REDUCTION]);
      break;
    }
    case MG_OP_ENS_IID: {
      const int E = op->i[MG_ENS_IID_I_E], reduction = op->i[MG_ENS_IID_I_REDUCTION];
      const long long n = op->l[MG_ENS_IID_L_N];
      const float* d = (const float*)op->p[MG_ENS_IID_P_PREDS];
      float *pred = (float*)op->p[MG_ENS_IID_P_PRED], *unc = (float*)op->p[MG_ENS_IID_P_UNC];
      MG_REQUIRE(E >= 1, "ens_iid: E %d must be >= 1", E);
      MG_REQUIRE(n >= 1 && n <= (1ll << 40), "ens_iid: bad element count %lld", n);
      MG_REQUIRE(reduction == 0 || reduction == 1, "ens_iid: Unrecognized reduction method: %d.", reduction);
      MG_REQUIRE(d && pred, "ens_iid: null pointer");
      MG_REQUIRE((((uintptr_t)d | (uintptr_t)pred | (uintptr_t)unc) & 3) == 0, "ens_iid: the members and the outputs must be 4-byte aligned");
      if (E > EMAX) {
        const int nblk = (int)min((n + 255) / 256, (long long)2048);
        MG_LAUNCH(iid_mem_kernel, dim3(nblk), dim3(256), 0, s, d, pred, unc, E, n, reduction);
      } else {
        with_member_bound(E, [&](auto bound) { launch_iid<decltype(bound)::value>(d, pred, unc, E, n, reduction, s); });
      }
      break;
    }
    default: MG_REQUIRE(false, "ensemble: bad op kind %d", op->kind);
  }
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- host arithmetic of the alignment objective (ensemble.py::DepthAligner.cost_and_grad) ----------------------------
// The reference's optimiser (marigold/util/ensemble.py:154-173: scipy BFGS) calls its cost ~100 times per map; the
// pairwise-RMSE part is a closed form of E x E numbers (ensemble.py, module docstring).  As numpy calls that is 30+
// array operations of ~1 us each on 10 x 10 operands; here it is one C call.  Same operations in the same order as the
// numpy form, INCLUDING numpy's pairwise summation (8 accumulators, blocks of 128), so the values - and with them the
// BFGS iterates - are bit-identical (tests/test_host.py pins that); this file is built with -ffp-contract=off.
namespace {
double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
      for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}
// np.add.reduce over a contiguous run of n doubles: numpy hands its inner loop at most `bufsize` (8192) elements at a time and
// adds each piece's pairwise sum to the running result (numpy 2.2; checked against ndarray.sum() for n on both sides of 8192) -
// the pair costs of more than 128 members are more than one piece
double np_sum(const double* a, int n) {
  double res = 0.;
  for (int i = 0; i < n; i += 8192) res += np_pairwise_sum(a + i, n - i < 8192 ? n - i : 8192);
  return res;
}
}  // namespace

extern "C" int mg_ens_align_cost_grad(int E, const double* s, const double* t, const double* mean, const double* C,
                                      double* cost, double* gs, double* gt) {
  MG_REQUIRE(E >= 1 && s && t && mean && C && cost && gs && gt, "ens_align_cost_grad: bad arguments");
  // scratch: 3 E + 3 E^2 doubles, kept per thread (the optimiser calls this ~100 times per map); any ensemble size
  static thread_local std::vector<double> scratch;
  if (scratch.size() < (size_t)3 * E + (size_t)3 * E * E) scratch.resize((size_t)3 * E + (size_t)3 * E * E);
  double* const u = scratch.data();
  double* const s2d = u + E;
  double* const sdc = s2d + E;
  double* const r = sdc + E;
  double* const w = r + (size_t)E * E;
  double* const tmp = w + (size_t)E * E;
  for (int i = 0; i < E; ++i) {
    u[i] = s[i] * mean[i] + t[i];
    s2d[i] = (s[i] * s[i]) * C[i * E + i];
    sdc[i] = s[i] * C[i * E + i];
  }
  for (int i = 0; i < E; ++i)
    for (int j = 0; j < E; ++j) {
      const double du = u[i] - u[j];
      double q = ((s2d[i] + s2d[j]) - ((2.0 * (s[i] * s[j])) * C[i * E + j])) + du * du;
      if (!(q > 0.0)) q = (q != q) ? q : 0.0;   // np.maximum(q, 0.0): NaN propagates
      const double rr = sqrt(q);
      r[i * E + j] = rr;
      w[i * E + j] = (rr > 0 && i != j) ? 0.5 / rr : 0.0;
    }
  int n = 0;
  for (int i = 0; i < E; ++i)
    for (int j = i + 1; j < E; ++j) tmp[n++] = r[i * E + j];
  *cost = np_sum(tmp, n);
  for (int i = 0; i < E; ++i) {
    for (int j = 0; j < E; ++j) {
      const double du = u[i] - u[j];
      tmp[j] = w[i * E + j] * (((2.0 * sdc[i]) - ((2.0 * s[j]) * C[i * E + j])) + ((2.0 * du) * mean[i]));
    }
    gs[i] = np_sum(tmp, E);
    for (int j = 0; j < E; ++j) tmp[j] = (w[i * E + j] * 2.0) * (u[i] - u[j]);
    gt[i] = np_sum(tmp, E);
  }
  return 0;
}
