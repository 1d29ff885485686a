// The order of the fp64 sums of the fit and score kernels (align.hip, tiles.hip, evalscore.hip, lpips.hip), defined once.
// Every kernel of that family makes the same claim - each sum is fp64, its order is fixed, two launches give the same bits - and the
// order is: the thread's own terms as its kernel adds them; the 64 lanes of a wave in the xor butterfly; the waves of a block in wave
// order; the rows of the partial table in row order (one thread per column) or lane-strided (lane l takes rows l, l + 64, ..., then
// the butterfly).  tests/reduction_order.py restates exactly this in numpy and tests/test_gpu_reduction_order.py holds the kernels
// to it bit for bit.  Device code only; no floating-point atomics anywhere.
//
// Include it only from files built with -ffp-contract=off (Makefile: FLAGS_<file>): the terms the kernels feed in are products that
// must round on their own.  The one place with products here, the solve, switches contraction off itself.
#pragma once

#include <hip/hip_runtime.h>

// Sum over the 64 lanes of a wave, the same bits in every lane: six steps v += v[lane ^ m], m = 32, 16, ..., 1 (a + b on both sides
// of a pair).  For double, float and unsigned.  NOT common.h's wave_sum_f: that one adds in DPP order (quads, rows, then the row
// broadcasts) and rounds differently - the two must not be exchanged anywhere.
template <class T>
__device__ __forceinline__ T wave_sum_xor(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// v[k] holds each wave's value (valid in lane 0 at least) -> LDS [waves][N] -> thread k < N adds waves 0, 1, 2, ... in that order
// -> dst[k].  Every thread of the block of THREADS calls it, once per kernel.
template <int N, int THREADS>
__device__ __forceinline__ void waves_sum_store(const double (&v)[N], double* __restrict__ dst) {
  static_assert(THREADS % 64 == 0 && N <= THREADS, "whole waves, a thread per column");
  __shared__ double red[THREADS / 64][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    double s = red[0][k];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) s += red[w][k];
    dst[k] = s;
  }
}

// v[k] summed over the block -> dst[k] (the block's row of a partial table): the butterfly, then the waves in order
template <int N, int THREADS>
__device__ __forceinline__ void block_sum_store(const double (&v)[N], double* __restrict__ dst) {
  double w[N];
#pragma unroll
  for (int k = 0; k < N; ++k) w[k] = wave_sum_xor(v[k]);
  waves_sum_store<N, THREADS>(w, dst);
}

// one column of a partial table: col[0], col[row_stride], ... of rows [0, nblk), added with b ascending
__device__ __forceinline__ double column_sum(const double* __restrict__ col, int nblk, size_t row_stride) {
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += col[(size_t)b * row_stride];
  return s;
}

// rows [0, nblk) of a table in row order -> S[N] in LDS, thread k < N its column k (nblk may differ between the columns); every
// thread of the block calls it and may read S afterwards
template <int N>
__device__ __forceinline__ void rows_sum(const double* __restrict__ part, int nblk, size_t row_stride, size_t col_stride, double (&S)[N]) {
  if (threadIdx.x < N) S[threadIdx.x] = column_sum(part + threadIdx.x * col_stride, nblk, row_stride);
  __syncthreads();
}

// one wave over rows [0, rows) of a table [rows][N]: lane l adds rows l, l + 64, ... in that order (the N columns inside the row
// loop), then the butterfly -> a[N], the same bits in every lane
template <int N>
__device__ __forceinline__ void lane_rows_sum(const double* __restrict__ part, long long rows, double (&a)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = 0.0;
  for (long long c = threadIdx.x; c < rows; c += 64)
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] += part[c * N + k];
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = wave_sum_xor(a[k]);
}

// The scale s and shift t of the least-squares line y = s x + t from (n, Sx, Sy, Sxx, Sxy): the 2 x 2 normal equations, each
// product, difference and quotient rounded on its own.  Unguarded - det may be 0 and the results not finite; what to accept and what
// to fall back to is the caller's rule (align, tiles and the scores differ on purpose).
struct scale_shift {
  double det, s, t;
};
__device__ __forceinline__ scale_shift scale_shift_solve(double n, double Sx, double Sy, double Sxx, double Sxy) {
#pragma clang fp contract(off)
  scale_shift r;
  r.det = n * Sxx - Sx * Sx;
  r.s = (n * Sxy - Sx * Sy) / r.det;
  r.t = (Sy - r.s * Sx) / n;
  return r;
}
