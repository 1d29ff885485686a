// MG_OP_RANDN: a stateless Gaussian generator - Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC'11; the Random123 constants) + Box-Muller.  The reference draws its initial latents and the LCM step noises with
// torch.randn(generator=...) (marigold/marigold_depth_pipeline.py:430-435, :466-468); a host without torch has no such source, so
// the library brings one whose values are a pure function of (seed, stream, element index):
//   key     = (seed lo, seed hi)
//   counter = (block lo, block hi, stream lo, stream hi),  block = (offset + i) / 4 for element i of the draw,
// and element offset + i takes word (offset + i) % 4 of its block.  Nothing else enters: not the grid, not n, not where a draw was
// split - [offset, offset + n) of a stream is that slice of any larger draw of it, bit for bit.
// Words (0, 1) and (2, 3) of a block are two Box-Muller pairs (a, b): u = ((a >> 9) + 1) 2^-23 in (0, 1] (exact in fp32, never 0),
// v = (b >> 8) 2^-24 in [0, 1) (exact), r = sqrtf(-2 logf(u)), outputs r cospi(2 v), r sinpi(2 v): the angle is never multiplied by
// a rounded pi.  |z| <= sqrt(2 * 23 * ln 2) = 5.647.
// A lane owns one block of four elements: one 16-byte (fp32 / words) or 8-byte (16-bit operands) store where the block lies inside
// the draw and its address is aligned; the blocks at either end of a draw whose offset or end is no multiple of four, and every
// block of an unaligned destination, store element by element.
#include <string.h>

#include "common.h"

namespace {

constexpr int RN_THREADS = 256;
constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0, hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;   // (the bump after the last round is dead code)
    k1 += PHILOX_W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
  const float u = (float)((a >> 9) + 1u) * 0x1p-23f;   // <= 2^23: exact
  const float v2 = (float)(b >> 8) * 0x1p-23f;          // 2 v, exact
  const float r = sqrtf(-2.0f * logf(u));
  float s, c;
  sincospif(v2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// T: float (normals, fp32), bf16_t (normals in the build's 16-bit operand type), unsigned (mode 1: the raw words).
// Lane t of the grid-stride loop owns block first_block + t; dst[e - offset] is element e of the stream.
template <typename T>
__global__ __launch_bounds__(RN_THREADS) void randn_kernel(T* __restrict__ dst, long long n, long long offset, unsigned long long seed,
                                                           unsigned long long stream_id, long long n_blocks, int vec) {
  const long long first = (long long)blockIdx.x * RN_THREADS + threadIdx.x, step = (long long)gridDim.x * RN_THREADS;
  const unsigned long long first_block = (unsigned long long)offset >> 2;
  const long long end = offset + n;
  for (long long t = first; t < n_blocks; t += step) {
    const unsigned long long blk = first_block + (unsigned long long)t;
    unsigned w[4];
    philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), (unsigned)stream_id, (unsigned)(stream_id >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
    T y[4];
    if constexpr (std::is_same_v<T, unsigned>) {
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] = w[k];
    } else {
      float z[4];
      box_muller(w[0], w[1], z[0], z[1]);
      box_muller(w[2], w[3], z[2], z[3]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (std::is_same_v<T, float>) y[k] = z[k];
        else y[k] = f2bf(z[k]);
      }
    }
    const long long e0 = (long long)(blk << 2);   // first element of the block (offset + n <= 2^62: no overflow)
    if (vec && e0 >= offset && e0 + 4 <= end) {
      T* __restrict__ p = dst + (e0 - offset);
      if constexpr (std::is_same_v<T, bf16_t>) *(uint2*)p = make_uint2((unsigned)y[0] | (unsigned)y[1] << 16, (unsigned)y[2] | (unsigned)y[3] << 16);
      else if constexpr (std::is_same_v<T, float>) *(float4*)p = make_float4(y[0], y[1], y[2], y[3]);
      else *(uint4*)p = make_uint4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k >= offset && e0 + k < end) dst[e0 + k - offset] = y[k];
    }
  }
}

template <typename T>
void launch_randn_as(T* dst, long long n, long long offset, unsigned long long seed, unsigned long long stream_id, hipStream_t s) {
  const long long n_blocks = ((offset + n - 1) >> 2) - (offset >> 2) + 1;
  // the address of a whole block, dst + (4 b - offset), is aligned for every b or for none
  const int vec = ((uintptr_t)dst - (uintptr_t)(offset & 3) * sizeof(T)) % (4 * sizeof(T)) == 0;
  const dim3 grid((unsigned)min((n_blocks + RN_THREADS - 1) / RN_THREADS, (long long)2048));
  MG_LAUNCH(randn_kernel<T>, grid, dim3(RN_THREADS), 0, s, dst, n, offset, seed, stream_id, n_blocks, vec);
}

}  // namespace

int mg_launch_randn(const mg_op* op, hipStream_t s) {
  void* dst = op->p[MG_RANDN_P_DST];
  const long long n = op->l[MG_RANDN_L_N], offset = op->l[MG_RANDN_L_OFFSET];
  const unsigned long long seed = (unsigned long long)op->l[MG_RANDN_L_SEED], stream_id = (unsigned long long)op->l[MG_RANDN_L_STREAM];
  const int mode = op->i[MG_RANDN_I_MODE], out16 = op->i[MG_RANDN_I_OUT16] != 0;
  MG_REQUIRE(dst, "randn: null pointer");
  MG_REQUIRE(n > 0 && n <= (1ll << 62) && offset >= 0 && offset <= (1ll << 62) - n, "randn: bad range: %lld elements from offset %lld", n, offset);
  MG_REQUIRE(mode == 0 || mode == 1, "randn: mode must be 0 (normals) or 1 (the raw words)");
  MG_REQUIRE(!(mode == 1 && out16), "randn: the raw words are 32 bits wide (out16 with mode 1)");
  MG_REQUIRE((uintptr_t)dst % (out16 ? 2 : 4) == 0, "randn: the destination must be aligned to its element");
  if (mode == 1) launch_randn_as((unsigned*)dst, n, offset, seed, stream_id, s);
  else if (out16) launch_randn_as((bf16_t*)dst, n, offset, seed, stream_id, s);
  else launch_randn_as((float*)dst, n, offset, seed, stream_id, s);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mg_randn(uint64_t seed, uint64_t stream_id, int64_t offset, int64_t n, void* dst, int out16, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_RANDN;
  op.p[MG_RANDN_P_DST] = dst;
  op.l[MG_RANDN_L_N] = n; op.l[MG_RANDN_L_OFFSET] = offset; op.l[MG_RANDN_L_SEED] = (int64_t)seed; op.l[MG_RANDN_L_STREAM] = (int64_t)stream_id;
  op.i[MG_RANDN_I_MODE] = 0; op.i[MG_RANDN_I_OUT16] = out16 != 0;
  return mg_launch_randn(&op, (hipStream_t)stream);
}
