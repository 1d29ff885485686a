// Image resampling on the device: the resize steps either side of the hot path
// (reference: marigold/util/image_util.py:90-120 `resize_max_res`, marigold_depth_pipeline.py:306-312
// resize-back, marigold/util/ensemble.py:158-161 nearest-exact down-size).  The reference calls
// torchvision.transforms.functional.resize(..., antialias=True), i.e. torch's separable anti-aliased
// bilinear / bicubic interpolation (align_corners = False) - restated here tap for tap:
//   scale = in / out; support = (interp/2) * max(scale, 1); for output i: center = scale * (i + 0.5),
//   xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), in) - xmin,
//   w_j = filter((j + xmin - center + 0.5) / max(scale, 1)) normalised to sum 1 (fp32 throughout),
// horizontal pass first (into an fp32 temporary), then vertical; uint8 inputs are computed in float,
// rounded half-to-even (clamped to [0, 255] for bicubic) and cast back.  nearest-exact:
// src = floor((i + 0.5) * scale).
#include <string.h>

#include "common.h"

namespace {

__device__ __forceinline__ float aa_filter(float x, int bicubic) {
  x = fabsf(x);
  if (!bicubic) return x < 1.0f ? 1.0f - x : 0.0f;
  const float a = -0.5f;
  if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
  return 0.0f;
}

// The byte a resampled uint8 image holds, as a float: round half to even like torch.round(), bicubic clamped to [0, 255] first.
__device__ __forceinline__ float u8_round(float v, int bicubic) {
  if (bicubic) v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (float)(uint8_t)rintf(v);
}

// torch's `x / 255.0 * 2.0 - 1.0` on a byte value, in fp32 with torch's roundings (the file is built without FMA contraction, and the
// intrinsics keep the compiler from re-associating): the host kernel divides (IEEE), the device kernel of a tensor divided by a
// scalar multiplies by fp32(1 / 255) - 111 of the 256 byte values end up one ulp apart, so the caller says which chain it replaces.
__device__ __forceinline__ float rgb_norm(float x, int reciprocal) {
  const float q = reciprocal ? __fmul_rn(x, 1.0f / 255.0f) : __fdiv_rn(x, 255.0f);
  return __fsub_rn(__fmul_rn(q, 2.0f), 1.0f);
}

// Where a pass reads and writes; `i` is always the index into [planes][rows][cols].
template <typename T>
struct plane_src {   // planes as MG_OP_RESIZE has them
  const T* __restrict__ p;
  __device__ __forceinline__ float ld(long long i) const { return (float)p[i]; }
};
struct hwc_src {     // the same three planes read from 3-byte pixels (PIL's layout); hw = rows * cols of the source
  const uint8_t* __restrict__ p;
  long long hw;
  __device__ __forceinline__ float ld(long long i) const {
    const int c = (i >= hw) + (i >= 2 * hw);
    return (float)p[(i - c * hw) * 3 + c];
  }
};
template <typename T>
struct plane_dst {
  T* __restrict__ p;
  __device__ __forceinline__ void st(long long i, float v, int bicubic) const {
    if constexpr (std::is_same_v<T, uint8_t>) p[i] = (uint8_t)u8_round(v, bicubic);
    else p[i] = v;
  }
};
template <typename T>
struct norm_dst {    // MG_OP_RGB_PREP's last pass: the uint8 result normalised in the store; T = float | bf16_t (the operand type)
  T* __restrict__ p;
  int reciprocal;
  __device__ __forceinline__ void st(long long i, float v, int bicubic) const {
    const float y = rgb_norm(u8_round(v, bicubic), reciprocal);
    if constexpr (std::is_same_v<T, float>) p[i] = y;
    else p[i] = f2bf(y);
  }
};

// One output element per thread.  The resampled axis has `in_len` -> `out_len` elements with element
// stride `s_axis`; the other in-plane axis has `other` elements with stride `s_other`; planes are
// contiguous (`plane_in` / `plane_out` elements).  Output is [planes][out rows][out cols] row-major.
template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void resize_aa_pass_kernel(const SRC src, const DST dst,
                                                             long long total, int in_len, int out_len, int other,
                                                             int horizontal, int bicubic, float scale) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  // output layout: horizontal pass -> [plane][other = rows][out_len = cols]; vertical -> [plane][out_len][other]
  int i, o;
  long long plane;
  if (horizontal) { i = (int)(idx % out_len); o = (int)((idx / out_len) % other); plane = idx / ((long long)out_len * other); }
  else { o = (int)(idx % other); i = (int)((idx / other) % out_len); plane = idx / ((long long)out_len * other); }
  const float support = (bicubic ? 2.0f : 1.0f) * (scale >= 1.0f ? scale : 1.0f);
  const float invscale = scale >= 1.0f ? (float)(1.0 / (double)scale) : 1.0f;
  const float center = scale * ((float)i + 0.5f);
  // torch evaluates `center - support` in fp32 and adds the 0.5 (and scales the filter argument) in fp64
  int xmin = (int)((double)(center - support) + 0.5);
  xmin = xmin > 0 ? xmin : 0;
  int xend = (int)((double)(center + support) + 0.5);
  xend = xend < in_len ? xend : in_len;
  const int xsize = xend - xmin;
  float total_w = 0.0f;
  auto weight = [&](int j) {
    return aa_filter((float)(((double)((float)(j + xmin) - center) + 0.5) * (double)invscale), bicubic);
  };
  for (int j = 0; j < xsize; ++j) total_w += weight(j);
  const long long base = plane * (long long)in_len * other;
  float t = 0.0f;
  for (int j = 0; j < xsize; ++j) {
    float w = weight(j);
    w = total_w != 0.0f ? w / total_w : 0.0f;
    const long long sidx = horizontal ? base + (long long)o * in_len + (j + xmin)
                                      : base + (long long)(j + xmin) * other + o;
    const float v = src.ld(sidx) * w;
    t = j == 0 ? v : t + v;
  }
  dst.st(idx, t, bicubic);
}

template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void resize_nearest_exact_kernel(const SRC src, const DST dst,
                                                                   long long total, int Hin, int Win, int Hout,
                                                                   int Wout, float sy, float sx) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % Wout), y = (int)((idx / Wout) % Hout);
  const long long plane = idx / ((long long)Wout * Hout);
  int iy = (int)floorf(((float)y + 0.5f) * sy), ix = (int)floorf(((float)x + 0.5f) * sx);
  iy = iy < Hin - 1 ? iy : Hin - 1;
  ix = ix < Win - 1 ? ix : Win - 1;
  dst.st(idx, src.ld((plane * Hin + iy) * Win + ix), 0);   // (a byte or an fp32 value passes through ld / st unchanged)
}

template <typename SRC, typename DST>
void launch_pass(const SRC src, const DST dst, long long total, int in_len, int out_len, int other, int horizontal,
                 int bicubic, hipStream_t s) {
  const float scale = (float)in_len / (float)out_len;
  MG_LAUNCH((resize_aa_pass_kernel<SRC, DST>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, total, in_len,
            out_len, other, horizontal, bicubic, scale);
}

// The resample of `planes` [Hin][Win] planes to [Hout][Wout] (sizes differ): nearest-exact in one launch, bilinear / bicubic
// horizontal first (rows = Hin, into the fp32 temporary), then vertical on the result - torch's order; one pass when one axis changes.
template <typename SRC, typename DST>
void launch_resample(const SRC src, const DST dst, float* tmp, long long planes, int Hin, int Win, int Hout, int Wout, int mode,
                     hipStream_t s) {
  if (mode == 2) {
    const long long total = planes * Hout * Wout;
    const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
    MG_LAUNCH((resize_nearest_exact_kernel<SRC, DST>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, total, Hin, Win,
              Hout, Wout, sy, sx);
    return;
  }
  const int bicubic = mode == 1;
  if (Win != Wout && Hin != Hout) {
    launch_pass(src, plane_dst<float>{tmp}, planes * Hin * Wout, Win, Wout, Hin, 1, bicubic, s);
    launch_pass(plane_src<float>{tmp}, dst, planes * Hout * Wout, Hin, Hout, Wout, 0, bicubic, s);
  } else if (Win != Wout) {
    launch_pass(src, dst, planes * Hin * Wout, Win, Wout, Hin, 1, bicubic, s);
  } else {
    launch_pass(src, dst, planes * Hout * Wout, Hin, Hout, Wout, 0, bicubic, s);
  }
}

}  // namespace

// Colour-mapped depth (marigold/util/image_util.py:38-76 colorize_depth_maps + the pipeline's (x * 255).astype(uint8),
// marigold_depth_pipeline.py:318-327): matplotlib's listed / segmented colormaps are 256-entry tables indexed by
// int(x * 256) (x == 1 -> 255); the table arrives as uint8 RGB (built once per colormap on the host from matplotlib
// itself), the output is the HWC uint8 image PIL takes.
// The same launch is the depth pipeline's whole output stage (:314-316 and script/depth/run.py's 16-bit PNG): `clipped` = np.clip(d, 0, 1)
// and `u16` = (np.clip(d, 0, 1) * 65535).astype(uint16), both of the depth itself (their range is (0, 1): lo = 0, inv_range = 1).  The
// clip is written with comparisons so that NaN falls through both (and -0.0 stays, as in numpy's contiguous loop); the 16-bit value
// is one fp32 product truncated, NaN -> 0.  Every output is optional; `clipped` may be `depth` (a lane reads its elements before
// it writes them, and no other lane touches them).
struct u32x3 { unsigned x, y, z; };   // 12 bytes, 4-byte aligned: four HWC pixels

__device__ __forceinline__ float clip_cmp(float x, float lo, float hi) {
  x = x < lo ? lo : x;
  x = x > hi ? hi : x;
  return x;
}

__device__ __forceinline__ unsigned depth_u16(float c) {   // c = the clipped depth, in [0, 1] or NaN
  const float y = __fmul_rn(c, 65535.0f);
  return y == y ? (unsigned)(int)y : 0u;
}

// The table entry of a depth: 3 k, or -1 for matplotlib's "bad" colour, RGBA (0, 0, 0, 0): a NaN depth is a black pixel, not entry 0
__device__ __forceinline__ int depth_entry(float d, float lo, float inv_range) {
  float x = (d - lo) * inv_range;
  if (x != x) return -1;
  x = clip_cmp(x, 0.f, 1.f);
  int k = (int)(x * 256.0f);
  k = k > 255 ? 255 : k;
  return 3 * k;
}

// vec: a lane owns four neighbouring elements - one 16-byte load, a 16-byte store of the clipped values, an 8-byte store of the 16-bit
// values, a 12-byte store of the colours (n % 4 == 0 and every pointer given aligned for its access); otherwise one element per lane.
__global__ __launch_bounds__(256) void colorize_kernel(const float* depth, const uint8_t* __restrict__ lut, uint8_t* __restrict__ out,
                                                       float* clipped, uint16_t* __restrict__ u16, long long n, float lo,
                                                       float inv_range, int vec) {
  __shared__ uint8_t tab[768];
  if (out) {   // (uniform over the grid)
    for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
    __syncthreads();
  }
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  if (vec) {
    for (long long q = first; q < n / 4; q += step) {
      const float4 d = ((const float4*)depth)[q];
      const float v[4] = {d.x, d.y, d.z, d.w};
      if (clipped || u16) {
        float c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = clip_cmp(v[j], 0.f, 1.f);
        if (clipped) ((float4*)clipped)[q] = make_float4(c[0], c[1], c[2], c[3]);
        if (u16) ((uint2*)u16)[q] = make_uint2(depth_u16(c[0]) | depth_u16(c[1]) << 16, depth_u16(c[2]) | depth_u16(c[3]) << 16);
      }
      if (out) {
        unsigned b[12];   // byte 3 j + c: channel c of pixel 4 q + j
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = depth_entry(v[j], lo, inv_range);
#pragma unroll
          for (int c = 0; c < 3; ++c) b[3 * j + c] = e < 0 ? 0u : (unsigned)tab[e + c];
        }
        u32x3 w;
        w.x = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
        w.y = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
        w.z = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
        ((u32x3*)out)[q] = w;
      }
    }
  } else {
    for (long long i = first; i < n; i += step) {
      const float d = depth[i];
      if (clipped || u16) {
        const float c = clip_cmp(d, 0.f, 1.f);
        if (clipped) clipped[i] = c;
        if (u16) u16[i] = (uint16_t)depth_u16(c);
      }
      if (out) {
        const int e = depth_entry(d, lo, inv_range);
        out[3 * i + 0] = e < 0 ? (uint8_t)0 : tab[e + 0];
        out[3 * i + 1] = e < 0 ? (uint8_t)0 : tab[e + 1];
        out[3 * i + 2] = e < 0 ? (uint8_t)0 : tab[e + 2];
      }
    }
  }
}

static int launch_colorize(const mg_op* op, hipStream_t s) {
  const long long n = op->l[MG_COLORIZE_L_N];
  const float* depth = (const float*)op->p[MG_COLORIZE_P_DEPTH];
  const uint8_t* lut = (const uint8_t*)op->p[MG_COLORIZE_P_LUT];
  uint8_t* out = (uint8_t*)op->p[MG_COLORIZE_P_OUT];
  float* clipped = (float*)op->p[MG_COLORIZE_P_CLIPPED];
  uint16_t* u16 = (uint16_t*)op->p[MG_COLORIZE_P_U16];
  const float lo = op->f[MG_COLORIZE_F_MIN_DEPTH], hi = op->f[MG_COLORIZE_F_MAX_DEPTH];
  MG_REQUIRE(n > 0 && depth && (out || clipped || u16) && (lut || !out), "colorize: null pointer / empty map");
  MG_REQUIRE(hi > lo, "colorize: max_depth must exceed min_depth");
  MG_REQUIRE(!(clipped || u16) || (lo == 0.0f && hi == 1.0f),
             "colorize: the clipped and the 16-bit output are defined for the range (0, 1) only (got %g, %g)", (double)lo, (double)hi);
  MG_REQUIRE((uintptr_t)depth % 4 == 0 && (uintptr_t)clipped % 4 == 0 && (uintptr_t)u16 % 2 == 0,
             "colorize: a pointer is not aligned to its element");
  const int vec = n % 4 == 0 && (uintptr_t)depth % 16 == 0 && (uintptr_t)clipped % 16 == 0 && (uintptr_t)u16 % 8 == 0 && (uintptr_t)out % 4 == 0;
  const long long work = vec ? n / 4 : n;
  MG_LAUNCH(colorize_kernel, dim3((unsigned)min((work + 255) / 256, (long long)4096)), dim3(256), 0, s, depth, lut, out, clipped, u16, n, lo,
            1.0f / (hi - lo), vec);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

// The output stage of the intrinsic-image pipeline (marigold/marigold_iid_pipeline.py:117-136, MarigoldIIDOutput.fill_entry): per
// target [3][H][W] in fp32 -> the HWC uint8 image PIL takes,
//   up to scale:  x <- x / max(max over the target, 1e-6)   (IEEE fp32 division: numpy divides the array by a float32 scalar)
//   linear:       x <- powf(x, fp32(1 / 2.2))
//   all:          (x * 255).astype(uint8): truncation to int32, low 8 bits kept; NaN and |x * 255| >= 2^31 give 0 (x86-64 cvttss2si
//                 returns 0x80000000 for them).
// The maximum keeps NaN like numpy's (IEEE maximum), so it does not depend on the order: thread -> wave -> block -> one slot of
// the target's row of a partial table, which every block of the map kernel reduces again.  Two launches for all targets of an image.
constexpr int IV_THREADS = 256;

__device__ __forceinline__ float iv_block_max(float v, float* __restrict__ red) {   // every thread of the block calls it
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max_keep_nan(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max_keep_nan(max_keep_nan(red[0], red[1]), max_keep_nan(red[2], red[3]));
}

// grid (parts, n): block (b, t) -> part[t][b] = max over its share of target t's n3 = 3 H W elements; targets outside `need` are skipped
__global__ __launch_bounds__(IV_THREADS) void iid_vis_max_kernel(const float* __restrict__ src, float* __restrict__ part,
                                                                 long long n3, unsigned need, int vec) {
  __shared__ float red[IV_THREADS / 64];
  const int t = blockIdx.y;
  if (!((need >> t) & 1u)) return;
  const float* __restrict__ x = src + (long long)t * n3;
  const long long first = (long long)blockIdx.x * IV_THREADS + threadIdx.x, step = (long long)gridDim.x * IV_THREADS;
  float m = -INFINITY;
  if (vec) {   // n3 % 4 == 0 and a 16-byte aligned base: every target starts on a 16-byte boundary
    const float4* __restrict__ x4 = (const float4*)x;
    for (long long i = first; i < n3 / 4; i += step) {
      const float4 v = x4[i];
      m = max_keep_nan(max_keep_nan(max_keep_nan(m, v.x), max_keep_nan(v.y, v.z)), v.w);
    }
  } else {
    for (long long i = first; i < n3; i += step) m = max_keep_nan(m, x[i]);
  }
  m = iv_block_max(m, red);
  if (threadIdx.x == 0) part[t * MG_IID_VIS_PARTS + blockIdx.x] = m;
}

__device__ __forceinline__ unsigned iv_byte(float x, float m, bool scale, bool linear) {
  if (scale) x = x / m;
  if (linear) x = powf(x, (float)(1.0 / 2.2));
  x = x * 255.0f;
  const int k = fabsf(x) < 2147483648.0f ? (int)x : 0;   // (int) truncates toward zero; NaN fails the comparison
  return (unsigned)k & 0xffu;
}

// grid (blocks, n).  vec: a lane owns four neighbouring pixels - three 16-byte loads, one per plane, and 12 contiguous output
// bytes (a wave writes 768 contiguous bytes); otherwise one pixel per lane.
__global__ __launch_bounds__(IV_THREADS) void iid_vis_map_kernel(const float* __restrict__ src, const float* __restrict__ part,
                                                                 uint8_t* __restrict__ out, long long HW, int parts,
                                                                 unsigned linear_mask, unsigned scale_mask, int vec) {
  __shared__ float red[IV_THREADS / 64];
  const int t = blockIdx.y;
  const bool linear = (linear_mask >> t) & 1u, scale = linear && ((scale_mask >> t) & 1u);
  float m = 1.0f;
  if (scale) {   // (uniform over the block)
    m = iv_block_max((int)threadIdx.x < parts ? part[t * MG_IID_VIS_PARTS + threadIdx.x] : -INFINITY, red);
    m = 1e-6f > m ? 1e-6f : m;   // Python's max(m, 1e-6): a NaN maximum stays
  }
  const float* __restrict__ x = src + (long long)t * 3 * HW;
  uint8_t* __restrict__ o = out + (long long)t * 3 * HW;
  const long long first = (long long)blockIdx.x * IV_THREADS + threadIdx.x, step = (long long)gridDim.x * IV_THREADS;
  if (vec) {   // HW % 4 == 0, src 16-byte and out 4-byte aligned
    const float4 *__restrict__ r4 = (const float4*)x, *__restrict__ g4 = (const float4*)(x + HW), *__restrict__ b4 = (const float4*)(x + 2 * HW);
    unsigned* __restrict__ o4 = (unsigned*)o;
    for (long long q = first; q < HW / 4; q += step) {
      const float4 r = r4[q], g = g4[q], b = b4[q];
      const unsigned w0 = iv_byte(r.x, m, scale, linear) | iv_byte(g.x, m, scale, linear) << 8 | iv_byte(b.x, m, scale, linear) << 16 |
                          iv_byte(r.y, m, scale, linear) << 24;
      const unsigned w1 = iv_byte(g.y, m, scale, linear) | iv_byte(b.y, m, scale, linear) << 8 | iv_byte(r.z, m, scale, linear) << 16 |
                          iv_byte(g.z, m, scale, linear) << 24;
      const unsigned w2 = iv_byte(b.z, m, scale, linear) | iv_byte(r.w, m, scale, linear) << 8 | iv_byte(g.w, m, scale, linear) << 16 |
                          iv_byte(b.w, m, scale, linear) << 24;
      o4[3 * q + 0] = w0;
      o4[3 * q + 1] = w1;
      o4[3 * q + 2] = w2;
    }
  } else {
    for (long long i = first; i < HW; i += step) {
      o[3 * i + 0] = (uint8_t)iv_byte(x[i], m, scale, linear);
      o[3 * i + 1] = (uint8_t)iv_byte(x[HW + i], m, scale, linear);
      o[3 * i + 2] = (uint8_t)iv_byte(x[2 * HW + i], m, scale, linear);
    }
  }
}

static int launch_iid_vis(const mg_op* op, hipStream_t s) {
  const int n = op->i[MG_IID_VIS_I_N], H = op->i[MG_IID_VIS_I_H], W = op->i[MG_IID_VIS_I_W];
  const unsigned linear = (unsigned)op->i[MG_IID_VIS_I_LINEAR_BITS], up_to_scale = (unsigned)op->i[MG_IID_VIS_I_UP_TO_SCALE_BITS];
  const float* pred = (const float*)op->p[MG_IID_VIS_P_PRED];
  uint8_t* out = (uint8_t*)op->p[MG_IID_VIS_P_OUT];
  float* ws = (float*)op->p[MG_IID_VIS_P_WS];
  MG_REQUIRE(n >= 1 && n <= 16, "iid_vis: 1 to 16 targets per launch (got %d)", n);
  MG_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1ll << 30), "iid_vis: bad size %d x %d", H, W);
  MG_REQUIRE(!((linear | up_to_scale) >> n), "iid_vis: a flag names a target beyond the %d given", n);
  MG_REQUIRE(pred && out, "iid_vis: null pointer");
  MG_REQUIRE((uintptr_t)pred % 4 == 0, "iid_vis: the prediction must be 4-byte aligned");
  const unsigned need = linear & up_to_scale;   // the maximum is used by the linear, up-to-scale targets only
  MG_REQUIRE(!need || (ws && (uintptr_t)ws % 4 == 0), "iid_vis: null or unaligned workspace (f32 [n][MG_IID_VIS_PARTS])");
  const long long HW = (long long)H * W;
  const int vec = HW % 4 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)out % 4 == 0;
  // a thread of the maximum takes at least 16 elements; the partial rows have MG_IID_VIS_PARTS slots
  const int parts = (int)min((3 * HW + 16 * IV_THREADS - 1) / (16 * IV_THREADS), (long long)MG_IID_VIS_PARTS);
  if (need) MG_LAUNCH(iid_vis_max_kernel, dim3(parts, n), dim3(IV_THREADS), 0, s, pred, ws, 3 * HW, need, vec);
  const long long work = vec ? HW / 4 : HW;
  MG_LAUNCH(iid_vis_map_kernel, dim3((unsigned)min((work + IV_THREADS - 1) / IV_THREADS, (long long)1024), n), dim3(IV_THREADS), 0, s,
            pred, (const float*)ws, out, HW, parts, linear, up_to_scale, vec);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

// The input stage of every pipeline (marigold/marigold_depth_pipeline.py:229-255: pil_to_tensor, resize_max_res, `rgb / 255.0 * 2.0 -
// 1.0`, the cast to the pipeline's dtype) on the uint8 picture as PIL holds it (HWC) or as a [3][H][W] tensor.  Same size: the
// kernel below; sizes differ: the resampling passes above with the normalisation in the last pass's store (launch_rgb_prep).
template <typename T>
__device__ __forceinline__ void rgb_prep_store4(T* __restrict__ p, long long q, float a, float b, float c, float d) {
  if constexpr (std::is_same_v<T, float>) ((float4*)p)[q] = make_float4(a, b, c, d);
  else ((uint2*)p)[q] = make_uint2(pack2bf(a, b), pack2bf(c, d));
}

// vec: a lane owns four neighbouring pixels - HWC: one 12-byte load, CHW: one 4-byte load per plane - and writes one vector per
// plane (16 bytes of fp32, 8 bytes of the operand type); otherwise one pixel per lane.
template <typename T>
__global__ __launch_bounds__(IV_THREADS) void rgb_prep_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, long long HW, int hwc,
                                                              int reciprocal, int vec) {
  const long long first = (long long)blockIdx.x * IV_THREADS + threadIdx.x, step = (long long)gridDim.x * IV_THREADS;
  if (vec) {   // W % 4 == 0 (so HW % 4 == 0: every plane starts on a vector boundary), src 4-byte and dst vector aligned
    for (long long q = first; q < HW / 4; q += step) {
      unsigned r, g, b;   // byte k of each: channel value of pixel 4 q + k
      if (hwc) {
        const u32x3 w = ((const u32x3*)src)[q];   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        r = (w.x & 0xffu) | (w.x >> 24) << 8 | ((w.y >> 16) & 0xffu) << 16 | ((w.z >> 8) & 0xffu) << 24;
        g = ((w.x >> 8) & 0xffu) | (w.y & 0xffu) << 8 | (w.y >> 24) << 16 | ((w.z >> 16) & 0xffu) << 24;
        b = ((w.x >> 16) & 0xffu) | ((w.y >> 8) & 0xffu) << 8 | (w.z & 0xffu) << 16 | (w.z >> 24) << 24;
      } else {
        const unsigned* __restrict__ s4 = (const unsigned*)src;
        r = s4[q]; g = s4[HW / 4 + q]; b = s4[HW / 2 + q];
      }
      const unsigned ch[3] = {r, g, b};
#pragma unroll
      for (int c = 0; c < 3; ++c)
        rgb_prep_store4(dst + c * HW, q, rgb_norm((float)(ch[c] & 0xffu), reciprocal), rgb_norm((float)((ch[c] >> 8) & 0xffu), reciprocal),
                        rgb_norm((float)((ch[c] >> 16) & 0xffu), reciprocal), rgb_norm((float)(ch[c] >> 24), reciprocal));
    }
  } else {
    for (long long i = first; i < HW; i += step) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float y = rgb_norm((float)(hwc ? src[3 * i + c] : src[c * HW + i]), reciprocal);
        if constexpr (std::is_same_v<T, float>) dst[c * HW + i] = y;
        else dst[c * HW + i] = f2bf(y);
      }
    }
  }
}

static int launch_rgb_prep(const mg_op* op, hipStream_t s) {
  const int Hin = op->i[MG_RGB_PREP_I_HIN], Win = op->i[MG_RGB_PREP_I_WIN], Hout = op->i[MG_RGB_PREP_I_HOUT], Wout = op->i[MG_RGB_PREP_I_WOUT];
  const int mode = op->i[MG_RGB_PREP_I_MODE], hwc = op->i[MG_RGB_PREP_I_HWC] != 0, out16 = op->i[MG_RGB_PREP_I_OUT16] != 0;
  const int reciprocal = op->i[MG_RGB_PREP_I_RECIPROCAL] != 0;
  const uint8_t* src = (const uint8_t*)op->p[MG_RGB_PREP_P_SRC];
  void* dst = op->p[MG_RGB_PREP_P_DST];
  float* tmp = (float*)op->p[MG_RGB_PREP_P_TMP];
  MG_REQUIRE(Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && (long long)Hin * Win <= (1ll << 30) && (long long)Hout * Wout <= (1ll << 30),
             "rgb_prep: bad size %d x %d -> %d x %d", Hin, Win, Hout, Wout);
  MG_REQUIRE(mode >= 0 && mode <= 2, "rgb_prep: mode must be 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)");
  MG_REQUIRE(src && dst, "rgb_prep: null pointer");
  MG_REQUIRE((uintptr_t)dst % (out16 ? 2 : 4) == 0, "rgb_prep: the destination must be aligned to its element");
  if (Hin == Hout && Win == Wout) {
    const long long HW = (long long)Hin * Win;
    const int vec = Win % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % (out16 ? 8 : 16) == 0;
    const long long work = vec ? HW / 4 : HW;
    const dim3 grid((unsigned)min((work + IV_THREADS - 1) / IV_THREADS, (long long)2048));
    if (out16) MG_LAUNCH(rgb_prep_kernel<bf16_t>, grid, dim3(IV_THREADS), 0, s, src, (bf16_t*)dst, HW, hwc, reciprocal, vec);
    else MG_LAUNCH(rgb_prep_kernel<float>, grid, dim3(IV_THREADS), 0, s, src, (float*)dst, HW, hwc, reciprocal, vec);
  } else {
    MG_REQUIRE(mode == 2 || Hin == Hout || Win == Wout || (tmp && (uintptr_t)tmp % 4 == 0),
               "rgb_prep: fp32 temporary [3][Hin][Wout] missing or unaligned");
    const hwc_src sh{src, (long long)Hin * Win};
    const plane_src<uint8_t> sp{src};
    const norm_dst<bf16_t> d16{(bf16_t*)dst, reciprocal};
    const norm_dst<float> d32{(float*)dst, reciprocal};
    if (hwc && out16) launch_resample(sh, d16, tmp, 3, Hin, Win, Hout, Wout, mode, s);
    else if (hwc) launch_resample(sh, d32, tmp, 3, Hin, Win, Hout, Wout, mode, s);
    else if (out16) launch_resample(sp, d16, tmp, 3, Hin, Win, Hout, Wout, mode, s);
    else launch_resample(sp, d32, tmp, 3, Hin, Win, Hout, Wout, mode, s);
  }
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

// The normals picture (marigold/marigold_normals_pipeline.py:297-301): clip(-1, 1) as numpy.clip does (NaN stays), (x + 1) * 127.5 in
// fp32 with two roundings, astype(uint8) = truncation to int32 and its low 8 bits; NaN gives 0 (MG_OP_IID_VIS's convention for
// x86-64).  After the clip the product lies in [0, 255], so nothing else is out of range.  The clipped values themselves are what
// the pipeline keeps as normals_np (:294): `c`, when given, receives them (it may be `x`: a lane reads its pixels before it
// writes them); either output may be NULL.
__device__ __forceinline__ unsigned nv_byte(float c) {   // c = the clipped value
  const float y = __fmul_rn(__fadd_rn(c, 1.0f), 127.5f);
  return (unsigned)(y == y ? (int)y : 0) & 0xffu;
}

__device__ __forceinline__ float4 nv_clip4(float4 v) {
  return make_float4(clip_keep_nan(v.x, -1.0f, 1.0f), clip_keep_nan(v.y, -1.0f, 1.0f), clip_keep_nan(v.z, -1.0f, 1.0f), clip_keep_nan(v.w, -1.0f, 1.0f));
}

// vec: a lane owns four neighbouring pixels - three 16-byte loads, one per plane, three 16-byte stores of the clipped values and 12
// contiguous output bytes; otherwise one pixel.
__global__ __launch_bounds__(IV_THREADS) void normals_vis_kernel(const float* x, float* c, uint8_t* __restrict__ o, long long HW, int vec) {
  const long long first = (long long)blockIdx.x * IV_THREADS + threadIdx.x, step = (long long)gridDim.x * IV_THREADS;
  if (vec) {   // HW % 4 == 0, x and c 16-byte and o 4-byte aligned
    const float4 *r4 = (const float4*)x, *g4 = (const float4*)(x + HW), *b4 = (const float4*)(x + 2 * HW);
    u32x3* __restrict__ o12 = (u32x3*)o;
    for (long long q = first; q < HW / 4; q += step) {
      const float4 r = nv_clip4(r4[q]), g = nv_clip4(g4[q]), b = nv_clip4(b4[q]);
      if (c) {
        ((float4*)c)[q] = r;
        ((float4*)(c + HW))[q] = g;
        ((float4*)(c + 2 * HW))[q] = b;
      }
      if (o) {
        u32x3 w;
        w.x = nv_byte(r.x) | nv_byte(g.x) << 8 | nv_byte(b.x) << 16 | nv_byte(r.y) << 24;
        w.y = nv_byte(g.y) | nv_byte(b.y) << 8 | nv_byte(r.z) << 16 | nv_byte(g.z) << 24;
        w.z = nv_byte(b.z) | nv_byte(r.w) << 8 | nv_byte(g.w) << 16 | nv_byte(b.w) << 24;
        o12[q] = w;
      }
    }
  } else {
    for (long long i = first; i < HW; i += step) {
      const float r = clip_keep_nan(x[i], -1.0f, 1.0f), g = clip_keep_nan(x[HW + i], -1.0f, 1.0f), b = clip_keep_nan(x[2 * HW + i], -1.0f, 1.0f);
      if (c) {
        c[i] = r;
        c[HW + i] = g;
        c[2 * HW + i] = b;
      }
      if (o) {
        o[3 * i + 0] = (uint8_t)nv_byte(r);
        o[3 * i + 1] = (uint8_t)nv_byte(g);
        o[3 * i + 2] = (uint8_t)nv_byte(b);
      }
    }
  }
}

static int launch_normals(const float* pred, int H, int W, float* clipped, uint8_t* out, hipStream_t s) {
  MG_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1ll << 30), "normals_vis: bad size %d x %d", H, W);
  MG_REQUIRE(pred && (out || clipped), "normals_vis: null pointer");
  MG_REQUIRE((uintptr_t)pred % 4 == 0 && (uintptr_t)clipped % 4 == 0, "normals_vis: the prediction must be 4-byte aligned");
  const long long HW = (long long)H * W;
  const int vec = HW % 4 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)clipped % 16 == 0 && (uintptr_t)out % 4 == 0;
  const long long work = vec ? HW / 4 : HW;
  MG_LAUNCH(normals_vis_kernel, dim3((unsigned)min((work + IV_THREADS - 1) / IV_THREADS, (long long)2048)), dim3(IV_THREADS), 0, s, pred,
            clipped, out, HW, vec);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

static int launch_normals_vis(const mg_op* op, hipStream_t s) {
  uint8_t* out = (uint8_t*)op->p[MG_NORMALS_VIS_P_OUT];
  MG_REQUIRE(out, "normals_vis: null pointer");
  return launch_normals((const float*)op->p[MG_NORMALS_VIS_P_PRED], op->i[MG_NORMALS_VIS_I_H], op->i[MG_NORMALS_VIS_I_W], nullptr, out, s);
}

int mg_launch_resize(const mg_op* op, hipStream_t s) {
  if (op->kind == MG_OP_IID_VIS) return launch_iid_vis(op, s);
  if (op->kind == MG_OP_RGB_PREP) return launch_rgb_prep(op, s);
  if (op->kind == MG_OP_NORMALS_VIS) return launch_normals_vis(op, s);
  if (op->kind == MG_OP_COLORIZE) return launch_colorize(op, s);
  const long long planes = op->i[MG_RESIZE_I_PLANES];
  const int Hin = op->i[MG_RESIZE_I_HIN], Win = op->i[MG_RESIZE_I_WIN], Hout = op->i[MG_RESIZE_I_HOUT], Wout = op->i[MG_RESIZE_I_WOUT];
  const int mode = op->i[MG_RESIZE_I_MODE];
  const int u8 = op->i[MG_RESIZE_I_U8];  // 1: uint8 in and out, 0: fp32
  void *src = op->p[MG_RESIZE_P_SRC], *dst = op->p[MG_RESIZE_P_DST];
  float* tmp = (float*)op->p[MG_RESIZE_P_TMP];
  MG_REQUIRE(planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "resize: empty image");
  MG_REQUIRE(mode >= 0 && mode <= 2, "resize: mode must be 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)");
  MG_REQUIRE(src && dst, "resize: null pointer");
  MG_REQUIRE(mode == 2 || Win != Wout || Hin != Hout, "resize: sizes are equal (the caller returns the input unchanged)");
  MG_REQUIRE(mode == 2 || !(Win != Wout && Hin != Hout) || tmp, "resize: fp32 temporary [planes][Hin][Wout] missing");
  if (u8) launch_resample(plane_src<uint8_t>{(const uint8_t*)src}, plane_dst<uint8_t>{(uint8_t*)dst}, tmp, planes, Hin, Win, Hout, Wout, mode, s);
  else launch_resample(plane_src<float>{(const float*)src}, plane_dst<float>{(float*)dst}, tmp, planes, Hin, Win, Hout, Wout, mode, s);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int mg_rgb_prepare(const uint8_t* src, int hwc, int Hin, int Win, void* dst, int out16, int Hout, int Wout, int mode, int reciprocal,
                   float* tmp_or_null, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_RGB_PREP;
  op.p[MG_RGB_PREP_P_SRC] = (void*)src; op.p[MG_RGB_PREP_P_DST] = dst; op.p[MG_RGB_PREP_P_TMP] = tmp_or_null;
  op.i[MG_RGB_PREP_I_HIN] = Hin; op.i[MG_RGB_PREP_I_WIN] = Win; op.i[MG_RGB_PREP_I_HOUT] = Hout; op.i[MG_RGB_PREP_I_WOUT] = Wout;
  op.i[MG_RGB_PREP_I_MODE] = mode; op.i[MG_RGB_PREP_I_HWC] = hwc != 0; op.i[MG_RGB_PREP_I_OUT16] = out16 != 0;
  op.i[MG_RGB_PREP_I_RECIPROCAL] = reciprocal != 0;
  return launch_rgb_prep(&op, (hipStream_t)stream);
}

int mg_normals_finish(const float* pred, int H, int W, float* clipped_out_or_null, uint8_t* picture_out_or_null, void* stream) {
  return launch_normals(pred, H, W, clipped_out_or_null, picture_out_or_null, (hipStream_t)stream);
}

int mg_normals_visualize(const float* pred, int H, int W, uint8_t* out_hwc, void* stream) {
  MG_REQUIRE(out_hwc, "normals_vis: null pointer");
  return mg_normals_finish(pred, H, W, nullptr, out_hwc, stream);
}

int mg_depth_visualize(const float* depth, const uint8_t* lut256x3_or_null, int64_t n, float* clipped_out_or_null, uint16_t* u16_out_or_null,
                       uint8_t* picture_out_or_null, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_COLORIZE;
  op.p[MG_COLORIZE_P_DEPTH] = (void*)depth; op.p[MG_COLORIZE_P_LUT] = (void*)lut256x3_or_null; op.p[MG_COLORIZE_P_OUT] = picture_out_or_null;
  op.p[MG_COLORIZE_P_CLIPPED] = clipped_out_or_null; op.p[MG_COLORIZE_P_U16] = u16_out_or_null;
  op.l[MG_COLORIZE_L_N] = n;
  op.f[MG_COLORIZE_F_MIN_DEPTH] = 0.0f; op.f[MG_COLORIZE_F_MAX_DEPTH] = 1.0f;
  return launch_colorize(&op, (hipStream_t)stream);
}

}  // extern "C"
