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

__device__ __forceinline__ float ld(const uint8_t* p, long long i) { return (float)p[i]; }
__device__ __forceinline__ float ld(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ void st(float* p, long long i, float v, int) { p[i] = v; }
__device__ __forceinline__ void st(uint8_t* p, long long i, float v, int bicubic) {
  if (bicubic) v = fminf(fmaxf(v, 0.0f), 255.0f);
  p[i] = (uint8_t)rintf(v);  // round half to even, like torch.round()
}

// One output element per thread.  The resampled axis has `in_len` -> `out_len` elements with element
// stride `s_axis`; the other in-plane axis has `other` elements with stride `s_other`; planes are
// contiguous (`plane_in` / `plane_out` elements).  Output is [planes][out rows][out cols] row-major.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void resize_aa_pass_kernel(const TI* __restrict__ src, TO* __restrict__ dst,
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
    const float v = ld(src, sidx) * w;
    t = j == 0 ? v : t + v;
  }
  st(dst, idx, t, bicubic);
}

template <typename T>
__global__ __launch_bounds__(256) void resize_nearest_exact_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                                   long long total, int Hin, int Win, int Hout,
                                                                   int Wout, float sy, float sx) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % Wout), y = (int)((idx / Wout) % Hout);
  const long long plane = idx / ((long long)Wout * Hout);
  int iy = (int)floorf(((float)y + 0.5f) * sy), ix = (int)floorf(((float)x + 0.5f) * sx);
  iy = iy < Hin - 1 ? iy : Hin - 1;
  ix = ix < Win - 1 ? ix : Win - 1;
  dst[idx] = src[(plane * Hin + iy) * Win + ix];
}

template <typename TI, typename TO>
void launch_pass(const void* src, void* dst, long long total, int in_len, int out_len, int other, int horizontal,
                 int bicubic, hipStream_t s) {
  const float scale = (float)in_len / (float)out_len;
  MG_LAUNCH((resize_aa_pass_kernel<TI, TO>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const TI*)src,
            (TO*)dst, total, in_len, out_len, other, horizontal, bicubic, scale);
}

}  // namespace

// Colour-mapped depth (marigold/util/image_util.py:38-76 colorize_depth_maps + the pipeline's (x * 255).astype(uint8),
// marigold_depth_pipeline.py:318-327): matplotlib's listed / segmented colormaps are 256-entry tables indexed by
// int(x * 256) (x == 1 -> 255); the table arrives as uint8 RGB (built once per colormap on the host from matplotlib
// itself), the output is the HWC uint8 image PIL takes.
__global__ __launch_bounds__(256) void colorize_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ lut,
                                                       uint8_t* __restrict__ out, long long n, float lo, float inv_range) {
  __shared__ uint8_t tab[768];
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float x = (depth[i] - lo) * inv_range;
    const bool bad = x != x;   // matplotlib's "bad" colour, RGBA (0, 0, 0, 0): a NaN depth is a black pixel, not entry 0 of the table
    x = fminf(fmaxf(x, 0.f), 1.f);
    int k = (int)(x * 256.0f);
    k = k > 255 ? 255 : k;
    out[3 * i + 0] = bad ? (uint8_t)0 : tab[3 * k + 0];
    out[3 * i + 1] = bad ? (uint8_t)0 : tab[3 * k + 1];
    out[3 * i + 2] = bad ? (uint8_t)0 : tab[3 * k + 2];
  }
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
  const int n = op->i[0], H = op->i[1], W = op->i[2];
  const unsigned linear = (unsigned)op->i[3], up_to_scale = (unsigned)op->i[4];
  MG_REQUIRE(n >= 1 && n <= 16, "iid_vis: 1 to 16 targets per launch (got %d)", n);
  MG_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1ll << 30), "iid_vis: bad size %d x %d", H, W);
  MG_REQUIRE(!((linear | up_to_scale) >> n), "iid_vis: a flag names a target beyond the %d given", n);
  MG_REQUIRE(op->p[0] && op->p[1], "iid_vis: null pointer");
  MG_REQUIRE((uintptr_t)op->p[0] % 4 == 0, "iid_vis: the prediction must be 4-byte aligned");
  const unsigned need = linear & up_to_scale;   // the maximum is used by the linear, up-to-scale targets only
  MG_REQUIRE(!need || (op->p[2] && (uintptr_t)op->p[2] % 4 == 0), "iid_vis: null or unaligned workspace (f32 [n][MG_IID_VIS_PARTS])");
  const long long HW = (long long)H * W;
  const int vec = HW % 4 == 0 && (uintptr_t)op->p[0] % 16 == 0 && (uintptr_t)op->p[1] % 4 == 0;
  // a thread of the maximum takes at least 16 elements; the partial rows have MG_IID_VIS_PARTS slots
  const int parts = (int)min((3 * HW + 16 * IV_THREADS - 1) / (16 * IV_THREADS), (long long)MG_IID_VIS_PARTS);
  if (need)
    MG_LAUNCH(iid_vis_max_kernel, dim3(parts, n), dim3(IV_THREADS), 0, s, (const float*)op->p[0], (float*)op->p[2], 3 * HW, need, vec);
  const long long work = vec ? HW / 4 : HW;
  MG_LAUNCH(iid_vis_map_kernel, dim3((unsigned)min((work + IV_THREADS - 1) / IV_THREADS, (long long)1024), n), dim3(IV_THREADS), 0, s,
            (const float*)op->p[0], (const float*)op->p[2], (uint8_t*)op->p[1], HW, parts, linear, up_to_scale, vec);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

int mg_launch_resize(const mg_op* op, hipStream_t s) {
  if (op->kind == MG_OP_IID_VIS) return launch_iid_vis(op, s);
  if (op->kind == MG_OP_COLORIZE) {
    const long long n = op->l[0];
    MG_REQUIRE(n > 0 && op->p[0] && op->p[1] && op->p[2], "colorize: null pointer / empty map");
    MG_REQUIRE(op->f[1] > op->f[0], "colorize: max_depth must exceed min_depth");
    MG_LAUNCH(colorize_kernel, dim3((unsigned)min((n + 255) / 256, (long long)4096)), dim3(256), 0, s, (const float*)op->p[0],
              (const uint8_t*)op->p[1], (uint8_t*)op->p[2], n, op->f[0], 1.0f / (op->f[1] - op->f[0]));
    if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const long long planes = op->i[0];
  const int Hin = op->i[1], Win = op->i[2], Hout = op->i[3], Wout = op->i[4], mode = op->i[5];
  const int u8 = op->i[6];  // 1: uint8 in and out, 0: fp32
  MG_REQUIRE(planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "resize: empty image");
  MG_REQUIRE(mode >= 0 && mode <= 2, "resize: mode must be 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)");
  MG_REQUIRE(op->p[0] && op->p[1], "resize: null pointer");
  if (mode == 2) {
    const long long total = planes * Hout * Wout;
    const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (u8) MG_LAUNCH(resize_nearest_exact_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)op->p[0],
                      (uint8_t*)op->p[1], total, Hin, Win, Hout, Wout, sy, sx);
    else MG_LAUNCH(resize_nearest_exact_kernel<float>, grid, dim3(256), 0, s, (const float*)op->p[0],
                   (float*)op->p[1], total, Hin, Win, Hout, Wout, sy, sx);
  } else {
    const int bicubic = mode == 1;
    const bool do_h = Win != Wout, do_v = Hin != Hout;
    MG_REQUIRE(!(do_h && do_v) || op->p[2], "resize: fp32 temporary [planes][Hin][Wout] missing");
    // horizontal first (rows = Hin), then vertical on the result - torch's order
    if (do_h && do_v) {
      if (u8) launch_pass<uint8_t, float>(op->p[0], op->p[2], planes * Hin * Wout, Win, Wout, Hin, 1, bicubic, s);
      else launch_pass<float, float>(op->p[0], op->p[2], planes * Hin * Wout, Win, Wout, Hin, 1, bicubic, s);
      if (u8) launch_pass<float, uint8_t>(op->p[2], op->p[1], planes * Hout * Wout, Hin, Hout, Wout, 0, bicubic, s);
      else launch_pass<float, float>(op->p[2], op->p[1], planes * Hout * Wout, Hin, Hout, Wout, 0, bicubic, s);
    } else if (do_h) {
      if (u8) launch_pass<uint8_t, uint8_t>(op->p[0], op->p[1], planes * Hin * Wout, Win, Wout, Hin, 1, bicubic, s);
      else launch_pass<float, float>(op->p[0], op->p[1], planes * Hin * Wout, Win, Wout, Hin, 1, bicubic, s);
    } else if (do_v) {
      if (u8) launch_pass<uint8_t, uint8_t>(op->p[0], op->p[1], planes * Hout * Wout, Hin, Hout, Wout, 0, bicubic, s);
      else launch_pass<float, float>(op->p[0], op->p[1], planes * Hout * Wout, Hin, Hout, Wout, 0, bicubic, s);
    } else {
      MG_REQUIRE(false, "resize: sizes are equal (the caller returns the input unchanged)");
    }
  }
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
