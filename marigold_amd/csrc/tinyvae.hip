// The tiny autoencoder (diffusers AutoencoderTiny / TAESD, restated in DESIGN.md "Tiny VAE"): thirty-odd 3x3 / pad-1 / 64 -> 64
// convolutions with ReLU, no GroupNorm, no attention - a layer neither the implicit GEMM (no ReLU epilogue, N tile 128) nor the
// patch kernels (128 channels and up) serve.  One hot kernel, tiny_conv_kernel, and two small ones for the four boundary layers.
//
// tiny_conv_kernel: a persistent grid of four-wave workgroups, one per CU.
//   LDS   [all nine taps' weights, 576 rows x 128 B = 73 728 B, staged once per workgroup | patch buffer 0 | patch buffer 1]
//   tile  stride 1: 8 x 32 output pixels, wave w owns rows 2w, 2w + 1 (two pixel fragments x two channel fragments of 32 x 32);
//         stride 2: 2 x 32 output pixels, wave w owns row w / 2 and channels 32 (w % 2) ...
//   loop  for each tile of this workgroup: { wait for its patch (LDS-DMA, issued one tile ahead) | barrier | issue the next tile's
//         patch into the other buffer | nine taps x four 16-channel steps of MFMAs on shifted fragment addresses | epilogue }
// One pixel is one 128-byte LDS row; the 16-byte slot of row r is XOR-swizzled with (r >> 1) & 7 on the DMA's source address and
// undone in the fragment read (conv_patch.hip's scheme).  The patch is laid out in the coordinates the convolution reads: with
// nearest x2 fused, patch entry (y, x) is fetched from input pixel (y >> 1, x >> 1) and no up-sampled tensor exists; padding
// entries come from the zero page.  No im2col in memory, no split-K, no atomics: one workgroup owns an output pixel and sums it in a
// fixed order, so a launch repeats bit for bit and a member's result does not depend on its batch.
// Epilogue: + fp32 bias, + residual (operand-typed, at the output's pixel), ReLU (NaN kept, as torch.relu), one rounding.
#include "common.h"

namespace {

constexpr int TV_WROWS = 9 * 64;                        // weight rows: tap * 64 + output channel
constexpr int TV_WBYTES = TV_WROWS * 128;
constexpr int TV_PROWS = 344;                           // patch rows per buffer: 10 x 34 (stride 1), 5 x 65 (stride 2) in whole 8-row pieces
constexpr int TV_PBYTES = TV_PROWS * 128;
constexpr int TV_LDS = TV_WBYTES + 2 * TV_PBYTES;       // 161 792 B
static_assert(TV_LDS <= 160 * 1024, "LDS budget exceeds 160 KiB");

struct TinyConvArgs {
  const bf16_t* x;      // [B][Hin][Win][64]
  const bf16_t* w;      // [9][64 out][64 in]
  const float* bias;    // [64] | NULL
  const bf16_t* res;    // [B][Ho][Wo][64] | NULL
  bf16_t* out;          // [B][Ho][Wo][64]
  const void* zero;
  int B, Hin, Win, Ho, Wo, tiles_x, tiles_y, ntiles, relu;
};

// round to nearest even, NaN and +-inf kept in both operand types (an overflow is an inf here: the network has no value near it)
__device__ __forceinline__ uint32_t tv_pack2(float lo, float hi) {
  const mg_f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, mg_bf16x2_t));
}
__device__ __forceinline__ float tv_relu(float v) { return v < 0.f ? 0.f : v; }   // NaN < 0 is false: kept

template <int S, int UP>
__global__ __launch_bounds__(256) void tiny_conv_kernel(const TinyConvArgs a) {
  constexpr int TW = 32, TH = S == 1 ? 8 : 2;
  constexpr int WN = S == 1 ? 1 : 2, WM = 4 / WN;        // waves over channels / over rows
  constexpr int MI = TH / WM, NI = 2 / WN;               // 32-pixel rows / 32-channel fragments per wave
  constexpr int PH = (TH - 1) * S + 3, PW = (TW - 1) * S + 3, PR = PH * PW;
  constexpr int NPIECE = (PR + 7) / 8;                   // 8-row (1 KiB) DMA pieces per patch
  static_assert(UP == 0 || S == 1, "nearest x2 is fused into the stride-1 form only");
  static_assert(NPIECE * 8 <= TV_PROWS, "patch buffer");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sW = smem;
  char* const sP0 = smem + TV_WBYTES;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;
  const int Hv = a.Hin << UP, Wv = a.Win << UP;          // the size the convolution reads
  const char* const zero = (const char*)a.zero;

  auto stage_patch = [&](int tile, int buf) {
    const int tx = tile % a.tiles_x;
    const int t2 = tile / a.tiles_x;
    const int ty = t2 % a.tiles_y, img = t2 / a.tiles_y;
    const int iy0 = ty * TH * S - 1, ix0 = tx * TW * S - 1;
#pragma unroll
    for (int k = 0; k < (NPIECE + 3) / 4; ++k) {
      const int i = k * 4 + wave;
      if (i >= NPIECE) break;                              // wave-uniform
      const int r = i * 8 + (lane >> 3);
      const int pr = r / PW, pc = r - pr * PW;
      const int iy = iy0 + pr, ix = ix0 + pc;
      const char* src = zero;
      if (r < PR && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv) {
        const long long pix = ((long long)img * a.Hin + (iy >> UP)) * a.Win + (ix >> UP);
        src = (const char*)(a.x + pix * 64 + (((lane & 7) ^ ((r >> 1) & 7)) << 3));
      }
      glds16(src, sP0 + buf * TV_PBYTES + i * 1024);
    }
  };

  // ---- all nine taps' weights, once per workgroup ----
#pragma unroll
  for (int k = 0; k < TV_WROWS / 8 / 4; ++k) {
    const int i = k * 4 + wave;
    const int r = i * 8 + (lane >> 3);
    glds16(a.w + r * 64 + (((lane & 7) ^ ((r >> 1) & 7)) << 3), sW + i * 1024);
  }
  int tile = blockIdx.x;
  if (tile < a.ntiles) stage_patch(tile, 0);

  for (int buf = 0; tile < a.ntiles; tile += gridDim.x, buf ^= 1) {
    // this tile's patch (and the weights) have landed; every wave is past its reads of the other buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (tile + (int)gridDim.x < a.ntiles) stage_patch(tile + gridDim.x, buf ^ 1);

    const char* const sP = sP0 + buf * TV_PBYTES;
    f32x16 acc[NI][MI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ni][mi][r] = 0.f;

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - dy * 3;
      int abase[MI], af[MI], bbase[NI], bf[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int r = ((wm * MI + mi) * S + dy) * PW + l31 * S + dx;
        abase[mi] = r * 128;
        af[mi] = ((r >> 1) & 7) << 4;
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int r = tap * 64 + (wn * NI + ni) * 32 + l31;
        bbase[ni] = r * 128;
        bf[ni] = ((r >> 1) & 7) << 4;
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int q16 = (ks * 2 + half) << 4;              // channels 16 ks + 8 half ... + 7
        bf16x8 fa[MI], fb[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) fa[mi] = __builtin_bit_cast(bf16x8, *(const uint4*)(sP + abase[mi] + (af[mi] ^ q16)));
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) fb[ni] = __builtin_bit_cast(bf16x8, *(const uint4*)(sW + bbase[ni] + (bf[ni] ^ q16)));
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = mg_mfma32(fb[ni], fa[mi], acc[ni][mi]);   // rows: channels, columns: pixels
      }
    }

    // ---- epilogue: lane (l31, half) ends up with 8 consecutive channels of pixel l31 (the regroup of conv_patch.hip) ----
    const int tx = tile % a.tiles_x;
    const int t2 = tile / a.tiles_x;
    const int ty = t2 % a.tiles_y, img = t2 / a.tiles_y;
    const int ox = tx * TW + l31;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int oy = ty * TH + wm * MI + mi;
      const bool pix_ok = oy < a.Ho && ox < a.Wo;
      const long long orow = (((long long)img * a.Ho + oy) * a.Wo + ox) * 64;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) half_swap(acc[ni][mi][8 * gp + j], acc[ni][mi][8 * gp + 4 + j], v[j], v[4 + j]);
          const int n = (wn * NI + ni) * 32 + 16 * gp + 8 * half;
          if (pix_ok) {
            if (a.bias) mg_add8(v, a.bias + n);
            if (a.res) mg_add8(v, *(const uint4*)(a.res + orow + n));
            if (a.relu) {
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = tv_relu(v[j]);
            }
            uint4 pk;
            pk.x = tv_pack2(v[0], v[1]); pk.y = tv_pack2(v[2], v[3]);
            pk.z = tv_pack2(v[4], v[5]); pk.w = tv_pack2(v[6], v[7]);
            *(uint4*)(a.out + orow + n) = pk;
          }
        }
      }
    }
  }
}

// ---- the first layer of either half: fp32 NCHW [B][CIN][H][W] -> map -> 3x3 / pad 1 -> 64 channels, operand-typed NHWC ----
// MAP 0: (x + 1) / 2 (the encoder's image), 1: 3 tanh(z / 3) (the decoder's latent); the padding is zero AFTER the map.
// One pixel per lane; the weights are wave-uniform (scalar loads).  fp32 [9 * CIN][64], row tap * CIN + ci.
template <int CIN, int MAP>
__global__ __launch_bounds__(256) void tiny_first_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ out, int B, int H, int W,
                                                         int relu) {
  const long long npix = (long long)B * H * W;
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const long long hw = (long long)H * W;
  const int b = (int)(pix / hw);
  const int p = (int)(pix - b * hw);
  const int y = p / W, xx = p - y * W;
  float in[9 * CIN];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int iy = y + t / 3 - 1, ix = xx + t % 3 - 1;
    const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      float v = 0.f;
      if (ok) {
        v = x[((long long)b * CIN + c) * hw + (long long)iy * W + ix];
        v = MAP == 0 ? (v + 1.0f) * 0.5f : 3.0f * tanhf(v / 3.0f);
      }
      in[t * CIN + c] = v;
    }
  }
  bf16_t* const o = out + pix * 64;
#pragma unroll
  for (int n8 = 0; n8 < 64; n8 += 8) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 9 * CIN; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(in[k], w[k * 64 + n8 + j], acc[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[j] += bias[n8 + j];
      if (relu) acc[j] = tv_relu(acc[j]);
    }
    uint4 pk;
    pk.x = tv_pack2(acc[0], acc[1]); pk.y = tv_pack2(acc[2], acc[3]);
    pk.z = tv_pack2(acc[4], acc[5]); pk.w = tv_pack2(acc[6], acc[7]);
    *(uint4*)(o + n8) = pk;
  }
}

// ---- the last layer of either half: operand-typed NHWC 64 channels -> 3x3 / pad 1 -> COUT <= 4 channels, fp32 NCHW ----
// weights fp32 [9][64][4] (columns >= COUT zero), bias fp32 [4].  DEC: y 2 - 1 and the MG_POST_* tail of MG_OP_POST_NCHW (misc.hip),
// NaN rules included.
template <int COUT, bool DEC>
__global__ __launch_bounds__(256) void tiny_last_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, int B, int H, int W,
                                                        int post) {
  const long long npix = (long long)B * H * W;
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const long long HW = (long long)H * W;
  const long long b = pix / HW, p = pix - b * HW;
  const int y = (int)(p / W), xx = (int)(p - (long long)y * W);
  float acc[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc[co] = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int iy = y + t / 3 - 1, ix = xx + t % 3 - 1;
    if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
    const uint4* src = (const uint4*)(x + ((b * H + iy) * W + ix) * 64);
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
      float v[8];
      mg_unpack8(src[c8], v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] = __builtin_fmaf(v[j], w[((t * 64 + c8 * 8 + j) << 2) + co], acc[co]);
    }
  }
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc[co] += bias[co];
  if constexpr (!DEC) {
#pragma unroll
    for (int co = 0; co < COUT; ++co) out[(b * COUT + co) * HW + p] = acc[co];
  } else {
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = acc[co] * 2.0f - 1.0f;
    if (post == MG_POST_DEPTH) {
      float m = 0.f;
#pragma unroll
      for (int co = 0; co < COUT; ++co) m += acc[co];
      m = m / (float)COUT;
      m = clip_keep_nan(m, -1.f, 1.f);
      out[b * HW + p] = (m + 1.0f) * 0.5f;
    } else if (post == MG_POST_NORMALS) {
      float n2 = 0.f;
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        acc[co] = clip_keep_nan(acc[co], -1.f, 1.f);
        n2 += acc[co] * acc[co];
      }
      const float inv = 1.0f / floor_keep_nan(sqrtf(n2), 1e-6f);
#pragma unroll
      for (int co = 0; co < COUT; ++co) out[(b * COUT + co) * HW + p] = acc[co] * inv;
    } else if (post == MG_POST_UNIT) {
#pragma unroll
      for (int co = 0; co < COUT; ++co) out[(b * COUT + co) * HW + p] = (clip_keep_nan(acc[co], -1.f, 1.f) + 1.0f) * 0.5f;
    } else {
#pragma unroll
      for (int co = 0; co < COUT; ++co) out[(b * COUT + co) * HW + p] = acc[co];
    }
  }
}

constexpr long long TV_MAX_PIXELS = 1ll << 26;   // B H W of the largest level: 64-bit element offsets, 31-bit grids

template <int S, int UP>
int launch_tiny_conv(TinyConvArgs a, hipStream_t s) {
  constexpr int TH = S == 1 ? 8 : 2;
  a.tiles_x = (a.Wo + 31) / 32;
  a.tiles_y = (a.Ho + TH - 1) / TH;
  const long long nt = (long long)a.tiles_x * a.tiles_y * a.B;
  MG_REQUIRE(nt > 0 && nt < (1ll << 31), "tiny conv3x3: bad tile count %lld", nt);
  a.ntiles = (int)nt;
  const int grid = (int)(nt < mg_cu_count() ? nt : mg_cu_count());
  void (*kern)(const TinyConvArgs) = tiny_conv_kernel<S, UP>;
  MG_KERNEL_MAX_LDS((const void*)kern, TV_LDS);
  MG_LAUNCH(kern, dim3((unsigned)grid), dim3(256), TV_LDS, s, a);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

// one 64 -> 64 layer; every argument has been checked by the caller
int tiny_conv(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int H, int W, int stride, int up2, int relu,
              hipStream_t s) {
  TinyConvArgs a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.res = (const bf16_t*)res; a.out = (bf16_t*)out; a.zero = g_zero_page;
  a.B = B; a.Hin = H; a.Win = W; a.relu = relu;
  a.Ho = stride == 2 ? (H - 1) / 2 + 1 : H << up2;
  a.Wo = stride == 2 ? (W - 1) / 2 + 1 : W << up2;
  a.tiles_x = a.tiles_y = a.ntiles = 0;
  if (stride == 2) return launch_tiny_conv<2, 0>(a, s);
  return up2 ? launch_tiny_conv<1, 1>(a, s) : launch_tiny_conv<1, 0>(a, s);
}

bool tv_size_ok(int which, int B, int H, int W) {   // H, W: the image (encode) or the latent (decode)
  if ((which != 0 && which != 1) || B < 1 || H < 1 || W < 1) return false;
  const long long full = (long long)B * H * W * (which == 1 ? 64 : 1);
  return H <= (1 << 16) && W <= (1 << 16) && full <= TV_MAX_PIXELS;
}

// a residual block on three rotating buffers: cur -> t1 -> t2 -> t1 (+ cur); returns the buffer that holds the result
int tiny_block(const void* const* w, const float* const* b, char** buf, int* cur, int B, int H, int W, hipStream_t s) {
  const int c = *cur, t1 = (c + 1) % 3, t2 = (c + 2) % 3;
  if (const int rc = tiny_conv(buf[c], w[0], b[0], nullptr, buf[t1], B, H, W, 1, 0, 1, s)) return rc;
  if (const int rc = tiny_conv(buf[t1], w[1], b[1], nullptr, buf[t2], B, H, W, 1, 0, 1, s)) return rc;
  if (const int rc = tiny_conv(buf[t2], w[2], b[2], buf[c], buf[t1], B, H, W, 1, 0, 1, s)) return rc;
  *cur = t1;
  return 0;
}

long long tv_level_bytes(int which, int B, int H, int W) {
  const long long full = (long long)B * H * W * (which == 1 ? 64 : 1);
  return (full * 128 + 255) / 256 * 256;
}

int tv_check_half(const char* what, const float* in_w, const float* in_b, const void* const* w, const float* const* b, const float* out_w,
                  const float* out_b, int plain /* index of the first bias-free layer */) {
  MG_REQUIRE(in_w && in_b && out_w && out_b, "%s: null pointer in the network (boundary layers)", what);
  MG_REQUIRE(((uintptr_t)in_w | (uintptr_t)in_b | (uintptr_t)out_w | (uintptr_t)out_b) % 16 == 0, "%s: network weights not 16-byte aligned", what);
  for (int l = 0; l < MG_TINY_VAE_LAYERS; ++l) {
    const bool no_bias = l >= plain && (l - plain) % 10 == 0;
    MG_REQUIRE(w[l] && (no_bias || b[l]), "%s: null pointer in the network (layer %d)", what, l);
    MG_REQUIRE(((uintptr_t)w[l] | (uintptr_t)b[l]) % 16 == 0, "%s: network weights not 16-byte aligned (layer %d)", what, l);
  }
  return 0;
}

}  // namespace

long long mg_tiny_vae_workspace_bytes(int which, int B, int H, int W) {
  if (!tv_size_ok(which, B, H, W)) {
    mg_set_error("mg_tiny_vae_workspace_bytes: which 0 (encode: image size) or 1 (decode: latent size), B, H, W >= 1 and at most 2^26 "
                 "full-size pixels required, got which %d, %d x %d x %d", which, B, H, W);
    return -1;
  }
  return 3 * tv_level_bytes(which, B, H, W);
}

int mg_tiny_conv3x3(const void* x, const void* w, const float* bias_or_null, const void* residual_or_null, void* out, int B, int H, int W,
                    int stride, int up2, int relu, void* stream) {
  MG_REQUIRE(x && w && out, "mg_tiny_conv3x3: null pointer");
  MG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "mg_tiny_conv3x3: B, H, W >= 1 required, got %d x %d x %d", B, H, W);
  MG_REQUIRE((stride == 1 && (up2 == 0 || up2 == 1)) || (stride == 2 && up2 == 0),
             "mg_tiny_conv3x3: stride 1 (up2 0 or 1) or stride 2 (up2 0) required, got stride %d, up2 %d", stride, up2);
  MG_REQUIRE(H <= (1 << 16) && W <= (1 << 16) && (long long)B * H * W * (up2 ? 4 : 1) <= TV_MAX_PIXELS,
             "mg_tiny_conv3x3: at most 2^26 pixels, got %d x %d x %d", B, H, W);
  MG_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)out | (uintptr_t)residual_or_null | (uintptr_t)bias_or_null) % 16 == 0,
             "mg_tiny_conv3x3: pointers need 16-byte alignment");
  MG_REQUIRE(out != x && out != residual_or_null, "mg_tiny_conv3x3: out may not alias an input (a tile reads its neighbours' pixels)");
  MG_REQUIRE(g_zero_page || g_dry_run, "mg_tiny_conv3x3: mg_init() not called");
  return tiny_conv(x, w, bias_or_null, residual_or_null, out, B, H, W, stride, up2, relu != 0, (hipStream_t)stream);
}

int mg_tiny_vae_encode(const mg_tiny_vae* net, const float* rgb, float* latent, int B, int H, int W, void* ws, long long ws_bytes,
                       void* stream) {
  MG_REQUIRE(net && rgb && latent && ws, "mg_tiny_vae_encode: null pointer");
  if (const int rc = tv_check_half("mg_tiny_vae_encode", net->enc_in_w, net->enc_in_b, net->enc_w, net->enc_b, net->enc_out_w, net->enc_out_b, 3))
    return rc;
  MG_REQUIRE(tv_size_ok(0, B, H, W), "mg_tiny_vae_encode: B, H, W >= 1 and at most 2^26 pixels required, got %d x %d x %d", B, H, W);
  MG_REQUIRE(((uintptr_t)rgb | (uintptr_t)latent) % 4 == 0 && (uintptr_t)ws % 16 == 0, "mg_tiny_vae_encode: rgb / latent not 4-byte or workspace not 16-byte aligned");
  const long long level = tv_level_bytes(0, B, H, W);
  MG_REQUIRE(ws_bytes >= 3 * level, "mg_tiny_vae_encode: workspace too small: %lld bytes, %d x %d x %d needs %lld", ws_bytes, B, H, W, 3 * level);
  MG_REQUIRE(g_zero_page || g_dry_run, "mg_tiny_vae_encode: mg_init() not called");
  hipStream_t s = (hipStream_t)stream;
  char* buf[3] = {(char*)ws, (char*)ws + level, (char*)ws + 2 * level};
  int cur = 0, h = H, w = W;
  const unsigned grid = (unsigned)(((long long)B * H * W + 255) / 256);
  MG_LAUNCH((tiny_first_kernel<3, 0>), dim3(grid), dim3(256), 0, s, rgb, net->enc_in_w, net->enc_in_b, (bf16_t*)buf[0], B, H, W, 0);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  int l = 0;
  if (const int rc = tiny_block(net->enc_w + l, net->enc_b + l, buf, &cur, B, h, w, s)) return rc;
  l += 3;
  for (int level_i = 0; level_i < 3; ++level_i) {
    const int nxt = (cur + 1) % 3;
    if (const int rc = tiny_conv(buf[cur], net->enc_w[l], nullptr, nullptr, buf[nxt], B, h, w, 2, 0, 0, s)) return rc;
    cur = nxt; ++l;
    h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1;
    for (int k = 0; k < 3; ++k, l += 3)
      if (const int rc = tiny_block(net->enc_w + l, net->enc_b + l, buf, &cur, B, h, w, s)) return rc;
  }
  const unsigned gl = (unsigned)(((long long)B * h * w + 255) / 256);
  MG_LAUNCH((tiny_last_kernel<4, false>), dim3(gl), dim3(256), 0, s, (const bf16_t*)buf[cur], net->enc_out_w, net->enc_out_b, latent, B, h, w, 0);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

int mg_tiny_vae_decode(const mg_tiny_vae* net, const float* latent, float* out, int B, int h, int w, int post, void* ws, long long ws_bytes,
                       void* stream) {
  MG_REQUIRE(net && latent && out && ws, "mg_tiny_vae_decode: null pointer");
  if (const int rc = tv_check_half("mg_tiny_vae_decode", net->dec_in_w, net->dec_in_b, net->dec_w, net->dec_b, net->dec_out_w, net->dec_out_b, 9))
    return rc;
  MG_REQUIRE(tv_size_ok(1, B, h, w), "mg_tiny_vae_decode: B, h, w >= 1 and at most 2^26 decoded pixels required, got %d x %d x %d", B, h, w);
  MG_REQUIRE(post == MG_POST_NONE || post == MG_POST_DEPTH || post == MG_POST_NORMALS || post == MG_POST_UNIT,
             "mg_tiny_vae_decode: unknown post %d (MG_POST_NONE, _DEPTH, _NORMALS or _UNIT)", post);
  MG_REQUIRE(((uintptr_t)latent | (uintptr_t)out) % 4 == 0 && (uintptr_t)ws % 16 == 0, "mg_tiny_vae_decode: latent / out not 4-byte or workspace not 16-byte aligned");
  const long long level = tv_level_bytes(1, B, h, w);
  MG_REQUIRE(ws_bytes >= 3 * level, "mg_tiny_vae_decode: workspace too small: %lld bytes, %d x %d x %d needs %lld", ws_bytes, B, h, w, 3 * level);
  MG_REQUIRE(g_zero_page || g_dry_run, "mg_tiny_vae_decode: mg_init() not called");
  hipStream_t s = (hipStream_t)stream;
  char* buf[3] = {(char*)ws, (char*)ws + level, (char*)ws + 2 * level};
  int cur = 0, H = h, W = w;
  const unsigned grid = (unsigned)(((long long)B * h * w + 255) / 256);
  MG_LAUNCH((tiny_first_kernel<4, 1>), dim3(grid), dim3(256), 0, s, latent, net->dec_in_w, net->dec_in_b, (bf16_t*)buf[0], B, h, w, 1);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  int l = 0;
  for (int level_i = 0; level_i < 3; ++level_i) {
    for (int k = 0; k < 3; ++k, l += 3)
      if (const int rc = tiny_block(net->dec_w + l, net->dec_b + l, buf, &cur, B, H, W, s)) return rc;
    const int nxt = (cur + 1) % 3;
    if (const int rc = tiny_conv(buf[cur], net->dec_w[l], nullptr, nullptr, buf[nxt], B, H, W, 1, 1, 0, s)) return rc;
    cur = nxt; ++l;
    H *= 2; W *= 2;
  }
  if (const int rc = tiny_block(net->dec_w + l, net->dec_b + l, buf, &cur, B, H, W, s)) return rc;
  const unsigned gl = (unsigned)(((long long)B * H * W + 255) / 256);
  MG_LAUNCH((tiny_last_kernel<3, true>), dim3(gl), dim3(256), 0, s, (const bf16_t*)buf[cur], net->dec_out_w, net->dec_out_b, out, B, H, W, post);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
