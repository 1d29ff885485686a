// Tiled predictions of a large picture: the plan of the tile starts along an axis, the per-tile scale-and-shift fit of
// depth tiles to a low-resolution guide, and the feathered blend of the tiles over the full-size canvas.  The contract of every entry
// point is in include/marigold_hip.h.  The blend is bound by memory: it reads every tile once and writes the canvas once, four pixels per
// lane.  The fit reads every tile once too, but its first launch is slower than that read: the fp64 sampling of the guide (small,
// cache-resident) is the likely bound - measured at 1.5 TB/s of tile bytes (docs/history/tiled.md).  That launch is a
// twenty-thousandth of a tiled prediction, and fp64 is the price of a result that can be checked to 1e-9.
// The file is built with -ffp-contract=off and the blend spells its roundings out; the order of the fit's sums is reduce.h's.
#include "common.h"
#include "reduce.h"

namespace {

struct tile_grid {
  int ys[MG_TILE_MAX_PER_AXIS], xs[MG_TILE_MAX_PER_AXIS];
  int ny, nx;
};

constexpr int FIT_THREADS = 256;
constexpr int FIT_VEC_PER_THREAD = MG_TILE_FIT_CHUNK / 4 / FIT_THREADS;   // float4s a lane takes from its chunk
static_assert(FIT_VEC_PER_THREAD * 4 * FIT_THREADS == MG_TILE_FIT_CHUNK, "a chunk is a whole number of float4s per lane");

// source index and weight of torch's bilinear resampling along one axis (align_corners = False): src = scale (dst + 0.5) - 0.5,
// clamped at 0; i1 = i0 + 1 clamped at the edge
__device__ __forceinline__ void bilinear_src(int dst, double scale, int in, int& i0, int& i1, double& l1) {
  double src = scale * ((double)dst + 0.5) - 0.5;
  src = src < 0.0 ? 0.0 : src;
  i0 = (int)src;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 < in - 1 ? i0 + 1 : i0;
  l1 = src - (double)i0;
  l1 = l1 < 0.0 ? 0.0 : (l1 > 1.0 ? 1.0 : l1);
}

// grid (chunks, n): block (c, i) sums chunk c of tile i -> part[(i * chunks + c) * 5 + {N, Sd, Sg, Sdd, Sdg}]
__global__ __launch_bounds__(FIT_THREADS) void tile_fit_partial_kernel(const float* __restrict__ tiles, int th, int tw, tile_grid g, int Hw,
                                                                       int Ww, const float* __restrict__ guide, int hg, int wg,
                                                                       double* __restrict__ part) {
  const int tile = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
  const int y0 = g.ys[tile / g.nx], x0 = g.xs[tile % g.nx];
  const int nvec = th * tw / 4;   // th tw <= 2^26: pixel and float4 indices fit an int
  const float4* src = (const float4*)(tiles + (long long)tile * th * tw);
  const double sy = (double)hg / (double)Hw, sx = (double)wg / (double)Ww;
  // the lane's float4s first, so that their loads are in flight together; beyond the tile a NaN, which no sum takes
  const float nan = __builtin_nanf("");
  float4 v[FIT_VEC_PER_THREAD];
#pragma unroll
  for (int j = 0; j < FIT_VEC_PER_THREAD; ++j) {
    const int q = chunk * (MG_TILE_FIT_CHUNK / 4) + j * FIT_THREADS + threadIdx.x;
    v[j] = q < nvec ? src[q] : make_float4(nan, nan, nan, nan);
  }
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < FIT_VEC_PER_THREAD; ++j) {
    const int q = chunk * (MG_TILE_FIT_CHUNK / 4) + j * FIT_THREADS + threadIdx.x;
    const int ty = (q * 4) / tw, tx = (q * 4) % tw;   // tw % 4 == 0: the four pixels lie in one row (guide indices are clamped: a q beyond the tile reads inside the guide)
    int r0, r1;
    double ly;
    bilinear_src(y0 + ty, sy, hg, r0, r1, ly);
    const float* g0 = guide + (long long)r0 * wg;
    const float* g1 = guide + (long long)r1 * wg;
    const float d4[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int c0, c1;
      double lx;
      bilinear_src(x0 + tx + k, sx, wg, c0, c1, lx);
      const double top = (1.0 - lx) * (double)g0[c0] + lx * (double)g0[c1];
      const double bot = (1.0 - lx) * (double)g1[c0] + lx * (double)g1[c1];
      const double G = (1.0 - ly) * top + ly * bot;
      const double d = (double)d4[k];
      if (isfinite(d4[k]) && isfinite(G)) {
        acc[0] += 1.0;
        acc[1] += d;
        acc[2] += G;
        acc[3] += d * d;
        acc[4] += d * G;
      }
    }
  }
  block_sum_store<5, FIT_THREADS>(acc, part + ((long long)tile * chunks + chunk) * 5);
}

// one wave per tile: the partials of its chunks, lane-strided (reduce.h), then lane 0 solves
__global__ __launch_bounds__(64) void tile_fit_solve_kernel(const double* __restrict__ part, int chunks, double* __restrict__ coef,
                                                            int* __restrict__ flags) {
  const int tile = blockIdx.x;
  double a[5];
  lane_rows_sum<5>(part + (long long)tile * chunks * 5, chunks, a);
  if (threadIdx.x != 0) return;
  const double N = a[0], Sd = a[1], Sg = a[2], Sdd = a[3], Sdg = a[4];
  double s = 0.0, t = N > 0.0 ? Sg / N : 0.0;
  int flag = 1;
  const scale_shift f = scale_shift_solve(N, Sd, Sg, Sdd, Sdg);
  if (N >= 2.0 && f.det > 1e-12 * N * N && f.s > 0.0) {
    s = f.s;
    t = f.t;
    flag = 0;
  }
  coef[2 * tile] = s;
  coef[2 * tile + 1] = t;
  flags[tile] = flag;
}

// the feather along one axis: u inside the tile of extent T, overlap O (as a float), neighbours before / behind
__device__ __forceinline__ float feather(int u, int T, float O, bool before, bool behind) {
  const float lo = before ? fminf(1.0f, __fdiv_rn((float)u + 0.5f, O)) : 1.0f;              // (u + 0.5 and T - u - 0.5 are exact)
  const float hi = behind ? fminf(1.0f, __fdiv_rn((float)(T - u) - 0.5f, O)) : 1.0f;
  return fminf(lo, hi);
}

// grid (ceil(Ww / 4 / 256), Hw): a lane owns four consecutive x of row y - starts and extents are multiples of 8, so the four see one
// covering set and every access is an aligned float4
template <int C>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int th, int tw, tile_grid g, int Hw, int Ww,
                                                         float oy, float ox, const double* __restrict__ coef, int normalize,
                                                         float* __restrict__ out) {
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
  if (x >= Ww) return;
  float num[C][4], den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) num[c][k] = 0.f;
  for (int iy = 0; iy < g.ny; ++iy) {
    const int uy = y - g.ys[iy];
    if (uy < 0 || uy >= th) continue;   // (uniform over the workgroup)
    const float wy = feather(uy, th, oy, iy > 0, iy < g.ny - 1);
    for (int ix = 0; ix < g.nx; ++ix) {
      const int ux = x - g.xs[ix];
      if (ux < 0 || ux >= tw) continue;
      const int tile = iy * g.nx + ix;
      float s = 1.f, t = 0.f;
      if (coef) {
        s = (float)coef[2 * tile];
        t = (float)coef[2 * tile + 1];
      }
      float w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = __fmul_rn(wy, feather(ux + k, tw, ox, ix > 0, ix < g.nx - 1));
        den[k] = __fadd_rn(den[k], w[k]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float4 d = *(const float4*)(tiles + (((long long)tile * C + c) * th + uy) * tw + ux);
        const float d4[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = coef ? __fmaf_rn(s, d4[k], t) : d4[k];
          num[c][k] = __fmaf_rn(w[k], v, num[c][k]);
        }
      }
    }
  }
  float r[C][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int c = 0; c < C; ++c) r[c][k] = __fdiv_rn(num[c][k], den[k]);
    if constexpr (C == 3) {
      if (normalize) {
        const float sq = __fadd_rn(__fadd_rn(__fmul_rn(r[0][k], r[0][k]), __fmul_rn(r[1][k], r[1][k])), __fmul_rn(r[2][k], r[2][k]));
        const float len = max_keep_nan(__fsqrt_rn(sq), 1e-6f);
#pragma unroll
        for (int c = 0; c < C; ++c) r[c][k] = __fdiv_rn(r[c][k], len);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) *(float4*)(out + ((long long)c * Hw + y) * Ww + x) = make_float4(r[c][0], r[c][1], r[c][2], r[c][3]);
}

// The gather of uint8 tiles out of a picture.  Both layouts are rows of bytes: hwc - a tile is th rows of 3 tw bytes, row r at
// ((y0 + r) Ww + x0) 3 of the picture; chw - 3 th rows of tw bytes, row c th + r at (c Hw + y0 + r) Ww + x0.  In `dst` the rows of a
// tile follow each other without a gap.  Starts and extents are multiples of 8, so every row starts and ends on a multiple of 8 bytes
// from either base: a lane moves one 8-byte word.  VEC: both bases are 8-byte aligned and the word is one load and one store; else
// eight byte loads and stores.  grid (ceil(words per tile / 256), count).
constexpr int CROP_THREADS = 256;
template <bool VEC>
__global__ __launch_bounds__(CROP_THREADS) void tile_crop_kernel(const uint8_t* __restrict__ src, int hwc, int Hw, int Ww, int th, int tw,
                                                                 tile_grid g, int first, uint8_t* __restrict__ dst) {
  const int row_words = (hwc ? 3 * tw : tw) / 8, rows = hwc ? th : 3 * th;
  const int w = blockIdx.x * CROP_THREADS + threadIdx.x;   // (3 th tw / 8 <= 3 * 2^23: word indices fit an int)
  if (w >= rows * row_words) return;
  const int tile = first + blockIdx.y, q = w / row_words, j = w % row_words;
  const int y0 = g.ys[tile / g.nx], x0 = g.xs[tile % g.nx];
  long long from;
  if (hwc) {
    from = ((long long)(y0 + q) * Ww + x0) * 3;
  } else {
    const int c = q / th, r = q % th;
    from = ((long long)c * Hw + y0 + r) * Ww + x0;
  }
  const uint8_t* s = src + from + (long long)j * 8;
  uint8_t* d = dst + (long long)blockIdx.y * 3 * th * tw + (long long)w * 8;
  if constexpr (VEC) {
    *(uint2*)d = *(const uint2*)s;
  } else {
    uint8_t b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = s[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = b[k];
  }
}

// the checks fit and blend share: the extents, the canvas and the starts of one axis (name: "y" / "x")
int check_axis(const char* fn, const char* name, const int* starts, int count, int T, int L) {
  MG_REQUIRE(starts, "%s: null pointer (%sstarts)", fn, name);
  MG_REQUIRE(count >= 1 && count <= MG_TILE_MAX_PER_AXIS, "%s: %d tiles along %s, 1 to %d are supported", fn, count, name, MG_TILE_MAX_PER_AXIS);
  MG_REQUIRE(T >= 8 && T % 8 == 0 && L >= 8 && L % 8 == 0, "%s: the tile extent %d and the canvas length %d along %s must be multiples of 8, 8 at least",
             fn, T, L, name);
  for (int i = 0; i < count; ++i)
    MG_REQUIRE(starts[i] >= 0 && starts[i] <= L - T, "%s: tile %d along %s, [%d, %d), lies outside the canvas [0, %d)", fn, i, name, starts[i],
               starts[i] + T, L);
  return 0;
}

// what the blend asks on top: the tiles cover the axis, in ascending order, on multiples of 8, with the overlap their feathers assume
int check_cover(const char* fn, const char* name, const int* starts, int count, int T, int L, int O) {
  MG_REQUIRE(O >= 8 && O % 8 == 0, "%s: the overlap %d along %s must be a multiple of 8, 8 at least", fn, O, name);
  MG_REQUIRE(count == 1 || 2 * O <= T, "%s: the overlap %d along %s exceeds half the tile extent %d", fn, O, name, T);
  MG_REQUIRE(starts[0] == 0 && starts[count - 1] + T == L, "%s: the tiles along %s cover [%d, %d), the canvas is [0, %d)", fn, name, starts[0],
             starts[count - 1] + T, L);
  for (int i = 0; i < count; ++i) {
    MG_REQUIRE(starts[i] % 8 == 0, "%s: start %d along %s is no multiple of 8", fn, starts[i], name);
    MG_REQUIRE(i == 0 || (starts[i] > starts[i - 1] && starts[i - 1] + T - starts[i] >= O),
               "%s: tiles %d and %d along %s (starts %d, %d) are not ascending with an overlap of at least %d", fn, i - 1, i, name, starts[i ? i - 1 : 0],
               starts[i], O);
  }
  return 0;
}

tile_grid make_grid(const int* ys, int ny, const int* xs, int nx) {
  tile_grid g = {};
  for (int i = 0; i < ny; ++i) g.ys[i] = ys[i];
  for (int i = 0; i < nx; ++i) g.xs[i] = xs[i];
  g.ny = ny;
  g.nx = nx;
  return g;
}

int check_tile_shape(const char* fn, long long n, int th, int tw) {
  MG_REQUIRE(n >= 1 && n <= MG_TILE_MAX_PER_AXIS * MG_TILE_MAX_PER_AXIS, "%s: %lld tiles, 1 to %d are supported", fn, n,
             MG_TILE_MAX_PER_AXIS * MG_TILE_MAX_PER_AXIS);
  MG_REQUIRE(th >= 8 && tw >= 8 && th % 8 == 0 && tw % 8 == 0, "%s: the tile extent %d x %d must be multiples of 8, 8 at least", fn, th, tw);
  MG_REQUIRE((long long)th * tw <= (1ll << 26), "%s: a tile of %d x %d exceeds 2^26 pixels", fn, th, tw);
  return 0;
}

// mg_tile_plan's checks -> the number of tiles along the axis
int plan_count(int L, int T, int O, const int* starts, int cap, int* n) {
  MG_REQUIRE(starts, "mg_tile_plan: null pointer (starts)");
  MG_REQUIRE(L >= 8 && T >= 8 && L % 8 == 0 && T % 8 == 0, "mg_tile_plan: the length %d and the tile length %d must be multiples of 8, 8 at least", L, T);
  MG_REQUIRE(O >= 8 && O % 8 == 0, "mg_tile_plan: the overlap %d must be a multiple of 8, 8 at least", O);
  MG_REQUIRE(2 * O <= T, "mg_tile_plan: the overlap %d exceeds half the tile length %d", O, T);
  *n = L <= T ? 1 : (L - O + (T - O) - 1) / (T - O);   // >= 2 when L > T
  MG_REQUIRE(*n <= MG_TILE_MAX_PER_AXIS, "mg_tile_plan: %d tiles along the axis, at most %d are supported", *n, MG_TILE_MAX_PER_AXIS);
  MG_REQUIRE(*n <= cap, "mg_tile_plan: %d tiles do not fit the %d entries of starts", *n, cap);
  return 0;
}

}  // namespace

extern "C" int mg_tile_plan(int L, int T, int O, int* starts, int cap) {
  int n = 0;
  if (plan_count(L, T, O, starts, cap, &n)) return -1;
  for (int i = 0; i < n - 1; ++i) starts[i] = (int)((long long)i * (L - T) / (n - 1) / 8 * 8);
  starts[n - 1] = n == 1 ? 0 : L - T;
  return n;
}

extern "C" long long mg_tiles_workspace_bytes(int n, int th, int tw) {
  if (check_tile_shape("mg_tiles_workspace_bytes", n, th, tw)) return -1;
  const long long chunks = ((long long)th * tw + MG_TILE_FIT_CHUNK - 1) / MG_TILE_FIT_CHUNK;
  return (long long)n * chunks * 5 * (long long)sizeof(double);
}

extern "C" int mg_tile_fit(const float* tiles, int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx, int Hw, int Ww,
                           const float* guide, int hg, int wg, double* coef, int* flags, void* ws, long long ws_bytes, void* stream) {
  const char* fn = "mg_tile_fit";
  MG_REQUIRE(tiles && guide && coef && flags && ws, "%s: null pointer", fn);
  if (int rc = check_axis(fn, "y", ystarts, ny, th, Hw)) return rc;
  if (int rc = check_axis(fn, "x", xstarts, nx, tw, Ww)) return rc;
  const int n = ny * nx;
  if (int rc = check_tile_shape(fn, n, th, tw)) return rc;
  MG_REQUIRE(hg >= 1 && wg >= 1 && (long long)hg * wg <= (1ll << 26), "%s: bad guide size %d x %d", fn, hg, wg);
  MG_REQUIRE((uintptr_t)tiles % 16 == 0, "%s: the tiles must be 16-byte aligned", fn);
  MG_REQUIRE((uintptr_t)guide % 4 == 0 && (uintptr_t)coef % 8 == 0 && (uintptr_t)flags % 4 == 0,
             "%s: guide, coef and flags must be aligned to their elements", fn);
  MG_REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
  const long long need = mg_tiles_workspace_bytes(n, th, tw);
  MG_REQUIRE(ws_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (mg_tiles_workspace_bytes)", fn, ws_bytes, need);
  const int chunks = (int)(((long long)th * tw + MG_TILE_FIT_CHUNK - 1) / MG_TILE_FIT_CHUNK);
  const tile_grid g = make_grid(ystarts, ny, xstarts, nx);
  MG_LAUNCH(tile_fit_partial_kernel, dim3(chunks, n), dim3(FIT_THREADS), 0, (hipStream_t)stream, tiles, th, tw, g, Hw, Ww, guide, hg, wg,
            (double*)ws);
  MG_LAUNCH(tile_fit_solve_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, (const double*)ws, chunks, coef, flags);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mg_tile_blend(const float* tiles, int C, int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx, int Hw, int Ww,
                             int oy, int ox, const double* coef_or_null, int normalize, float* out, void* stream) {
  const char* fn = "mg_tile_blend";
  MG_REQUIRE(tiles && out, "%s: null pointer", fn);
  MG_REQUIRE(C == 1 || C == 3, "%s: %d channels, 1 (depth) or 3 (normals) are supported", fn, C);
  MG_REQUIRE(normalize == 0 || (normalize == 1 && C == 3), "%s: normalize = %d needs 3 channels and is 0 or 1", fn, normalize);
  if (int rc = check_axis(fn, "y", ystarts, ny, th, Hw)) return rc;
  if (int rc = check_axis(fn, "x", xstarts, nx, tw, Ww)) return rc;
  if (int rc = check_tile_shape(fn, (long long)ny * nx, th, tw)) return rc;
  if (int rc = check_cover(fn, "y", ystarts, ny, th, Hw, oy)) return rc;
  if (int rc = check_cover(fn, "x", xstarts, nx, tw, Ww, ox)) return rc;
  MG_REQUIRE((long long)Hw * Ww <= (1ll << 28) && Hw <= 65535, "%s: a canvas of %d x %d is not supported", fn, Hw, Ww);
  MG_REQUIRE((uintptr_t)tiles % 16 == 0 && (uintptr_t)out % 16 == 0, "%s: tiles and out must be 16-byte aligned", fn);
  MG_REQUIRE((uintptr_t)coef_or_null % 8 == 0, "%s: coef must be aligned to its elements", fn);
  const tile_grid g = make_grid(ystarts, ny, xstarts, nx);
  const dim3 grid((Ww / 4 + 255) / 256, Hw);
  if (C == 1)
    MG_LAUNCH(tile_blend_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, tiles, th, tw, g, Hw, Ww, (float)oy, (float)ox, coef_or_null, normalize, out);
  else
    MG_LAUNCH(tile_blend_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, tiles, th, tw, g, Hw, Ww, (float)oy, (float)ox, coef_or_null, normalize, out);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mg_tile_crop(const uint8_t* src, int hwc, int Hw, int Ww, int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx,
                            int first, int count, uint8_t* dst, void* stream) {
  const char* fn = "mg_tile_crop";
  MG_REQUIRE(src && dst, "%s: null pointer", fn);
  if (int rc = check_axis(fn, "y", ystarts, ny, th, Hw)) return rc;
  if (int rc = check_axis(fn, "x", xstarts, nx, tw, Ww)) return rc;
  if (int rc = check_tile_shape(fn, (long long)ny * nx, th, tw)) return rc;
  for (int i = 0; i < ny; ++i) MG_REQUIRE(ystarts[i] % 8 == 0, "%s: start %d along y is no multiple of 8", fn, ystarts[i]);
  for (int i = 0; i < nx; ++i) MG_REQUIRE(xstarts[i] % 8 == 0, "%s: start %d along x is no multiple of 8", fn, xstarts[i]);
  MG_REQUIRE((long long)Hw * Ww <= (1ll << 28), "%s: a canvas of %d x %d is not supported", fn, Hw, Ww);
  MG_REQUIRE(first >= 0 && count >= 1 && (long long)first + count <= (long long)ny * nx, "%s: tiles [%d, %d + %d) of a grid of %d x %d", fn, first,
             first, count, ny, nx);
  const tile_grid g = make_grid(ystarts, ny, xstarts, nx);
  const dim3 grid((3 * th * tw / 8 + CROP_THREADS - 1) / CROP_THREADS, count);   // (th tw <= 2^26; count <= 1024)
  if ((uintptr_t)src % 8 == 0 && (uintptr_t)dst % 8 == 0)
    MG_LAUNCH(tile_crop_kernel<true>, grid, dim3(CROP_THREADS), 0, (hipStream_t)stream, src, hwc, Hw, Ww, th, tw, g, first, dst);
  else
    MG_LAUNCH(tile_crop_kernel<false>, grid, dim3(CROP_THREADS), 0, (hipStream_t)stream, src, hwc, Hw, Ww, th, tw, g, first, dst);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
