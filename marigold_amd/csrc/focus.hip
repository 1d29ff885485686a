// Depth to focus: the picture refocused from its depth map - mg_depth_focus, a synthetic shallow depth of field.  The
// definitions (focus distance, blur radius, bad focus, order, contribution, weight, result, outputs) and the contract are in
// include/marigold_hip.h, block DEPTH TO FOCUS; depth, z, usable, coef, mask and the range are depth3d.h's.
// Three launches, none of which waits on another workgroup; only stream order separates them:
//   1. `count` to zeros;
//   2. the prepare: one lane per pixel decides whether it is usable, reads the focus distance (from the focus pixel, on the device, or
//      from the argument), computes r16 in fp64 and writes (float)z and r16 into the workspace, `valid` and `radius`; the three pixel
//      counts of a workgroup are summed in LDS and added to `count` with one integer atomicAdd each;
//   3. the gather: a workgroup owns a tile of 32 x 8 targets.  It takes the largest r16 of the usable pixels within max_radius of the
//      tile - no tap beyond that can contribute - stages the tile with a halo of that many pixels in LDS ((float)z, r16, the three
//      colour bytes: 9 bytes per pixel, 96 x 72 pixels at the most) and every lane walks its window from LDS, bounded per row by the
//      disc of that radius.  64-bit integer sums per lane; the contributions are counted like the pixels.
// Integer sums commute: every output byte is a function of the inputs alone.  No float atomics, no tickets, no workgroup waits on
// another.  The fp64 of r16 is built with -ffp-contract=off; everything after it is integer arithmetic.
#include "depth3d.h"   // the rules, shared with points.hip, mesh.hip and view.hip

namespace {

constexpr int FOCUS_THREADS = 256;
constexpr int TILE_W = 32, TILE_H = 8;   // a 32-lane half of a wave reads one row of the window: consecutive LDS addresses
constexpr int FOCUS_R = MG_FOCUS_MAX_RADIUS;
constexpr int FOCUS_E = 16 * FOCUS_R;    // the largest r16
constexpr int HALO_W = TILE_W + 2 * FOCUS_R, HALO_H = TILE_H + 2 * FOCUS_R, HALO_N = HALO_W * HALO_H;
constexpr unsigned short FOCUS_UNUSABLE = 0xFFFFu;
enum { COUNT_USABLE = 0, COUNT_SHARP, COUNT_CAPPED, COUNT_TAPS, COUNT_BAD_FOCUS, FOCUS_COUNTS };
static_assert(TILE_W * TILE_H == FOCUS_THREADS, "one lane per target of the tile");
static_assert(HALO_N * 9 + (FOCUS_E + 1) * 4 + 64 <= 65536, "the staged window and the weights fit a static LDS allocation");

// W[e] = floor(2^24 / N[e]), N[e] the integer offsets of the plane with 256 (dx^2 + dy^2) <= e^2: a compile-time table.  The offsets
// are counted by their squared length k = dx^2 + dy^2 <= 1024; N[e] is the number with k <= floor(e^2 / 256).
struct FocusWeights {
  unsigned w[FOCUS_E + 1];
};

constexpr FocusWeights focus_weights() {
  FocusWeights t = {};
  unsigned below[FOCUS_R * FOCUS_R + 1] = {};
  for (int dy = -FOCUS_R; dy <= FOCUS_R; ++dy)
    for (int dx = -FOCUS_R; dx <= FOCUS_R; ++dx)
      if (dx * dx + dy * dy <= FOCUS_R * FOCUS_R) ++below[dx * dx + dy * dy];
  for (int k = 1; k <= FOCUS_R * FOCUS_R; ++k) below[k] += below[k - 1];
  for (int e = 0; e <= FOCUS_E; ++e) t.w[e] = (1u << 24) / below[(e * e) / 256];
  return t;
}

constexpr FocusWeights FOCUS_W_HOST = focus_weights();
static_assert(FOCUS_W_HOST.w[0] == 1u << 24 && FOCUS_W_HOST.w[16] == (1u << 24) / 5 && FOCUS_W_HOST.w[FOCUS_E] == (1u << 24) / 3209, "N[0], N[16], N[512]");
__device__ const FocusWeights FOCUS_W = focus_weights();

struct FocusArgs {
  int space, max_radius, focus_x, focus_y;
  double gain, z_focus;
};

// grid (1): `count` to zeros
__global__ void focus_clear_kernel(long long* __restrict__ count) {
  if (threadIdx.x < FOCUS_COUNTS) count[threadIdx.x] = 0;
}

// grid (ceil(n / threads)): lane i owns pixel i
__global__ __launch_bounds__(FOCUS_THREADS) void focus_prepare_kernel(PointsArgs a, FocusArgs f, float* __restrict__ zs, unsigned short* __restrict__ rs,
                                                                      unsigned char* __restrict__ valid, unsigned short* __restrict__ radius,
                                                                      long long* __restrict__ count) {
  __shared__ unsigned tally[COUNT_CAPPED + 1];
  if (threadIdx.x <= COUNT_CAPPED) tally[threadIdx.x] = 0;
  __syncthreads();
  const long long n = (long long)a.h * a.w, i = (long long)blockIdx.x * FOCUS_THREADS + threadIdx.x;
  double s, t;
  load_coef(a, s, t);
  // the focus distance, the same in every lane
  double zf = f.z_focus;
  bool bad = false;
  if (f.focus_x >= 0) bad = !depth_at(a, s, t, f.focus_y, f.focus_x, zf);
  bad = bad || !isfinite(zf) || (f.space == 0 && zf <= 0.0);
  if (i == 0) count[COUNT_BAD_FOCUS] = bad ? 1 : 0;   // (no other lane touches this entry)
  if (i < n) {
    const int y = (int)(i / a.w), x = (int)(i - (long long)y * a.w);
    double z;
    const bool usable = depth_at(a, s, t, y, x, z);
    int r16 = 0;
    if (usable && !bad) {
      const double b = f.space == 0 ? f.gain * fabs(1.0 / z - 1.0 / zf) : f.gain * fabs(z - zf);
      r16 = !(b < (double)f.max_radius) ? 16 * f.max_radius : (int)llrint(16.0 * b);
    }
    zs[i] = usable ? (float)z : 0.0f;
    rs[i] = usable ? (unsigned short)r16 : FOCUS_UNUSABLE;
    valid[i] = usable ? 1 : 0;
    if (radius != nullptr) radius[i] = usable ? (unsigned short)r16 : FOCUS_UNUSABLE;
    if (usable) {
      atomicAdd(&tally[COUNT_USABLE], 1u);
      if (r16 == 0) atomicAdd(&tally[COUNT_SHARP], 1u);
      if (f.max_radius > 0 && r16 == 16 * f.max_radius) atomicAdd(&tally[COUNT_CAPPED], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x <= COUNT_CAPPED && tally[threadIdx.x] != 0)
    atomicAdd((unsigned long long*)&count[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// grid (tiles_x * tiles_y): workgroup b owns the targets of tile (b % tiles_x, b / tiles_x); lane l the target (l % 32, l / 32) of it
__global__ __launch_bounds__(FOCUS_THREADS) void focus_gather_kernel(const float* __restrict__ zs, const unsigned short* __restrict__ rs,
                                                                     const unsigned char* __restrict__ colors, int hwc, int h, int w, int max_radius,
                                                                     int tiles_x, unsigned char* __restrict__ rgb, long long* __restrict__ count) {
  __shared__ float sz[HALO_N];
  __shared__ unsigned weight[FOCUS_E + 1];
  __shared__ unsigned short sr[HALO_N];   // 0 for a pixel that is not usable or outside the picture: it passes no test but its own
  __shared__ unsigned char sc[3][HALO_N];
  __shared__ unsigned reach, taps;
  const int tid = (int)threadIdx.x;
  const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
  const int x0 = tile_x * TILE_W, y0 = tile_y * TILE_H;
  const long long n = (long long)h * w;
  if (tid == 0) {
    reach = 0;
    taps = 0;
  }
  for (int e = tid; e <= FOCUS_E; e += FOCUS_THREADS) weight[e] = FOCUS_W.w[e];
  __syncthreads();
  // the largest r16 of the usable pixels within max_radius of the tile, inside the picture
  {
    const int ya = max(y0 - max_radius, 0), yb = min(y0 + TILE_H + max_radius, h), xa = max(x0 - max_radius, 0), xb = min(x0 + TILE_W + max_radius, w);
    const int cols = xb - xa, cells = cols * (yb - ya);   // at most HALO_N
    unsigned m = 0;
    for (int k = tid; k < cells; k += FOCUS_THREADS) {
      const int ly = k / cols, lx = k - ly * cols;
      const unsigned r = rs[(long long)(ya + ly) * w + (xa + lx)];
      if (r != FOCUS_UNUSABLE) m = max(m, r);
    }
    if (m != 0) atomicMax(&reach, m);
  }
  __syncthreads();
  const int top = (int)reach;        // wave-uniform: no tap with 256 (dx^2 + dy^2) > top^2 contributes to a target of this tile
  const int R = top >> 4;            // so |dx|, |dy| <= R <= max_radius
  const int sw = TILE_W + 2 * R, sh = TILE_H + 2 * R;
  for (int k = tid; k < sw * sh; k += FOCUS_THREADS) {
    const int ly = k / sw, lx = k - ly * sw, y = y0 - R + ly, x = x0 - R + lx;
    unsigned short r = 0;
    float z = 0.0f;
    unsigned char c[3] = {0, 0, 0};
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const long long i = (long long)y * w + x;
      const unsigned short got = rs[i];
      if (got != FOCUS_UNUSABLE) {
        r = got;
        z = zs[i];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = hwc ? colors[i * 3 + ch] : colors[(long long)ch * n + i];
      }
    }
    sz[k] = z;
    sr[k] = r;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sc[ch][k] = c[ch];
  }
  __syncthreads();
  const int tx = tid % TILE_W, ty = tid / TILE_W, x = x0 + tx, y = y0 + ty;
  unsigned mine = 0;
  if (x < w && y < h) {
    const long long i = (long long)y * w + x;
    const unsigned short got = rs[i];
    unsigned char out[3];
    if (got == FOCUS_UNUSABLE) {   // keeps its source bytes
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = hwc ? colors[i * 3 + ch] : colors[(long long)ch * n + i];
    } else {
      const int at = (ty + R) * sw + (tx + R), rp = (int)got;
      const float zp = sz[at];
      unsigned long long D = 0, C[3] = {0, 0, 0};
      int reach_x = R;               // the widest |dx| of the disc of radius top / 16 in this row: it shrinks as |dy| grows
      for (int ady = 0; ady <= R; ++ady) {
        const int rest = top * top - 256 * ady * ady;   // >= 0: 16 ady <= 16 R <= top
        while (256 * reach_x * reach_x > rest) --reach_x;
        for (int side = 0; side < (ady == 0 ? 1 : 2); ++side) {
          const int dy = side == 0 ? ady : -ady, row = at + dy * sw;
          for (int dx = -reach_x; dx <= reach_x; ++dx) {
            const int rq = (int)sr[row + dx], far2 = 256 * (dx * dx + ady * ady);
            if (far2 > rq * rq) continue;             // e <= r16_q
            const int e = sz[row + dx] <= zp ? rq : min(rq, rp);
            if (far2 > e * e) continue;
            const unsigned wq = weight[e];
            D += wq;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) C[ch] += (unsigned long long)wq * sc[ch][row + dx];
            ++mine;
          }
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = (unsigned char)((C[ch] + D / 2) / D);   // D >= W[r16_p] > 0: p contributes to itself
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (hwc) rgb[i * 3 + ch] = out[ch];
      else rgb[(long long)ch * n + i] = out[ch];
    }
  }
  if (mine != 0) atomicAdd(&taps, mine);   // at most 256 * 4225
  __syncthreads();
  if (tid == 0 && taps != 0) atomicAdd((unsigned long long*)&count[COUNT_TAPS], (unsigned long long)taps);
}

long long z_bytes(long long n) { return (n * (long long)sizeof(float) + 15) / 16 * 16; }

}  // namespace

extern "C" long long mg_depth_focus_workspace_bytes(long long n) {
  if (n < 1 || n > DEPTH3D_MAX_N) {
    mg_set_error("mg_depth_focus_workspace_bytes: %lld pixels, 1 to 2^30 are supported", n);
    return -1;
  }
  // (float)z and r16 per pixel, each array rounded up to 16 bytes; the counts are summed in `count` itself
  return z_bytes(n) + (n * (long long)sizeof(unsigned short) + 15) / 16 * 16;
}

extern "C" int mg_depth_focus(const float* d, const unsigned char* colors, int hwc, const unsigned char* mask_or_null, const double* coef_or_null, int h,
                              int w, double z_min, double z_max, int space, double gain, int max_radius, int focus_x, int focus_y, double z_focus,
                              unsigned char* rgb, unsigned char* valid, unsigned short* radius_or_null, long long* count, void* ws,
                              long long ws_bytes, void* stream) {
  const char* fn = "mg_depth_focus";
  MG_REQUIRE(d && colors && rgb && valid && count && ws, "%s: null pointer", fn);
  if (const int rc = check_common(fn, h, w, 1.0, 1.0, 0.0, 0.0, z_min, z_max, 0.0, MG_NORMALS_FRAME_CAMERA)) return rc;   // (no camera here)
  MG_REQUIRE(space == MG_FOCUS_SPACE_LENS || space == MG_FOCUS_SPACE_LINEAR, "%s: unknown space %d", fn, space);
  MG_REQUIRE(std::isfinite(gain) && gain >= 0.0, "%s: gain %g is not finite and >= 0", fn, gain);
  MG_REQUIRE(max_radius >= 0 && max_radius <= MG_FOCUS_MAX_RADIUS, "%s: max_radius %d, 0 to %d are supported", fn, max_radius, MG_FOCUS_MAX_RADIUS);
  MG_REQUIRE((focus_x >= 0 && focus_y >= 0) || (focus_x == -1 && focus_y == -1),
             "%s: the focus pixel (%d, %d) is neither a pixel nor (-1, -1) for the distance z_focus", fn, focus_x, focus_y);
  MG_REQUIRE(focus_x < w && focus_y < h, "%s: the focus pixel (%d, %d) is outside the picture of %d x %d", fn, focus_x, focus_y, h, w);
  MG_REQUIRE((uintptr_t)d % 4 == 0 && (uintptr_t)radius_or_null % 2 == 0 && (uintptr_t)count % 8 == 0 && (uintptr_t)coef_or_null % 8 == 0,
             "%s: d, radius, count and coef must be aligned to their elements", fn);
  MG_REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
  const long long n = (long long)h * w, need = mg_depth_focus_workspace_bytes(n);
  MG_REQUIRE(ws_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (mg_depth_focus_workspace_bytes)", fn, ws_bytes, need);
  const PointsArgs a = {d, mask_or_null, coef_or_null, h, w, 1.0, 1.0, 0.0, 0.0, z_min, z_max, 0.0, MG_NORMALS_FRAME_CAMERA};
  const FocusArgs f = {space, max_radius, focus_x, focus_y, gain, z_focus};
  float* zs = (float*)ws;
  unsigned short* rs = (unsigned short*)((char*)ws + z_bytes(n));
  const hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (w + TILE_W - 1) / TILE_W, tiles_y = (h + TILE_H - 1) / TILE_H;   // tiles_x tiles_y < 2^28
  const dim3 block(FOCUS_THREADS), pixels((unsigned)((n + FOCUS_THREADS - 1) / FOCUS_THREADS)), tiles((unsigned)tiles_x * (unsigned)tiles_y);
  MG_LAUNCH(focus_clear_kernel, dim3(1), dim3(64), 0, st, count);
  MG_LAUNCH(focus_prepare_kernel, pixels, block, 0, st, a, f, zs, rs, valid, radius_or_null, count);
  MG_LAUNCH(focus_gather_kernel, tiles, block, 0, st, (const float*)zs, (const unsigned short*)rs, colors, hwc, h, w, max_radius, tiles_x, rgb, count);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
