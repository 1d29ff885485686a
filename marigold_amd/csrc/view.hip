// Depth to views: the faces of 6i seen from a second pinhole camera - mg_depth_view, a small software rasteriser.  The
// definitions (target camera, transform, dropped faces, coverage, depth and key, colour, fill, outputs) and the contract are in
// include/marigold_hip.h, block DEPTH TO VIEW; usable, joined, the point of a pixel and the cell rules are depth3d.h's.
// Three launches, none of which waits on another workgroup; only stream order separates them:
//   1. the key buffer (one 64-bit word per target pixel) is set to all ones and `count` to zeros;
//   2. the splat: one lane per cell decides its faces again, transforms their corners, drops a face that is near, off, back or over the
//      span cap, and offers every covered pixel centre its key - the fp32 depth's bits above the face id - with a 64-bit atomicMin;
//      the six face counts of a workgroup are summed in LDS and added to `count` with one integer atomicAdd each;
//   3. the resolve: one lane per target pixel reads its key, computes the winning face again from its id for the colour, or looks
//      along its row in the KEY buffer for the nearest covered pixels and takes the farther one; the two pixel counts are added likewise.
// Integer minima and integer sums commute: every output byte is a function of the inputs alone.  No float atomics, no tickets, no
// workgroup waits on another.  fp64 throughout, built with -ffp-contract=off; all coverage arithmetic is int64.
#include "depth3d.h"   // the rules, shared with points.hip and mesh.hip

namespace {

constexpr int VIEW_THREADS = 256;
constexpr unsigned long long VIEW_EMPTY = ~0ull;                 // no offer: above every key (a key's upper word is a finite fp32 > 0)
constexpr double VIEW_OFF = 1048576.0;                           // 2^20 pixels
enum { COUNT_FACES = 0, COUNT_DRAWN, COUNT_NEAR, COUNT_OFF, COUNT_BACK, COUNT_SPAN, COUNT_COVERED, COUNT_FILLED, VIEW_COUNTS };

struct ViewArgs {
  double pose[12];   // the rows of [R | t]
  double fx, fy, cx, cy, z_near;
  int h, w, fill;
};

enum { FACE_DRAWN = 0, FACE_NEAR, FACE_OFF, FACE_BACK, FACE_SPAN };

// a face in the target camera: the snapped corners, 1 / Z' of each, the doubled area and the box of pixel centres before clamping
struct Projected {
  long long xi[3], yi[3], area, x0, x1, y0, y1;
  double q[3];
};

// the doubled signed area of (a, b, c) in snapped coordinates, positive for every face of the identity view
__device__ __forceinline__ long long edge(long long ax, long long ay, long long bx, long long by, long long cx, long long cy) {
  return (cx - ax) * (by - ay) - (bx - ax) * (cy - ay);
}

// face `slot` of the cell anchored at (x, y), of `form` -> the first reason to drop it, or FACE_DRAWN with `f` filled
__device__ __forceinline__ int project(const PointsArgs& a, const ViewArgs& v, double s, double t, int x, int y, int form, int slot, Projected& f) {
  const unsigned tri = triangle_of(form, slot);
  double u[3], vv[3];
  bool near = false, off = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned c = (tri >> (2 * k)) & 3u;
    const int px = x + (int)(c & 1u), py = y + (int)(c >> 1);
    double z;
    depth_at(a, s, t, py, px, z);   // (usable: the corner of a face)
    const Vec3 P = point_of(a, px, py, z);
    const double X = ((v.pose[0] * P.x + v.pose[1] * P.y) + v.pose[2] * P.z) + v.pose[3];
    const double Y = ((v.pose[4] * P.x + v.pose[5] * P.y) + v.pose[6] * P.z) + v.pose[7];
    const double Z = ((v.pose[8] * P.x + v.pose[9] * P.y) + v.pose[10] * P.z) + v.pose[11];
    near = near || !isfinite(Z) || Z < v.z_near;
    u[k] = (v.fx * X) / Z + v.cx;
    vv[k] = (v.fy * Y) / Z + v.cy;
    f.q[k] = 1.0 / Z;
    off = off || !(fabs(u[k]) <= VIEW_OFF) || !(fabs(vv[k]) <= VIEW_OFF);   // (a NaN is off)
  }
  if (near) return FACE_NEAR;
  if (off) return FACE_OFF;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f.xi[k] = llrint(256.0 * u[k]);   // |.| <= 2^28; round half to even
    f.yi[k] = llrint(256.0 * vv[k]);
  }
  f.area = edge(f.xi[0], f.yi[0], f.xi[1], f.yi[1], f.xi[2], f.yi[2]);
  if (f.area <= 0) return FACE_BACK;
  const long long xlo = min(f.xi[0], min(f.xi[1], f.xi[2])), xhi = max(f.xi[0], max(f.xi[1], f.xi[2]));
  const long long ylo = min(f.yi[0], min(f.yi[1], f.yi[2])), yhi = max(f.yi[0], max(f.yi[1], f.yi[2]));
  f.x0 = (xlo + 255) >> 8;   // ceil and floor of a 24.8 coordinate
  f.x1 = xhi >> 8;
  f.y0 = (ylo + 255) >> 8;
  f.y1 = yhi >> 8;
  if (f.x1 - f.x0 + 1 > MG_VIEW_MAX_SPAN || f.y1 - f.y0 + 1 > MG_VIEW_MAX_SPAN) return FACE_SPAN;
  return FACE_DRAWN;
}

// the three edge values of pixel centre (px, py): e_k opposite corner k, e0 + e1 + e2 == area
__device__ __forceinline__ void edges_at(const Projected& f, long long px, long long py, long long e[3]) {
  const long long X = px * 256, Y = py * 256;
  e[0] = edge(X, Y, f.xi[1], f.yi[1], f.xi[2], f.yi[2]);
  e[1] = edge(f.xi[0], f.yi[0], X, Y, f.xi[2], f.yi[2]);
  e[2] = edge(f.xi[0], f.yi[0], f.xi[1], f.yi[1], X, Y);
}

// grid (ceil(n2 / threads)): the key buffer to "no offer"; block 0 clears the counts
__global__ __launch_bounds__(VIEW_THREADS) void view_clear_kernel(unsigned long long* __restrict__ keys, long long n2, long long* __restrict__ count) {
  const long long i = (long long)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (i < n2) keys[i] = VIEW_EMPTY;
  if (blockIdx.x == 0 && threadIdx.x < VIEW_COUNTS) count[threadIdx.x] = 0;
}

// grid (ceil(n / threads)): lane i owns the cell anchored at source pixel i
__global__ __launch_bounds__(VIEW_THREADS) void view_splat_kernel(PointsArgs a, ViewArgs v, unsigned long long* __restrict__ keys,
                                                                  long long* __restrict__ count) {
  __shared__ unsigned tally[COUNT_SPAN + 1];
  if (threadIdx.x <= COUNT_SPAN) tally[threadIdx.x] = 0;
  __syncthreads();
  const long long n = (long long)a.h * a.w, i = (long long)blockIdx.x * VIEW_THREADS + threadIdx.x;
  double s, t;
  load_coef(a, s, t);
  const unsigned code = i < n ? cell_code(a, s, t, i) : 0u;
  if (code & 3u) {
    const int y = (int)(i / a.w), x = (int)(i - (long long)y * a.w), form = (int)(code >> 2);
    for (int slot = 0; slot < 2; ++slot) {
      if (!((code >> slot) & 1u)) continue;
      atomicAdd(&tally[COUNT_FACES], 1u);
      Projected f;
      const int why = project(a, v, s, t, x, y, form, slot, f);
      atomicAdd(&tally[COUNT_DRAWN + why], 1u);   // (FACE_* follow COUNT_DRAWN in the order of `count`)
      if (why != FACE_DRAWN) continue;
      const unsigned long long id = 2ull * (unsigned long long)i + (unsigned)slot;   // < 2^31
      const long long x0 = max(f.x0, 0ll), x1 = min(f.x1, (long long)v.w - 1), y0 = max(f.y0, 0ll), y1 = min(f.y1, (long long)v.h - 1);
      for (long long py = y0; py <= y1; ++py) {       // at most MG_VIEW_MAX_SPAN^2 tests, all inside the target
        for (long long px = x0; px <= x1; ++px) {
          long long e[3];
          edges_at(f, px, py, e);
          if (e[0] < 0 || e[1] < 0 || e[2] < 0) continue;
          const double sum = ((double)e[0] * f.q[0] + (double)e[1] * f.q[1]) + (double)e[2] * f.q[2];
          const float zv = (float)((double)f.area / sum);
          if (!(isfinite(zv) && zv > 0.0f)) continue;
          atomicMin(&keys[py * v.w + px], (unsigned long long)__float_as_uint(zv) << 32 | id);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x <= COUNT_SPAN && tally[threadIdx.x] != 0)
    atomicAdd((unsigned long long*)&count[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// the colour of target pixel (px, py) under the face its key names -> three bytes
__device__ __forceinline__ void shade(const PointsArgs& a, const ViewArgs& v, double s, double t, const unsigned char* __restrict__ colors, int hwc,
                                      unsigned long long key, long long px, long long py, unsigned char out[3]) {
  const long long n = (long long)a.h * a.w, id = (long long)(key & 0xffffffffull), cell = id >> 1;
  const int slot = (int)(id & 1), y = (int)(cell / a.w), x = (int)(cell - (long long)y * a.w);
  const int form = (int)(cell_code(a, s, t, cell) >> 2);
  Projected f;
  project(a, v, s, t, x, y, form, slot, f);   // (drawn: it made an offer)
  long long e[3];
  edges_at(f, px, py, e);
  const double w0 = (double)e[0] * f.q[0], w1 = (double)e[1] * f.q[1], w2 = (double)e[2] * f.q[2], sum = (w0 + w1) + w2;
  const unsigned tri = triangle_of(form, slot);
  long long at[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned c = (tri >> (2 * k)) & 3u;
    at[k] = cell + (long long)(c & 1u) + (long long)(c >> 1) * a.w;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (double)(hwc ? colors[at[k] * 3 + ch] : colors[(long long)ch * n + at[k]]);
    const double mix = ((w0 * c[0] + w1 * c[1]) + w2 * c[2]) / sum;
    out[ch] = (unsigned char)min((int)(mix + 0.5), 255);
  }
}

// grid (ceil(n2 / threads)): lane i owns target pixel i
__global__ __launch_bounds__(VIEW_THREADS) void view_resolve_kernel(PointsArgs a, ViewArgs v, const unsigned char* __restrict__ colors, int hwc,
                                                                    const unsigned long long* __restrict__ keys, unsigned char* __restrict__ rgb,
                                                                    float* __restrict__ depth, unsigned char* __restrict__ valid,
                                                                    int* __restrict__ face, long long* __restrict__ count) {
  __shared__ unsigned tally[2];
  if (threadIdx.x < 2) tally[threadIdx.x] = 0;
  __syncthreads();
  const long long n2 = (long long)v.h * v.w, i = (long long)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (i < n2) {
    double s, t;
    load_coef(a, s, t);
    const long long py = i / v.w, px = i - py * v.w;
    unsigned long long key = keys[i];
    long long from = px;
    unsigned char state = 1;
    if (key != VIEW_EMPTY) {
      if (face != nullptr) face[i] = (int)(key & 0xffffffffull);
    } else {
      if (face != nullptr) face[i] = -1;
      state = 0;
      unsigned long long left = VIEW_EMPTY, right = VIEW_EMPTY;
      long long lx = 0, rx = 0;
      for (int k = 1; k <= v.fill && left == VIEW_EMPTY && px - k >= 0; ++k) {
        left = keys[i - k];
        lx = px - k;
      }
      for (int k = 1; k <= v.fill && right == VIEW_EMPTY && px + k < v.w; ++k) {
        right = keys[i + k];
        rx = px + k;
      }
      // the farther of the two; a key's upper word orders like its depth; on equal depth, or alone, the left
      if (right != VIEW_EMPTY && (left == VIEW_EMPTY || (right >> 32) > (left >> 32))) {
        key = right;
        from = rx;
      } else if (left != VIEW_EMPTY) {
        key = left;
        from = lx;
      }
      if (key != VIEW_EMPTY) state = 2;
    }
    unsigned char out[3] = {0, 0, 0};
    float z = 0.0f;
    if (state != 0) {
      shade(a, v, s, t, colors, hwc, key, from, py, out);
      z = __uint_as_float((unsigned)(key >> 32));
      atomicAdd(&tally[state - 1], 1u);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (hwc) rgb[i * 3 + ch] = out[ch];
      else rgb[(long long)ch * n2 + i] = out[ch];
    }
    depth[i] = z;
    valid[i] = state;
  }
  __syncthreads();
  if (threadIdx.x < 2 && tally[threadIdx.x] != 0)
    atomicAdd((unsigned long long*)&count[COUNT_COVERED + threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

}  // namespace

extern "C" long long mg_depth_view_workspace_bytes(long long n2) {
  if (n2 < 1 || n2 > DEPTH3D_MAX_N) {
    mg_set_error("mg_depth_view_workspace_bytes: %lld target pixels, 1 to 2^30 are supported", n2);
    return -1;
  }
  // a key per target pixel; the counts are summed in `count` itself
  return (n2 * (long long)sizeof(unsigned long long) + 15) / 16 * 16;
}

extern "C" int mg_depth_view(const float* d, const unsigned char* colors, int hwc, const unsigned char* mask_or_null, const double* coef_or_null, int h,
                             int w, double fx, double fy, double cx, double cy, double z_min, double z_max, double edge_rel,
                             const double* pose_or_null, double fx2, double fy2, double cx2, double cy2, int h2, int w2, double z_near,
                             int fill_radius, unsigned char* rgb, float* depth, unsigned char* valid, int* face_or_null, long long* count, void* ws,
                             long long ws_bytes, void* stream) {
  const char* fn = "mg_depth_view";
  MG_REQUIRE(d && colors && rgb && depth && valid && count && ws, "%s: null pointer", fn);
  if (const int rc = check_common(fn, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, MG_NORMALS_FRAME_CAMERA)) return rc;
  MG_REQUIRE(h2 >= 1 && w2 >= 1 && (long long)h2 * w2 <= DEPTH3D_MAX_N, "%s: a target of %d x %d, 1 to 2^30 pixels are supported", fn, h2, w2);
  MG_REQUIRE(std::isfinite(fx2) && fx2 > 0.0 && std::isfinite(fy2) && fy2 > 0.0, "%s: the target's focal lengths (%g, %g) are not finite and > 0", fn,
             fx2, fy2);
  MG_REQUIRE(std::isfinite(cx2) && std::isfinite(cy2), "%s: the target's principal point (%g, %g) is not finite", fn, cx2, cy2);
  ViewArgs v = {{1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0}, fx2, fy2, cx2, cy2, z_near, h2, w2, fill_radius};
  if (pose_or_null != nullptr) {
    for (int k = 0; k < 12; ++k) {
      MG_REQUIRE(std::isfinite(pose_or_null[k]), "%s: pose entry %d (%g) is not finite", fn, k, pose_or_null[k]);
      v.pose[k] = pose_or_null[k];
    }
  }
  MG_REQUIRE(std::isfinite(z_near) && z_near > 0.0, "%s: z_near %g is not finite and > 0", fn, z_near);
  MG_REQUIRE(fill_radius >= 0 && fill_radius <= MG_VIEW_MAX_FILL, "%s: fill_radius %d, 0 to %d are supported", fn, fill_radius, MG_VIEW_MAX_FILL);
  MG_REQUIRE((uintptr_t)d % 4 == 0 && (uintptr_t)depth % 4 == 0 && (uintptr_t)face_or_null % 4 == 0 && (uintptr_t)count % 8 == 0 &&
                 (uintptr_t)coef_or_null % 8 == 0,
             "%s: d, depth, face, count and coef must be aligned to their elements", fn);
  MG_REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
  const long long n = (long long)h * w, n2 = (long long)h2 * w2, need = mg_depth_view_workspace_bytes(n2);
  MG_REQUIRE(ws_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (mg_depth_view_workspace_bytes)", fn, ws_bytes, need);
  const PointsArgs a = {d, mask_or_null, coef_or_null, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, MG_NORMALS_FRAME_CAMERA};
  unsigned long long* keys = (unsigned long long*)ws;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(VIEW_THREADS), source((unsigned)((n + VIEW_THREADS - 1) / VIEW_THREADS)), target((unsigned)((n2 + VIEW_THREADS - 1) / VIEW_THREADS));
  MG_LAUNCH(view_clear_kernel, target, block, 0, st, keys, n2, count);
  MG_LAUNCH(view_splat_kernel, source, block, 0, st, a, v, keys, count);
  MG_LAUNCH(view_resolve_kernel, target, block, 0, st, a, v, colors, hwc, (const unsigned long long*)keys, rgb, depth, valid, face_or_null, count);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
