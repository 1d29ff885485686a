// Depth to 3D: camera-space points and surface normals from a depth map - mg_depth_normals, the dense normals map in one
// launch, and mg_depth_points, the kept pixels compacted in row-major order without the host learning how many there are.  The
// definitions (usable, joined, kept, point, normal) and the contract of every entry point are in include/marigold_hip.h.
// The cloud is three launches, none of which waits on another workgroup: the kept pixels of every fixed chunk are counted; one
// workgroup adds the counts in chunk order into the chunks' offsets and `count`; the scatter decides again what is kept and ranks a
// pixel inside its chunk with 64-lane ballots and population counts.  No atomics, no tickets: the record a pixel goes to is a
// function of the inputs alone.  Bound by memory where it is bound by anything (two passes over d and the mask, one over the colours of
// kept pixels); the five depths a pixel looks at come from the caches.  fp64 throughout, built with -ffp-contract=off: every product,
// sum and quotient below is rounded on its own, in the order the header writes them, so a numpy float64 restatement gives the same
// values.
#include "depth3d.h"   // the rules, shared with mesh.hip

namespace {

constexpr int POINTS_THREADS = 256;
constexpr int POINTS_CHUNK = 2048;                             // pixels per workgroup of the count and the scatter
constexpr int POINTS_PER_THREAD = POINTS_CHUNK / POINTS_THREADS;
constexpr int POINTS_WAVES = POINTS_THREADS / 64;
constexpr int POINTS_SCAN_LANES = 256;                         // lanes of the one workgroup that turns counts into offsets
constexpr long long POINTS_MAX_N = DEPTH3D_MAX_N;

// grid (ceil(n / 256)): one pixel per lane
__global__ __launch_bounds__(POINTS_THREADS) void depth_normals_kernel(PointsArgs a, float* __restrict__ out, unsigned char* __restrict__ valid) {
  const long long n = (long long)a.h * a.w, i = (long long)blockIdx.x * POINTS_THREADS + threadIdx.x;
  if (i >= n) return;
  double s, t;
  load_coef(a, s, t);
  const Pixel p = classify(a, s, t, i);
  Vec3 N = {0.0, 0.0, 0.0};
  bool has = false;
  if (p.kept) {
    has = normal_of(a, p, point_of(a, p.x, p.y, p.z), N);
    if (!has) N = {0.0, 0.0, 0.0};
  }
  out[i] = (float)N.x;
  out[n + i] = (float)N.y;
  out[2 * n + i] = (float)N.z;
  valid[i] = has ? 1 : 0;
}

// grid (chunks): block c counts the kept pixels of [c POINTS_CHUNK, (c + 1) POINTS_CHUNK) -> counts[c]
__global__ __launch_bounds__(POINTS_THREADS) void points_count_kernel(PointsArgs a, long long* __restrict__ counts) {
  const long long n = (long long)a.h * a.w, base = (long long)blockIdx.x * POINTS_CHUNK + threadIdx.x;
  double s, t;
  load_coef(a, s, t);
  int mine = 0;   // (the same in every lane of a wave)
#pragma unroll
  for (int j = 0; j < POINTS_PER_THREAD; ++j) {
    const long long i = base + (long long)j * POINTS_THREADS;
    const bool kept = i < n && classify(a, s, t, i).kept;
    mine += __popcll(__ballot(kept));
  }
  __shared__ int lds[POINTS_WAVES];
  if (threadIdx.x % 64 == 0) lds[threadIdx.x / 64] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long v = 0;
    for (int k = 0; k < POINTS_WAVES; ++k) v += lds[k];
    counts[blockIdx.x] = v;
  }
}

// one workgroup: lane l owns the chunks [l per, (l + 1) per), adds their counts, learns what the lanes before it hold, and writes its
// chunks' offsets; the last lane ends with the total.  Integers: the order changes nothing, and it is fixed anyway.
__global__ __launch_bounds__(POINTS_SCAN_LANES) void points_scan_kernel(const long long* __restrict__ counts, long long chunks, long long capacity,
                                                                        long long* __restrict__ offsets, long long* __restrict__ count) {
  __shared__ long long sums[POINTS_SCAN_LANES];
  const long long per = (chunks + POINTS_SCAN_LANES - 1) / POINTS_SCAN_LANES;
  const long long lo = min((long long)threadIdx.x * per, chunks), hi = min(lo + per, chunks);
  long long v = 0;
  for (long long c = lo; c < hi; ++c) v += counts[c];
  sums[threadIdx.x] = v;
  __syncthreads();
  long long before = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) before += sums[k];
  for (long long c = lo; c < hi; ++c) {
    offsets[c] = before;
    before += counts[c];
  }
  if (threadIdx.x == POINTS_SCAN_LANES - 1) {
    count[0] = before;
    count[1] = before < capacity ? before : capacity;
  }
}

// grid (chunks): block c decides again which of its pixels are kept; a kept pixel's record is offsets[c] + the kept pixels before it
// in the chunk: those of the passes before its own, of the waves before its own in this pass, of the lanes before it in its wave.
__global__ __launch_bounds__(POINTS_THREADS) void points_scatter_kernel(PointsArgs a, const unsigned char* __restrict__ colors, int hwc,
                                                                        const long long* __restrict__ offsets, long long capacity,
                                                                        float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                                        float* __restrict__ nrm, int* __restrict__ index) {
  const long long n = (long long)a.h * a.w, base = (long long)blockIdx.x * POINTS_CHUNK + threadIdx.x;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  double s, t;
  load_coef(a, s, t);
  __shared__ int lds[POINTS_PER_THREAD][POINTS_WAVES];
  unsigned keep = 0;                    // bit j: the pixel of pass j is kept
  int below[POINTS_PER_THREAD];         // kept pixels of the lanes before this one, in pass j
#pragma unroll
  for (int j = 0; j < POINTS_PER_THREAD; ++j) {
    const long long i = base + (long long)j * POINTS_THREADS;
    const bool kept = i < n && classify(a, s, t, i).kept;
    const unsigned long long votes = __ballot(kept);
    below[j] = __popcll(votes & ((1ull << lane) - 1ull));
    keep |= (kept ? 1u : 0u) << j;
    if (lane == 0) lds[j][wave] = __popcll(votes);
  }
  __syncthreads();
  long long r = offsets[blockIdx.x];
#pragma unroll
  for (int j = 0; j < POINTS_PER_THREAD; ++j) {
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < POINTS_WAVES; ++k) {
      const int c = lds[j][k];
      before += k < wave ? c : 0;
      all += c;
    }
    const long long rec = r + before + below[j];
    r += all;
    if (!((keep >> j) & 1u) || rec >= capacity) continue;
    const long long i = base + (long long)j * POINTS_THREADS;
    const Pixel p = classify(a, s, t, i);
    const Vec3 P = point_of(a, p.x, p.y, p.z);
    xyz[rec * 3 + 0] = (float)P.x;
    xyz[rec * 3 + 1] = (float)P.y;
    xyz[rec * 3 + 2] = (float)P.z;
    if (rgb != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[rec * 3 + c] = hwc ? colors[i * 3 + c] : colors[(long long)c * n + i];
    }
    if (nrm != nullptr) {
      Vec3 N;
      if (!normal_of(a, p, P, N)) N = {0.0, 0.0, 0.0};
      nrm[rec * 3 + 0] = (float)N.x;
      nrm[rec * 3 + 1] = (float)N.y;
      nrm[rec * 3 + 2] = (float)N.z;
    }
    if (index != nullptr) index[rec] = (int)i;
  }
}

long long chunks_of(long long n) { return (n + POINTS_CHUNK - 1) / POINTS_CHUNK; }

}  // namespace

extern "C" int mg_depth_normals(const float* d, const unsigned char* mask_or_null, const double* coef_or_null, int h, int w, double fx, double fy,
                                double cx, double cy, double z_min, double z_max, double edge_rel, int normals_frame, float* out,
                                unsigned char* valid, void* stream) {
  const char* fn = "mg_depth_normals";
  MG_REQUIRE(d && out && valid, "%s: null pointer", fn);
  if (const int rc = check_common(fn, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, normals_frame)) return rc;
  MG_REQUIRE((uintptr_t)d % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)coef_or_null % 8 == 0, "%s: d, out and coef must be aligned to their elements",
             fn);
  const PointsArgs a = {d, mask_or_null, coef_or_null, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, normals_frame};
  const long long n = (long long)h * w;
  MG_LAUNCH(depth_normals_kernel, dim3((unsigned)((n + POINTS_THREADS - 1) / POINTS_THREADS)), dim3(POINTS_THREADS), 0, (hipStream_t)stream, a, out,
            valid);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" long long mg_depth_points_workspace_bytes(long long n) {
  if (n < 1 || n > POINTS_MAX_N) {
    mg_set_error("mg_depth_points_workspace_bytes: %lld pixels, 1 to 2^30 are supported", n);
    return -1;
  }
  return chunks_of(n) * 2 * (long long)sizeof(long long);   // the chunks' counts, then their offsets
}

extern "C" int mg_depth_points(const float* d, const unsigned char* colors_or_null, int hwc, const unsigned char* mask_or_null,
                               const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy, double z_min, double z_max,
                               double edge_rel, int normals_frame, long long capacity, float* xyz, unsigned char* rgb_or_null, float* nrm_or_null,
                               int* index_or_null, long long* count, void* ws, long long ws_bytes, void* stream) {
  const char* fn = "mg_depth_points";
  MG_REQUIRE(d && xyz && count && ws, "%s: null pointer", fn);
  MG_REQUIRE((colors_or_null != nullptr) == (rgb_or_null != nullptr), "%s: colors and rgb go together, one of them is null", fn);
  if (const int rc = check_common(fn, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, normals_frame)) return rc;
  MG_REQUIRE(capacity >= 1, "%s: a capacity of %lld records, 1 at least is needed", fn, capacity);
  MG_REQUIRE((uintptr_t)d % 4 == 0 && (uintptr_t)xyz % 4 == 0 && (uintptr_t)nrm_or_null % 4 == 0 && (uintptr_t)index_or_null % 4 == 0 &&
                 (uintptr_t)count % 8 == 0 && (uintptr_t)coef_or_null % 8 == 0,
             "%s: d, xyz, nrm, index, count and coef must be aligned to their elements", fn);
  MG_REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
  const long long n = (long long)h * w, need = mg_depth_points_workspace_bytes(n);
  MG_REQUIRE(ws_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (mg_depth_points_workspace_bytes)", fn, ws_bytes, need);
  const PointsArgs a = {d, mask_or_null, coef_or_null, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, normals_frame};
  const long long chunks = chunks_of(n);   // (<= 2^19: a grid's x extent)
  long long* counts = (long long*)ws;
  long long* offsets = counts + chunks;
  const hipStream_t st = (hipStream_t)stream;
  MG_LAUNCH(points_count_kernel, dim3((unsigned)chunks), dim3(POINTS_THREADS), 0, st, a, counts);
  MG_LAUNCH(points_scan_kernel, dim3(1), dim3(POINTS_SCAN_LANES), 0, st, (const long long*)counts, chunks, capacity, offsets, count);
  MG_LAUNCH(points_scatter_kernel, dim3((unsigned)chunks), dim3(POINTS_THREADS), 0, st, a, colors_or_null, hwc, (const long long*)offsets, capacity,
            xyz, rgb_or_null, nrm_or_null, index_or_null);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
