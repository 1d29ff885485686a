// Depth to mesh: a depth map as vertices and triangles that stop at depth edges - mg_depth_mesh, both streams compacted
// consistently without the host learning a count.  The definitions (cell, candidate, face, vertex, count) and the contract are in
// include/marigold_hip.h; the rules shared with the point clouds (usable, joined, point, normal) and the cell rules
// (a cell's code, its form, the corners of its candidates) are depth3d.h's.
// Five launches, none of which waits on another workgroup; only stream order separates them:
//   1. every anchor pixel decides its cell's code - the form (split, or which corner is missing) and which of T0 / T1 are faces - into
//      a byte map, and the faces of every chunk of anchors are counted;
//   2. a pixel is a vertex when one of the up to four cells around it holds a face that uses it, read from the codes; the vertices of
//      every chunk are counted;
//   3. one workgroup adds both tables in chunk order into the chunks' offsets and writes `count`;
//   4. the vertex scatter ranks a vertex inside its chunk by passes, waves and lanes (ballots and population counts), writes its
//      record, and its rank into an int32 map;
//   5. the face scatter ranks the faces likewise and reads the three indices from that map.
// No atomics, no tickets: where a record goes is a function of the inputs alone.  fp64 throughout, built with -ffp-contract=off.
#include "depth3d.h"   // the rules, shared with points.hip and view.hip

namespace {

constexpr int MESH_THREADS = 256;
constexpr int MESH_CHUNK = 2048;                               // pixels (anchors of cells) per workgroup of the counts and the scatters
constexpr int MESH_PER_THREAD = MESH_CHUNK / MESH_THREADS;
constexpr int MESH_WAVES = MESH_THREADS / 64;
constexpr int MESH_SCAN_LANES = 256;                           // lanes of the one workgroup that turns counts into offsets

// bit c: corner c of the cell belongs to one of its faces
__device__ __forceinline__ unsigned corners_in_faces(unsigned code) {
  unsigned used = 0;
  const int form = (int)(code >> 2);
#pragma unroll
  for (int slot = 0; slot < 2; ++slot) {
    if (!((code >> slot) & 1u)) continue;
    const unsigned tri = triangle_of(form, slot);
    used |= 1u << (tri & 3u) | 1u << ((tri >> 2) & 3u) | 1u << ((tri >> 4) & 3u);
  }
  return used;
}

// whether pixel (x, y) is a corner of a face: it is D of the cell up and to the left, C of the one above, B of the one to the left and A
// of its own
__device__ __forceinline__ bool is_vertex(const unsigned char* __restrict__ codes, int h, int w, long long i) {
  const int y = (int)(i / w), x = (int)(i - (long long)y * w);
  bool v = false;
  if (x < w - 1 && y < h - 1) v = v || ((corners_in_faces(codes[i]) >> CORNER_A) & 1u);
  if (x > 0 && y < h - 1) v = v || ((corners_in_faces(codes[i - 1]) >> CORNER_B) & 1u);
  if (x < w - 1 && y > 0) v = v || ((corners_in_faces(codes[i - w]) >> CORNER_C) & 1u);
  if (x > 0 && y > 0) v = v || ((corners_in_faces(codes[i - w - 1]) >> CORNER_D) & 1u);
  return v;
}

// lane 0 of every wave holds `mine`, the wave's part of the chunk's count -> counts[block]
__device__ __forceinline__ void store_chunk_count(int mine, long long* __restrict__ counts) {
  __shared__ int lds[MESH_WAVES];
  if (threadIdx.x % 64 == 0) lds[threadIdx.x / 64] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long v = 0;
    for (int k = 0; k < MESH_WAVES; ++k) v += lds[k];
    counts[blockIdx.x] = v;
  }
}

// grid (chunks): block c writes the codes of the cells anchored in [c MESH_CHUNK, (c + 1) MESH_CHUNK) and counts their faces
__global__ __launch_bounds__(MESH_THREADS) void mesh_cells_kernel(PointsArgs a, unsigned char* __restrict__ codes, long long* __restrict__ counts) {
  const long long n = (long long)a.h * a.w, base = (long long)blockIdx.x * MESH_CHUNK + threadIdx.x;
  double s, t;
  load_coef(a, s, t);
  int mine = 0;   // (the same in every lane of a wave)
#pragma unroll
  for (int j = 0; j < MESH_PER_THREAD; ++j) {
    const long long i = base + (long long)j * MESH_THREADS;
    const unsigned code = i < n ? cell_code(a, s, t, i) : 0u;
    if (i < n) codes[i] = (unsigned char)code;
    mine += __popcll(__ballot(code & 1u)) + __popcll(__ballot(code & 2u));
  }
  store_chunk_count(mine, counts);
}

// grid (chunks): block c counts the vertices among its pixels
__global__ __launch_bounds__(MESH_THREADS) void mesh_vertex_count_kernel(const unsigned char* __restrict__ codes, int h, int w,
                                                                         long long* __restrict__ counts) {
  const long long n = (long long)h * w, base = (long long)blockIdx.x * MESH_CHUNK + threadIdx.x;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < MESH_PER_THREAD; ++j) {
    const long long i = base + (long long)j * MESH_THREADS;
    mine += __popcll(__ballot(i < n && is_vertex(codes, h, w, i)));
  }
  store_chunk_count(mine, counts);
}

// one table of the scan: lane l owns the chunks [lo, hi), adds their counts, learns what the lanes before it hold, and writes its
// chunks' offsets -> what stands before chunk hi (the total, in the last lane).  Integers: the order changes nothing, and it is fixed.
__device__ __forceinline__ long long scan_table(const long long* __restrict__ counts, long long lo, long long hi, long long* __restrict__ offsets,
                                                long long* sums) {
  long long v = 0;
  for (long long c = lo; c < hi; ++c) v += counts[c];
  __syncthreads();   // (the table before this one has been read out of `sums`)
  sums[threadIdx.x] = v;
  __syncthreads();
  long long before = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) before += sums[k];
  for (long long c = lo; c < hi; ++c) {
    offsets[c] = before;
    before += counts[c];
  }
  return before;
}

// one workgroup: both tables in chunk order; the last lane ends with the totals and writes `count`
__global__ __launch_bounds__(MESH_SCAN_LANES) void mesh_scan_kernel(const long long* __restrict__ face_counts, const long long* __restrict__ vertex_counts,
                                                                    long long chunks, long long capacity_v, long long capacity_f,
                                                                    long long* __restrict__ face_offsets, long long* __restrict__ vertex_offsets,
                                                                    long long* __restrict__ count) {
  __shared__ long long sums[MESH_SCAN_LANES];
  const long long per = (chunks + MESH_SCAN_LANES - 1) / MESH_SCAN_LANES;
  const long long lo = min((long long)threadIdx.x * per, chunks), hi = min(lo + per, chunks);
  const long long faces = scan_table(face_counts, lo, hi, face_offsets, sums);
  const long long vertices = scan_table(vertex_counts, lo, hi, vertex_offsets, sums);
  if (threadIdx.x == MESH_SCAN_LANES - 1) {
    count[0] = vertices;
    count[1] = vertices < capacity_v ? vertices : capacity_v;
    count[2] = faces;
    count[3] = vertices > capacity_v ? 0 : faces < capacity_f ? faces : capacity_f;   // cut vertices: no face could be trusted
  }
}

// grid (chunks): block c decides again which of its pixels are vertices; a vertex's rank is offsets[c] + the vertices before it in the
// chunk: those of the passes before its own, of the waves before its own in this pass, of the lanes before it in its wave.  The rank
// goes to ranks[pixel] whatever the capacity; the record only below it.
__global__ __launch_bounds__(MESH_THREADS) void mesh_vertex_scatter_kernel(PointsArgs a, const unsigned char* __restrict__ codes,
                                                                           const unsigned char* __restrict__ colors, int hwc,
                                                                           const long long* __restrict__ offsets, long long capacity,
                                                                           float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                                           float* __restrict__ nrm, int* __restrict__ index, int* __restrict__ ranks) {
  const long long n = (long long)a.h * a.w, base = (long long)blockIdx.x * MESH_CHUNK + threadIdx.x;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  double s, t;
  load_coef(a, s, t);
  __shared__ int lds[MESH_PER_THREAD][MESH_WAVES];
  unsigned keep = 0;                  // bit j: the pixel of pass j is a vertex
  int below[MESH_PER_THREAD];         // vertices of the lanes before this one, in pass j
#pragma unroll
  for (int j = 0; j < MESH_PER_THREAD; ++j) {
    const long long i = base + (long long)j * MESH_THREADS;
    const bool vertex = i < n && is_vertex(codes, a.h, a.w, i);
    const unsigned long long votes = __ballot(vertex);
    below[j] = __popcll(votes & ((1ull << lane) - 1ull));
    keep |= (vertex ? 1u : 0u) << j;
    if (lane == 0) lds[j][wave] = __popcll(votes);
  }
  __syncthreads();
  long long r = offsets[blockIdx.x];
#pragma unroll
  for (int j = 0; j < MESH_PER_THREAD; ++j) {
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < MESH_WAVES; ++k) {
      const int c = lds[j][k];
      before += k < wave ? c : 0;
      all += c;
    }
    const long long rec = r + before + below[j];
    r += all;
    if (!((keep >> j) & 1u)) continue;
    const long long i = base + (long long)j * MESH_THREADS;
    ranks[i] = (int)rec;   // (< n <= 2^30)
    if (rec >= capacity) continue;
    const Pixel p = classify(a, s, t, i);   // (usable: a face names it)
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

// grid (chunks): block c ranks the faces of its cells the same way - a cell holds up to two, T0 before T1 - and writes those below
// count[3], the faces that may be written, with the corners' ranks
__global__ __launch_bounds__(MESH_THREADS) void mesh_face_scatter_kernel(const unsigned char* __restrict__ codes, int h, int w,
                                                                         const long long* __restrict__ offsets, const long long* __restrict__ count,
                                                                         const int* __restrict__ ranks, int* __restrict__ faces) {
  const long long n = (long long)h * w, base = (long long)blockIdx.x * MESH_CHUNK + threadIdx.x;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  __shared__ int lds[MESH_PER_THREAD][MESH_WAVES];
  unsigned mine[MESH_PER_THREAD];     // the code of the cell of pass j
  int below[MESH_PER_THREAD];         // faces of the lanes before this one, in pass j
#pragma unroll
  for (int j = 0; j < MESH_PER_THREAD; ++j) {
    const long long i = base + (long long)j * MESH_THREADS;
    mine[j] = i < n ? codes[i] : 0u;
    const unsigned long long t0 = __ballot(mine[j] & 1u), t1 = __ballot(mine[j] & 2u), lower = (1ull << lane) - 1ull;
    below[j] = __popcll(t0 & lower) + __popcll(t1 & lower);
    if (lane == 0) lds[j][wave] = __popcll(t0) + __popcll(t1);
  }
  __syncthreads();
  const long long limit = count[3];
  long long r = offsets[blockIdx.x];
#pragma unroll
  for (int j = 0; j < MESH_PER_THREAD; ++j) {
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < MESH_WAVES; ++k) {
      const int c = lds[j][k];
      before += k < wave ? c : 0;
      all += c;
    }
    long long rec = r + before + below[j];
    r += all;
    if (!(mine[j] & 3u)) continue;
    const long long i = base + (long long)j * MESH_THREADS;   // a cell's anchor: i + w + 1 < n
    const long long corner[4] = {i, i + 1, i + w, i + w + 1};
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
      if (!((mine[j] >> slot) & 1u)) continue;
      if (rec < limit) {
        const unsigned tri = triangle_of((int)(mine[j] >> 2), slot);
        faces[rec * 3 + 0] = ranks[corner[tri & 3u]];
        faces[rec * 3 + 1] = ranks[corner[(tri >> 2) & 3u]];
        faces[rec * 3 + 2] = ranks[corner[(tri >> 4) & 3u]];
      }
      ++rec;
    }
  }
}

long long chunks_of(long long n) { return (n + MESH_CHUNK - 1) / MESH_CHUNK; }

}  // namespace

extern "C" long long mg_depth_mesh_workspace_bytes(long long n) {
  if (n < 1 || n > DEPTH3D_MAX_N) {
    mg_set_error("mg_depth_mesh_workspace_bytes: %lld pixels, 1 to 2^30 are supported", n);
    return -1;
  }
  // the chunks' face counts, vertex counts, face offsets and vertex offsets; the ranks; the codes
  const long long bytes = chunks_of(n) * 4 * (long long)sizeof(long long) + n * (long long)sizeof(int) + n;
  return (bytes + 15) / 16 * 16;
}

extern "C" int mg_depth_mesh(const float* d, const unsigned char* colors_or_null, int hwc, const unsigned char* mask_or_null,
                             const double* coef_or_null, int h, int w, double fx, double fy, double cx, double cy, double z_min, double z_max,
                             double edge_rel, int normals_frame, long long capacity_v, long long capacity_f, float* xyz,
                             unsigned char* rgb_or_null, float* nrm_or_null, int* index_or_null, int* faces, long long* count, void* ws,
                             long long ws_bytes, void* stream) {
  const char* fn = "mg_depth_mesh";
  MG_REQUIRE(d && xyz && faces && count && ws, "%s: null pointer", fn);
  MG_REQUIRE((colors_or_null != nullptr) == (rgb_or_null != nullptr), "%s: colors and rgb go together, one of them is null", fn);
  if (const int rc = check_common(fn, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, normals_frame)) return rc;
  MG_REQUIRE(capacity_v >= 1 && capacity_f >= 1, "%s: capacities of %lld vertices and %lld faces, 1 at least is needed of each", fn, capacity_v,
             capacity_f);
  MG_REQUIRE((uintptr_t)d % 4 == 0 && (uintptr_t)xyz % 4 == 0 && (uintptr_t)nrm_or_null % 4 == 0 && (uintptr_t)index_or_null % 4 == 0 &&
                 (uintptr_t)faces % 4 == 0 && (uintptr_t)count % 8 == 0 && (uintptr_t)coef_or_null % 8 == 0,
             "%s: d, xyz, nrm, index, faces, count and coef must be aligned to their elements", fn);
  MG_REQUIRE((uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
  const long long n = (long long)h * w, need = mg_depth_mesh_workspace_bytes(n);
  MG_REQUIRE(ws_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed (mg_depth_mesh_workspace_bytes)", fn, ws_bytes, need);
  const PointsArgs a = {d, mask_or_null, coef_or_null, h, w, fx, fy, cx, cy, z_min, z_max, edge_rel, normals_frame};
  const long long chunks = chunks_of(n);   // (<= 2^19: a grid's x extent)
  long long* face_counts = (long long*)ws;
  long long* vertex_counts = face_counts + chunks;
  long long* face_offsets = vertex_counts + chunks;
  long long* vertex_offsets = face_offsets + chunks;
  int* ranks = (int*)(vertex_offsets + chunks);
  unsigned char* codes = (unsigned char*)(ranks + n);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)chunks), block(MESH_THREADS);
  MG_LAUNCH(mesh_cells_kernel, grid, block, 0, st, a, codes, face_counts);
  MG_LAUNCH(mesh_vertex_count_kernel, grid, block, 0, st, (const unsigned char*)codes, h, w, vertex_counts);
  MG_LAUNCH(mesh_scan_kernel, dim3(1), dim3(MESH_SCAN_LANES), 0, st, (const long long*)face_counts, (const long long*)vertex_counts, chunks,
            capacity_v, capacity_f, face_offsets, vertex_offsets, count);
  MG_LAUNCH(mesh_vertex_scatter_kernel, grid, block, 0, st, a, (const unsigned char*)codes, colors_or_null, hwc, (const long long*)vertex_offsets,
            capacity_v, xyz, rgb_or_null, nrm_or_null, index_or_null, ranks);
  MG_LAUNCH(mesh_face_scatter_kernel, grid, block, 0, st, (const unsigned char*)codes, h, w, (const long long*)face_offsets, (const long long*)count,
            (const int*)ranks, faces);
  if (!g_dry_run) MG_CHECK_HIP(hipGetLastError());
  return 0;
}
