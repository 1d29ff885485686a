// Depth to mesh from a C host: raw image bytes, a seed and a camera in; a coloured triangle mesh, a binary PLY that 3D viewers open,
// out - depth_to_mesh(...).write_ply of the Python package as calls of libmarigold_hip.so (include/marigold_hip.h), composed by the host
// because meshes are no stage of the one-call predictions:
//     mg_model_predict          the ensembled depth map at the decoded size
//     mg_resize (uint8)         the picture's planes brought to that size: the vertices' colours
//     mg_depth_mesh             vertices in row-major pixel order, faces in row-major cell order; their numbers stay on the device
// then ONE read-back: `count`, and the records it tells of.
// Build (gfx950 box):  hipcc -O2 examples/host_mesh.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_mesh
// Run:                 ./host_mesh model.mgimg image.u8 Hin Win seed fov_deg near far edge_rel normals out.ply
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds); resampled (bilinear) to the model's size when it differs
//   fov_deg           the horizontal field of view of the picture: square pixels, the principal point at the centre; rescaled to the
//                     map's size under the pixel-centre rule (intrinsics_from_fov, scale_intrinsics)
//   near far          z = near + depth * (far - near): the model's depth is affine-invariant, the range is the caller's choice
//   edge_rel          no triangle spans two distances that differ by more than this fraction of the nearer one (0: no rule)
//   normals           0 | 1: add nx ny nz, in the camera's frame, to the vertex records
// The Python package writes the same file, byte for byte, from pipe(image, generator=NativeNoise(seed), match_input_res=False)
// (tests/test_gpu_mesh_c_host.py builds and runs this program and compares).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "marigold_hip.h"

#define CHECK(x)                                                              \
  do {                                                                        \
    if ((x) != 0) {                                                           \
      fprintf(stderr, "%s failed: %s\n", #x, mg_last_error());                \
      return 1;                                                               \
    }                                                                         \
  } while (0)
#define HIPCHECK(x)                                                           \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));          \
      return 1;                                                               \
    }                                                                         \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 12) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed fov_deg near far edge_rel normals out.ply\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  const double fov = strtod(argv[6], nullptr), z_near = strtod(argv[7], nullptr), z_far = strtod(argv[8], nullptr), edge_rel = strtod(argv[9], nullptr);
  const bool normals = atoi(argv[10]) != 0;
  if (Hin <= 0 || Win <= 0 || !(fov > 0.0 && fov < 180.0) || !(z_near >= 0.0 && z_far > z_near)) {
    fprintf(stderr, "bad image size %s x %s, field of view %s or range %s .. %s\n", argv[3], argv[4], argv[6], argv[7], argv[8]);
    return 2;
  }
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH];
  const int h = cfg[MG_CFG_OUT_H], w = cfg[MG_CFG_OUT_W];   // the decoded size: the map's
  if (cfg[MG_CFG_POST] != MG_POST_DEPTH) {
    fprintf(stderr, "a depth model image is expected\n");
    return 2;
  }
  // the camera of the picture, then of the map (marigold_amd.points.intrinsics_from_fov and scale_intrinsics, operation for operation)
  const double f = (Win / 2.0) / tan((fov * (M_PI / 180.0)) / 2.0);
  const bool same = Hin == h && Win == w;
  double fx = f, fy = f, cx = (Win - 1) / 2.0, cy = (Hin - 1) / 2.0;
  if (!same) {
    fx = fx * w / Win;
    fy = fy * h / Hin;
    cx = (cx + 0.5) * w / Win - 0.5;
    cy = (cy + 0.5) * h / Hin - 0.5;
  }
  const size_t n_in = (size_t)Hin * Win, n = (size_t)h * w;
  const size_t cap_f = (h > 1 && w > 1) ? 2 * (size_t)(h - 1) * (w - 1) : 1;   // every cell's two triangles: nothing is cut
  std::vector<uint8_t> bytes(3 * n_in), planes(3 * n_in);
  FILE* file = fopen(argv[2], "rb");
  if (!file || fread(bytes.data(), 1, bytes.size(), file) != bytes.size()) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", bytes.size(), argv[2]);
    return 1;
  }
  fclose(file);
  for (size_t p = 0; p < n_in; ++p)   // mg_resize reads planes; every call below takes the picture as [3][Hin][Win]
    for (int c = 0; c < 3; ++c) planes[c * n_in + p] = bytes[3 * p + c];
  const long long ws_bytes = mg_depth_mesh_workspace_bytes((long long)n);
  if (ws_bytes < 0) {
    fprintf(stderr, "%s\n", mg_last_error());
    return 1;
  }
  uint8_t *d_rgb, *d_lo, *d_col;
  float *d_pred, *d_unc, *d_tmp, *d_xyz, *d_nrm;
  int* d_faces;
  double* d_coef;
  long long* d_count;
  void* d_ws;
  HIPCHECK(hipMalloc(&d_rgb, planes.size()));
  HIPCHECK(hipMalloc(&d_lo, 3 * n));
  HIPCHECK(hipMalloc(&d_tmp, (size_t)3 * Hin * w * 4));
  HIPCHECK(hipMalloc(&d_pred, n * 4));
  HIPCHECK(hipMalloc(&d_unc, n * 4));
  HIPCHECK(hipMalloc(&d_xyz, 3 * n * 4));
  HIPCHECK(hipMalloc(&d_nrm, 3 * n * 4));
  HIPCHECK(hipMalloc(&d_col, 3 * n));
  HIPCHECK(hipMalloc(&d_faces, 3 * cap_f * 4));
  HIPCHECK(hipMalloc(&d_coef, 2 * sizeof(double)));
  HIPCHECK(hipMalloc(&d_count, 4 * sizeof(long long)));
  HIPCHECK(hipMalloc(&d_ws, (size_t)ws_bytes));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  const double coef[2] = {z_far - z_near, z_near};
  HIPCHECK(hipMemcpy(d_rgb, planes.data(), planes.size(), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_coef, coef, sizeof(coef), hipMemcpyHostToDevice));
  // 1. the prediction; the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides otherwise
  const int reciprocal = Hin != H || Win != W;
  double info[4];
  CHECK(mg_model_predict(m, d_rgb, 0, Hin, Win, 0, reciprocal, seed, nullptr, d_pred, d_unc, info, s));
  // 2. the colours at the map's size (a picture of that size is its own)
  const uint8_t* colours = d_rgb;
  if (!same) {
    CHECK(mg_resize(d_rgb, d_lo, d_tmp, 3, Hin, Win, h, w, 0, 1, s));
    colours = d_lo;
  }
  // 3. the mesh: room for every pixel and for two triangles per cell
  CHECK(mg_depth_mesh(d_pred, colours, 0, nullptr, d_coef, h, w, fx, fy, cx, cy, 0.0, INFINITY, edge_rel, MG_NORMALS_FRAME_CAMERA, (long long)n,
                      (long long)cap_f, d_xyz, d_col, normals ? d_nrm : nullptr, nullptr, d_faces, d_count, d_ws, ws_bytes, s));
  // the one read-back
  HIPCHECK(hipStreamSynchronize(s));
  long long count[4];
  HIPCHECK(hipMemcpy(count, d_count, sizeof(count), hipMemcpyDeviceToHost));
  const size_t vertices = (size_t)count[1], triangles = (size_t)count[3];
  std::vector<float> xyz(3 * vertices), nrm(normals ? 3 * vertices : 0);
  std::vector<uint8_t> col(3 * vertices);
  std::vector<int32_t> faces(3 * triangles);
  HIPCHECK(hipMemcpy(xyz.data(), d_xyz, xyz.size() * 4, hipMemcpyDeviceToHost));
  if (normals) HIPCHECK(hipMemcpy(nrm.data(), d_nrm, nrm.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(col.data(), d_col, col.size(), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(faces.data(), d_faces, faces.size() * 4, hipMemcpyDeviceToHost));
  // the PLY of marigold_amd.mesh.write_mesh_ply: packed little-endian vertex records of 15 or 27 bytes, then faces of 13
  const size_t stride = normals ? 27 : 15;
  std::vector<uint8_t> rec(vertices * stride + triangles * 13);
  for (size_t i = 0; i < vertices; ++i) {
    uint8_t* r = rec.data() + i * stride;
    memcpy(r, &xyz[3 * i], 12);
    if (normals) memcpy(r + 12, &nrm[3 * i], 12);
    memcpy(r + stride - 3, &col[3 * i], 3);
  }
  for (size_t i = 0; i < triangles; ++i) {
    uint8_t* r = rec.data() + vertices * stride + i * 13;
    r[0] = 3;
    memcpy(r + 1, &faces[3 * i], 12);
  }
  file = fopen(argv[11], "wb");
  bool ok = file != nullptr;
  if (ok) {
    ok = fprintf(file, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n", vertices) > 0;
    if (normals) ok = ok && fputs("property float nx\nproperty float ny\nproperty float nz\n", file) >= 0;
    ok = ok && fputs("property uchar red\nproperty uchar green\nproperty uchar blue\n", file) >= 0;
    ok = ok && fprintf(file, "element face %zu\nproperty list uchar int vertex_indices\nend_header\n", triangles) > 0;
    ok = ok && fwrite(rec.data(), 1, rec.size(), file) == rec.size();
    ok = fclose(file) == 0 && ok;
  }
  if (!ok) {
    fprintf(stderr, "cannot write %s\n", argv[11]);
    return 1;
  }
  printf("depth map %dx%d: %lld vertices and %lld faces, %zu and %zu written to %s\n", h, w, count[0], count[2], vertices, triangles, argv[11]);
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_lo));
  HIPCHECK(hipFree(d_tmp));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_xyz));
  HIPCHECK(hipFree(d_nrm));
  HIPCHECK(hipFree(d_col));
  HIPCHECK(hipFree(d_faces));
  HIPCHECK(hipFree(d_coef));
  HIPCHECK(hipFree(d_count));
  HIPCHECK(hipFree(d_ws));
  mg_model_destroy(m);
  return 0;
}
