// Depth to views from a C host: raw image bytes, a seed, a camera and a baseline in; a stereo picture, the left eye beside the right
// as one binary PPM, out - stereo_pair(...) of the Python package as calls of libmarigold_hip.so (include/marigold_hip.h), composed by
// the host because views are no stage of the one-call predictions:
//     mg_model_predict          the ensembled depth map at the decoded size
//     mg_resize (uint8)         the picture's planes brought to that size: the colours that are drawn
//     mg_depth_view (twice)     the map's triangles seen from x = -baseline / 2 and from x = +baseline / 2
// then ONE read-back per eye: its picture.
// Build (gfx950 box):  hipcc -O2 examples/host_view.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_view
// Run:                 ./host_view model.mgimg image.u8 Hin Win seed fov_deg near far edge_rel baseline fill out.ppm
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds); resampled (bilinear) to the model's size when it differs
//   fov_deg           the horizontal field of view of the picture: square pixels, the principal point at the centre; rescaled to the
//                     map's size under the pixel-centre rule (intrinsics_from_fov, scale_intrinsics)
//   near far          z = near + depth * (far - near): the model's depth is affine-invariant, the range is the caller's choice
//   edge_rel          no triangle spans two distances that differ by more than this fraction of the nearer one (0: no rule)
//   baseline          the distance between the eyes, in the units of near and far
//   fill              0 .. 64: fill a pixel no triangle covers from the farther of the nearest covered pixels of its row within this
// The Python package writes the same picture, byte for byte, from pipe(image, generator=NativeNoise(seed), match_input_res=False)
// (tests/test_gpu_view_c_host.py builds and runs this program and compares).
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
  if (argc != 13) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed fov_deg near far edge_rel baseline fill out.ppm\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  const double fov = strtod(argv[6], nullptr), z_near = strtod(argv[7], nullptr), z_far = strtod(argv[8], nullptr), edge_rel = strtod(argv[9], nullptr);
  const double baseline = strtod(argv[10], nullptr);
  const int fill = atoi(argv[11]);
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
  const int h = cfg[MG_CFG_OUT_H], w = cfg[MG_CFG_OUT_W];   // the decoded size: the map's, and both eyes'
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
  std::vector<uint8_t> bytes(3 * n_in), planes(3 * n_in);
  FILE* file = fopen(argv[2], "rb");
  if (!file || fread(bytes.data(), 1, bytes.size(), file) != bytes.size()) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", bytes.size(), argv[2]);
    return 1;
  }
  fclose(file);
  for (size_t p = 0; p < n_in; ++p)   // mg_resize reads planes; every call below takes the picture as [3][Hin][Win]
    for (int c = 0; c < 3; ++c) planes[c * n_in + p] = bytes[3 * p + c];
  const long long ws_bytes = mg_depth_view_workspace_bytes((long long)n);
  if (ws_bytes < 0) {
    fprintf(stderr, "%s\n", mg_last_error());
    return 1;
  }
  uint8_t *d_rgb, *d_lo, *d_eye[2], *d_valid;
  float *d_pred, *d_unc, *d_tmp, *d_depth;
  double* d_coef;
  long long* d_count;
  void* d_ws;
  HIPCHECK(hipMalloc(&d_rgb, planes.size()));
  HIPCHECK(hipMalloc(&d_lo, 3 * n));
  HIPCHECK(hipMalloc(&d_tmp, (size_t)3 * Hin * w * 4));
  HIPCHECK(hipMalloc(&d_pred, n * 4));
  HIPCHECK(hipMalloc(&d_unc, n * 4));
  HIPCHECK(hipMalloc(&d_eye[0], 3 * n));
  HIPCHECK(hipMalloc(&d_eye[1], 3 * n));
  HIPCHECK(hipMalloc(&d_depth, n * 4));
  HIPCHECK(hipMalloc(&d_valid, n));
  HIPCHECK(hipMalloc(&d_coef, 2 * sizeof(double)));
  HIPCHECK(hipMalloc(&d_count, 2 * 8 * sizeof(long long)));
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
  // 3. the two eyes: cameras at x = -baseline / 2 and x = +baseline / 2, so t = (+baseline / 2, 0, 0) and (-baseline / 2, 0, 0); the
  //    workspace serves both calls, one after the other on the stream
  for (int eye = 0; eye < 2; ++eye) {
    const double tx = eye == 0 ? baseline / 2.0 : -baseline / 2.0;
    const double pose[12] = {1.0, 0.0, 0.0, tx, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    CHECK(mg_depth_view(d_pred, colours, 0, nullptr, d_coef, h, w, fx, fy, cx, cy, 0.0, INFINITY, edge_rel, pose, fx, fy, cx, cy, h, w, 1e-6, fill,
                        d_eye[eye], d_depth, d_valid, nullptr, d_count + 8 * eye, d_ws, ws_bytes, s));
  }
  // the read-back: the two pictures (planes) and their counts
  HIPCHECK(hipStreamSynchronize(s));
  long long count[16];
  HIPCHECK(hipMemcpy(count, d_count, sizeof(count), hipMemcpyDeviceToHost));
  std::vector<uint8_t> eyes[2] = {std::vector<uint8_t>(3 * n), std::vector<uint8_t>(3 * n)};
  for (int eye = 0; eye < 2; ++eye) HIPCHECK(hipMemcpy(eyes[eye].data(), d_eye[eye], 3 * n, hipMemcpyDeviceToHost));
  // the PPM: rows of 2 w pixels, the left eye's then the right eye's
  std::vector<uint8_t> pic(3 * 2 * n);
  for (int y = 0; y < h; ++y)
    for (int eye = 0; eye < 2; ++eye)
      for (int x = 0; x < w; ++x)
        for (int c = 0; c < 3; ++c) pic[((size_t)y * 2 * w + (size_t)eye * w + x) * 3 + c] = eyes[eye][c * n + (size_t)y * w + x];
  file = fopen(argv[12], "wb");
  bool ok = file != nullptr;
  if (ok) {
    ok = fprintf(file, "P6\n%d %d\n255\n", 2 * w, h) > 0;
    ok = ok && fwrite(pic.data(), 1, pic.size(), file) == pic.size();
    ok = fclose(file) == 0 && ok;
  }
  if (!ok) {
    fprintf(stderr, "cannot write %s\n", argv[12]);
    return 1;
  }
  for (int eye = 0; eye < 2; ++eye)
    printf("%s eye %dx%d: %lld faces, %lld drawn, %lld pixels covered, %lld filled\n", eye == 0 ? "left" : "right", h, w, count[8 * eye],
           count[8 * eye + 1], count[8 * eye + 6], count[8 * eye + 7]);
  printf("written to %s\n", argv[12]);
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_lo));
  HIPCHECK(hipFree(d_tmp));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_eye[0]));
  HIPCHECK(hipFree(d_eye[1]));
  HIPCHECK(hipFree(d_depth));
  HIPCHECK(hipFree(d_valid));
  HIPCHECK(hipFree(d_coef));
  HIPCHECK(hipFree(d_count));
  HIPCHECK(hipFree(d_ws));
  mg_model_destroy(m);
  return 0;
}
