// Depth to focus from a C host: raw image bytes, a seed, a camera, a focus pixel and an aperture in; the picture with a shallow depth of
// field, one binary PPM, out - refocus(...) of the Python package as calls of libmarigold_hip.so (include/marigold_hip.h), composed by
// the host because refocusing is no stage of the one-call predictions:
//     mg_model_predict          the ensembled depth map at the decoded size
//     mg_resize (uint8)         the picture's planes brought to that size: the colours that are blurred
//     mg_depth_focus            every pixel blurred by the circle of confusion of a thin lens focused on the pixel's distance, which
//                               the call reads on the device: the host never sees the map
// then ONE read-back: the picture.
// Build (gfx950 box):  hipcc -O2 examples/host_focus.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_focus
// Run:                 ./host_focus model.mgimg image.u8 Hin Win seed fov_deg near far focus_y focus_x aperture max_radius out.ppm
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds); resampled (bilinear) to the model's size when it differs
//   fov_deg           the horizontal field of view of the picture: square pixels; rescaled to the map's size (intrinsics_from_fov,
//                     scale_intrinsics): only the focal length in pixels counts here
//   near far          z = near + depth * (far - near): the model's depth is affine-invariant, the range is the caller's choice
//   focus_y focus_x   the pixel of the MAP to focus on (row, column)
//   aperture          the diameter of the lens in the units of near and far: gain = 0.5 * fx * aperture
//   max_radius        0 .. 32: the largest blur radius in pixels
// The Python package writes the same picture, byte for byte, from pipe(image, generator=NativeNoise(seed), match_input_res=False)
// (tests/test_gpu_focus_c_host.py builds and runs this program and compares).
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
  if (argc != 14) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed fov_deg near far focus_y focus_x aperture max_radius out.ppm\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  const double fov = strtod(argv[6], nullptr), z_near = strtod(argv[7], nullptr), z_far = strtod(argv[8], nullptr);
  const int focus_y = atoi(argv[9]), focus_x = atoi(argv[10]);
  const double aperture = strtod(argv[11], nullptr);
  const int max_radius = atoi(argv[12]);
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
  const int h = cfg[MG_CFG_OUT_H], w = cfg[MG_CFG_OUT_W];   // the decoded size: the map's, and the picture's that is written
  if (cfg[MG_CFG_POST] != MG_POST_DEPTH) {
    fprintf(stderr, "a depth model image is expected\n");
    return 2;
  }
  // the focal length of the picture, then of the map (marigold_amd.points.intrinsics_from_fov and scale_intrinsics, operation for
  // operation), and the gain of the thin lens
  double fx = (Win / 2.0) / tan((fov * (M_PI / 180.0)) / 2.0);
  const bool same = Hin == h && Win == w;
  if (!same) fx = fx * w / Win;
  const double gain = 0.5 * fx * aperture;
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
  const long long ws_bytes = mg_depth_focus_workspace_bytes((long long)n);
  if (ws_bytes < 0) {
    fprintf(stderr, "%s\n", mg_last_error());
    return 1;
  }
  uint8_t *d_rgb, *d_lo, *d_out, *d_valid;
  float *d_pred, *d_unc, *d_tmp;
  double* d_coef;
  long long* d_count;
  void* d_ws;
  HIPCHECK(hipMalloc(&d_rgb, planes.size()));
  HIPCHECK(hipMalloc(&d_lo, 3 * n));
  HIPCHECK(hipMalloc(&d_tmp, (size_t)3 * Hin * w * 4));
  HIPCHECK(hipMalloc(&d_pred, n * 4));
  HIPCHECK(hipMalloc(&d_unc, n * 4));
  HIPCHECK(hipMalloc(&d_out, 3 * n));
  HIPCHECK(hipMalloc(&d_valid, n));
  HIPCHECK(hipMalloc(&d_coef, 2 * sizeof(double)));
  HIPCHECK(hipMalloc(&d_count, 5 * sizeof(long long)));
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
  // 3. the refocused picture: the focus distance is the map's own value at the pixel, read by the call
  CHECK(mg_depth_focus(d_pred, colours, 0, nullptr, d_coef, h, w, 0.0, INFINITY, MG_FOCUS_SPACE_LENS, gain, max_radius, focus_x, focus_y, 0.0, d_out,
                       d_valid, nullptr, d_count, d_ws, ws_bytes, s));
  // the read-back: the picture (planes) and the counts
  HIPCHECK(hipStreamSynchronize(s));
  long long count[5];
  HIPCHECK(hipMemcpy(count, d_count, sizeof(count), hipMemcpyDeviceToHost));
  std::vector<uint8_t> got(3 * n), pic(3 * n);
  HIPCHECK(hipMemcpy(got.data(), d_out, 3 * n, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < n; ++p)
    for (int c = 0; c < 3; ++c) pic[3 * p + c] = got[c * n + p];
  file = fopen(argv[13], "wb");
  bool ok = file != nullptr;
  if (ok) {
    ok = fprintf(file, "P6\n%d %d\n255\n", w, h) > 0;
    ok = ok && fwrite(pic.data(), 1, pic.size(), file) == pic.size();
    ok = fclose(file) == 0 && ok;
  }
  if (!ok) {
    fprintf(stderr, "cannot write %s\n", argv[13]);
    return 1;
  }
  printf("%dx%d: %lld usable pixels, %lld sharp, %lld capped, %lld contributions%s\n", h, w, count[0], count[1], count[2], count[3],
         count[4] ? ", the focus was bad: the picture is the source" : "");
  printf("written to %s\n", argv[13]);
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_lo));
  HIPCHECK(hipFree(d_tmp));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_out));
  HIPCHECK(hipFree(d_valid));
  HIPCHECK(hipFree(d_coef));
  HIPCHECK(hipFree(d_count));
  HIPCHECK(hipFree(d_ws));
  mg_model_destroy(m);
  return 0;
}
