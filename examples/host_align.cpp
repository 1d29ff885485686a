// host_sequence.cpp with every frame's depth map ALIGNED to the frame before: raw image bytes and a seed per frame in; per frame the map
// at the frame's own size (clipped), the 16-bit depth and the picture out - what map_video(frames, strength, align=dict(delta=..,
// iters=.., reference=..)) of the depth pipeline returns.  Alignment is no stage of the one-call predictions, so the host composes the
// chain per frame from calls of libmarigold_hip.so (include/marigold_hip.h):
//     mg_model_predict_next     the ensembled map at the decoded size, started from the latent of the frame before
//     mg_depth_align_fit        the robust scale and shift that carry it onto the kept reference (frame 0 is the first reference)
//     mg_depth_align_apply      s * map + t, unclipped - under "previous" the next reference; the uncertainty times s
//     mg_resize                 the pipelines' match_input_res, where the frame's size is not the decoded one
//     mg_depth_visualize        the pipelines' output stage: the clip, the 16-bit depth, the picture
// Nothing is read back between the calls: the coefficients stay on the device from the fit to the apply.
// Build (gfx950 box):  hipcc -O2 examples/host_align.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_align
// Run:                 ./host_align model.mgimg Hin Win strength delta iters reference out_prefix [table.lut] -- frame0.u8 seed0 frame1.u8 seed1 ...
//   frame<k>.u8       raw uint8 [Hin][Win][3] (what PIL holds), one size for all frames
//   strength          the weight of the previous frame's latent, in [0, 1] (the recipe's 0.1)
//   delta iters       of mg_depth_align_fit: the residual at which a pixel's weight is a half (0.05), the reweighted solves (4)
//   reference         previous | first: what a frame is fitted to
//   table.lut         the colour table, 768 bytes (marigold_amd.image.export_color_table); without it no picture
//   out_prefix.<k>.f32 / .unc.f32 / .pgm / .ppm: the files host_sequence.cpp writes, for frame k; out_prefix.<k>.coef: s, t as two
//   doubles and the flag as a third
// The Python pipeline gives the same arrays and pictures, bit for bit, with generators=[marigold_amd.NativeNoise(seed_k)]
// (tests/test_gpu_align_pipeline.py builds and runs this program and compares).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
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

static bool write_file(const std::string& path, const char* head, const void* data, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && (!head || fputs(head, f) >= 0) && fwrite(data, 1, bytes, f) == bytes;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "cannot write %s\n", path.c_str());
  return ok;
}

int main(int argc, char** argv) {
  const int sep = argc > 10 && !strcmp(argv[10], "--") ? 10 : 9;
  const int n = argc > sep ? (argc - sep - 1) / 2 : 0;
  if (argc <= sep || strcmp(argv[sep], "--") || n < 1 || (argc - sep - 1) % 2) {
    fprintf(stderr, "usage: %s model.mgimg Hin Win strength delta iters previous|first out_prefix [table.lut] -- frame0.u8 seed0 [frame1.u8 seed1 ...]\n",
            argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[2]), Win = atoi(argv[3]);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[2], argv[3]);
    return 2;
  }
  const float strength = strtof(argv[4], nullptr);
  const double delta = strtod(argv[5], nullptr);
  const int iters = atoi(argv[6]);
  if (strcmp(argv[7], "previous") && strcmp(argv[7], "first")) {
    fprintf(stderr, "the reference is `previous` or `first`, not %s\n", argv[7]);
    return 2;
  }
  const bool previous = !strcmp(argv[7], "previous");
  const std::string prefix = argv[8];
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int B = cfg[MG_CFG_MEMBERS], H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH], steps = cfg[MG_CFG_STEPS];
  const int Ho = cfg[MG_CFG_OUT_H], Wo = cfg[MG_CFG_OUT_W];
  if (cfg[MG_CFG_POST] != MG_POST_DEPTH) {
    fprintf(stderr, "a depth model image is expected: only depth has a scale and shift to align\n");
    return 2;
  }
  printf("model image: %d member(s), %dx%d, %d steps; %d frame(s), strength %g; aligned to the %s frame, delta %g, %d solve(s)\n", B, H, W, steps, n,
         (double)strength, previous ? "previous" : "first", delta, iters);
  uint8_t* d_lut = nullptr;
  if (sep == 10) {
    uint8_t table[768];
    FILE* f = fopen(argv[9], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[9]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
  }
  const bool picture = d_lut != nullptr, enlarge = Hin != Ho || Win != Wo;
  const size_t in_bytes = (size_t)Hin * Win * 3, n_out = (size_t)Hin * Win, n_lo = (size_t)Ho * Wo;
  const long long ws_bytes = mg_depth_align_workspace_bytes((long long)n_lo);
  if (ws_bytes < 0) {
    fprintf(stderr, "%s\n", mg_last_error());
    return 1;
  }
  std::vector<uint8_t> bytes(in_bytes), pic(3 * n_out);
  std::vector<float> pred(n_out), unc(n_lo);
  std::vector<uint16_t> u16(n_out);
  uint8_t *d_rgb, *d_pic;
  uint16_t* d_u16;
  float *d_pred, *d_unc, *d_ref, *d_aligned, *d_tmp, *d_out;
  double* d_coef;
  int* d_flag;
  void* d_ws;
  HIPCHECK(hipMalloc(&d_rgb, in_bytes));
  HIPCHECK(hipMalloc(&d_pred, n_lo * 4));
  HIPCHECK(hipMalloc(&d_unc, n_lo * 4));
  HIPCHECK(hipMalloc(&d_ref, n_lo * 4));
  HIPCHECK(hipMalloc(&d_aligned, n_lo * 4));
  HIPCHECK(hipMalloc(&d_tmp, (size_t)Ho * Win * 4));
  HIPCHECK(hipMalloc(&d_out, n_out * 4));
  HIPCHECK(hipMalloc(&d_u16, n_out * 2));
  HIPCHECK(hipMalloc(&d_pic, 3 * n_out));
  HIPCHECK(hipMalloc(&d_coef, 2 * sizeof(double)));
  HIPCHECK(hipMalloc(&d_flag, sizeof(int)));
  HIPCHECK(hipMalloc(&d_ws, (size_t)ws_bytes));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise
  const int reciprocal = Hin != H || Win != W;
  char head[64];
  for (int k = 0; k < n; ++k) {
    const char* path = argv[sep + 1 + 2 * k];
    const uint64_t seed = strtoull(argv[sep + 2 + 2 * k], nullptr, 0);
    FILE* f = fopen(path, "rb");
    if (!f || fread(bytes.data(), 1, in_bytes, f) != in_bytes) {
      fprintf(stderr, "cannot read %zu bytes from %s\n", in_bytes, path);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMemcpyAsync(d_rgb, bytes.data(), in_bytes, hipMemcpyHostToDevice, s));
    double info[4], coef[3] = {1.0, 0.0, 0.0};
    // 1. the ensembled map at the decoded size (its clip to [0, 1] changes nothing: the map lies there already)
    CHECK(mg_model_predict_next(m, d_rgb, 1, Hin, Win, 0, reciprocal, seed, nullptr, nullptr, d_pred, d_unc, nullptr, nullptr, info, s, strength));
    const float* map = d_pred;
    if (k == 0) {   // the first frame passes as it is and becomes the reference
      HIPCHECK(hipMemcpyAsync(d_ref, d_pred, n_lo * 4, hipMemcpyDeviceToDevice, s));
    } else {
      // 2. the fit from (1, 0), 3. s * map + t without a clip, the uncertainty times s in place
      CHECK(mg_depth_align_fit(d_pred, d_ref, nullptr, (long long)n_lo, 1, iters, MG_ALIGN_START_GIVEN, 1.0, 0.0, delta, d_coef, d_flag, d_ws, ws_bytes, s));
      CHECK(mg_depth_align_apply(d_pred, (long long)n_lo, d_coef, 1, 1.f, 0.f, d_aligned, s));
      if (B > 1) CHECK(mg_depth_align_apply(d_unc, (long long)n_lo, d_coef, 0, 1.f, 0.f, d_unc, s));
      if (previous) HIPCHECK(hipMemcpyAsync(d_ref, d_aligned, n_lo * 4, hipMemcpyDeviceToDevice, s));
      map = d_aligned;
    }
    // 4. to the frame's size, 5. the output stage
    if (enlarge) CHECK(mg_resize(map, d_out, d_tmp, 1, Ho, Wo, Hin, Win, 0, 0, s));
    else HIPCHECK(hipMemcpyAsync(d_out, map, n_out * 4, hipMemcpyDeviceToDevice, s));
    CHECK(mg_depth_visualize(d_out, d_lut, (int64_t)n_out, d_out, d_u16, picture ? d_pic : nullptr, s));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipMemcpy(pred.data(), d_out, n_out * 4, hipMemcpyDeviceToHost));
    if (B > 1) HIPCHECK(hipMemcpy(unc.data(), d_unc, n_lo * 4, hipMemcpyDeviceToHost));   // (one member: nothing was written)
    HIPCHECK(hipMemcpy(u16.data(), d_u16, n_out * 2, hipMemcpyDeviceToHost));
    if (picture) HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
    if (k > 0) {
      int flag = 0;
      HIPCHECK(hipMemcpy(coef, d_coef, 2 * sizeof(double), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost));
      coef[2] = flag;
    }
    const std::string pre = prefix + "." + std::to_string(k);
    if (!write_file(pre + ".f32", nullptr, pred.data(), n_out * 4)) return 1;
    if (B > 1 && !write_file(pre + ".unc.f32", nullptr, unc.data(), n_lo * 4)) return 1;
    if (!write_file(pre + ".coef", nullptr, coef, sizeof(coef))) return 1;
    std::vector<uint8_t> be(2 * n_out);   // PGM's 16-bit samples: most significant byte first
    for (size_t j = 0; j < n_out; ++j) {
      be[2 * j] = (uint8_t)(u16[j] >> 8);
      be[2 * j + 1] = (uint8_t)(u16[j] & 0xff);
    }
    snprintf(head, sizeof(head), "P5\n%d %d\n65535\n", Win, Hin);
    if (!write_file(pre + ".pgm", head, be.data(), be.size())) return 1;
    if (picture) {
      snprintf(head, sizeof(head), "P6\n%d %d\n255\n", Win, Hin);
      if (!write_file(pre + ".ppm", head, pic.data(), pic.size())) return 1;
    }
    double sum = 0;
    for (size_t j = 0; j < n_out; ++j) sum += pred[j];
    printf("frame %d: depth map %dx%d written, mean %.6f, s %.9g, t %.9g%s%s\n", k, Hin, Win, sum / n_out, coef[0], coef[1],
           coef[2] != 0.0 ? " (degenerate: passed unchanged)" : "", B > 1 ? "; uncertainty" : "");
  }
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_ref));
  HIPCHECK(hipFree(d_aligned));
  HIPCHECK(hipFree(d_tmp));
  HIPCHECK(hipFree(d_out));
  HIPCHECK(hipFree(d_u16));
  HIPCHECK(hipFree(d_pic));
  HIPCHECK(hipFree(d_coef));
  HIPCHECK(hipFree(d_flag));
  HIPCHECK(hipFree(d_ws));
  if (d_lut) HIPCHECK(hipFree(d_lut));
  mg_model_destroy(m);
  return 0;
}
