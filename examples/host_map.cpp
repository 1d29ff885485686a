// A host program WITHOUT Python and without input files made by Python: raw image bytes and a seed in, the ensembled map out - the
// reference's pipeline call (marigold/marigold_depth_pipeline.py:154-338, marigold_normals_pipeline.py:139-308, with
// match_input_res=False) as ONE call of libmarigold_hip.so (include/marigold_hip.h):
//     mg_model_predict = mg_rgb_prepare -> encode -> MG_OP_RANDN (the latents) -> denoise -> decode -> ensemble
// Build (gfx950 box):  hipcc -O2 examples/host_map.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_map
// Run:                 ./host_map model.mgimg image.u8 Hin Win seed pred_out.f32
//   image.u8      raw uint8 [Hin][Win][3] (what PIL holds); resampled to the model's size when it differs (bilinear, the pipelines'
//                 default) and normalised as the pipelines' input stage normalises it
//   pred_out.f32  raw fp32 [channels][H'][W'] (depth: 1 channel in [0, 1]; normals: 3 channels); a depth map is also written as a
//                 16-bit binary PGM, pred_out.f32.pgm (65535 = far, the reference's 16-bit PNG values)
// The Python pipelines give the same map, bit for bit, with generator=marigold_amd.NativeNoise(seed)
// (tests/test_gpu_native_noise.py builds and runs this program and compares).
// A model image with the tiny autoencoder (export_model_image(..., tiny_vae=True), a version-3 file, MG_CFG_VAE = MG_VAE_TINY) runs through this
// program unchanged: every size it uses comes from cfg16, where the latent and decoded sizes follow that VAE's ceiling rule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed pred_out.f32\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[3], argv[4]);
    return 2;
  }
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int B = cfg[MG_CFG_MEMBERS], H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH], steps = cfg[MG_CFG_STEPS];
  const int C = cfg[MG_CFG_CHANNELS], Ho = cfg[MG_CFG_OUT_H], Wo = cfg[MG_CFG_OUT_W];
  printf("model image: %d member(s) of %dx%d, %d steps, %d prediction channel(s), %.1f MB on the device\n", B, H, W, steps, C,
         mg_model_device_bytes(m) / 1e6);
  std::vector<uint8_t> bytes((size_t)Hin * Win * 3);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", bytes.size(), argv[2]);
    return 1;
  }
  fclose(f);
  std::vector<float> pred((size_t)C * Ho * Wo);
  uint8_t* d_rgb;
  float* d_pred;
  HIPCHECK(hipMalloc(&d_rgb, bytes.size()));
  HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  HIPCHECK(hipMemcpy(d_rgb, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise
  const int reciprocal = Hin != H || Win != W;
  double info[4] = {0, 0, 0, 0};
  CHECK(mg_model_predict(m, d_rgb, 1, Hin, Win, /*bilinear*/ 0, reciprocal, seed, nullptr, d_pred, nullptr, info, s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[6], "wb");
  if (!f || fwrite(pred.data(), 4, pred.size(), f) != pred.size()) {
    fprintf(stderr, "cannot write %s\n", argv[6]);
    return 1;
  }
  fclose(f);
  if (C == 1) {   // (depth * 65535).astype(uint16), big-endian as PGM wants it
    const std::string pgm = std::string(argv[6]) + ".pgm";
    std::vector<uint8_t> px(pred.size() * 2);
    for (size_t i = 0; i < pred.size(); ++i) {
      const float d = pred[i] < 0.f ? 0.f : pred[i] > 1.f ? 1.f : pred[i];
      const unsigned v = d == d ? (unsigned)(d * 65535.0f) : 0u;
      px[2 * i] = (uint8_t)(v >> 8);
      px[2 * i + 1] = (uint8_t)(v & 0xff);
    }
    f = fopen(pgm.c_str(), "wb");
    if (!f || fprintf(f, "P5\n%d %d\n65535\n", Wo, Ho) < 0 || fwrite(px.data(), 1, px.size(), f) != px.size()) {
      fprintf(stderr, "cannot write %s\n", pgm.c_str());
      return 1;
    }
    fclose(f);
  }
  double sum = 0;
  for (float v : pred) sum += v;
  printf("prediction %dx%dx%d written, mean %.6f; alignment: cost %.6g after %d evaluations / %d iterations (status %d)\n", C, Ho, Wo,
         sum / pred.size(), info[0], (int)info[1], (int)info[2], (int)info[3]);
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_pred));
  mg_model_destroy(m);
  return 0;
}
