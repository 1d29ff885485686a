// host_picture.cpp for the consecutive frames of ONE sequence: raw image bytes and a seed per frame in; per frame the map at the frame's
// own size (clipped), the 16-bit depth and the picture out - what map_video(frames, strength, match_input_res=True) of the depth /
// normals pipeline returns, one mg_model_predict_next call per frame:
//     mg_model_predict_next = mg_model_predict_out, with the denoised latent of the frame before blended into the initial latents
//                             (mg_latent_carry: (1 - strength) noise + strength latent) and this frame's latent kept for the next
// Build (gfx950 box):  hipcc -O2 examples/host_sequence.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_sequence
// Run:                 ./host_sequence model.mgimg Hin Win strength out_prefix [table.lut] -- frame0.u8 seed0 frame1.u8 seed1 ...
//   frame<k>.u8       raw uint8 [Hin][Win][3] (what PIL holds), one size for all frames
//   strength          the weight of the previous frame's latent, in [0, 1] (the recipe's 0.1)
//   table.lut         a depth model's colour table, 768 bytes (marigold_amd.image.export_color_table); without it no depth picture
//   out_prefix.<k>.f32 / .unc.f32 / .pgm / .ppm: the files host_picture.cpp writes, for frame k, at Hin x Win (bilinear)
// The Python pipelines give the same arrays and pictures, bit for bit, with generators=[marigold_amd.NativeNoise(seed_k)]
// (tests/test_gpu_sequence.py builds and runs this program and compares).
// A model image with the tiny autoencoder (export_model_image(..., tiny_vae=True), a version-3 file, MG_CFG_VAE = MG_VAE_TINY) runs through this
// program unchanged: every size it uses comes from cfg16, where the latent and decoded sizes follow that VAE's ceiling rule.
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
  const int sep = argc > 7 && !strcmp(argv[7], "--") ? 7 : 6;
  const int n = argc > sep ? (argc - sep - 1) / 2 : 0;
  if (argc <= sep || strcmp(argv[sep], "--") || n < 1 || (argc - sep - 1) % 2) {
    fprintf(stderr, "usage: %s model.mgimg Hin Win strength out_prefix [table.lut] -- frame0.u8 seed0 [frame1.u8 seed1 ...]\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[2]), Win = atoi(argv[3]);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[2], argv[3]);
    return 2;
  }
  const float strength = strtof(argv[4], nullptr);
  const std::string prefix = argv[5];
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int B = cfg[MG_CFG_MEMBERS], H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH], steps = cfg[MG_CFG_STEPS];
  const int C = cfg[MG_CFG_CHANNELS], post = cfg[MG_CFG_POST], Ho = cfg[MG_CFG_OUT_H], Wo = cfg[MG_CFG_OUT_W];
  const bool depth = post == MG_POST_DEPTH;
  printf("model image: %d member(s), %dx%d, %d steps; %d frame(s), strength %g\n", B, H, W, steps, n, (double)strength);
  mg_output_opts out = MG_OUTPUT_OPTS_DEFAULT;   // match_input_res: every output at the frame's size
  out.out_h = Hin;
  out.out_w = Win;
  uint8_t* d_lut = nullptr;
  if (sep == 7) {
    uint8_t table[768];
    FILE* f = fopen(argv[6], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[6]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
    out.lut256x3 = d_lut;
  }
  const bool picture = depth ? d_lut != nullptr : true;
  const size_t in_bytes = (size_t)Hin * Win * 3, n_out = (size_t)Hin * Win, n_unc = (size_t)Ho * Wo;
  std::vector<uint8_t> bytes(in_bytes), pic(3 * n_out);
  std::vector<float> pred(C * n_out), unc(n_unc);
  std::vector<uint16_t> u16(n_out);
  uint8_t *d_rgb, *d_pic;
  uint16_t* d_u16;
  float *d_pred, *d_unc;
  HIPCHECK(hipMalloc(&d_rgb, in_bytes));
  HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
  HIPCHECK(hipMalloc(&d_unc, unc.size() * 4));
  HIPCHECK(hipMalloc(&d_u16, u16.size() * 2));
  HIPCHECK(hipMalloc(&d_pic, pic.size()));
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
    double info[4];
    // one call per frame: the handle carries the latent from frame to frame
    CHECK(mg_model_predict_next(m, d_rgb, 1, Hin, Win, 0, reciprocal, seed, nullptr, &out, d_pred, d_unc, depth ? d_u16 : nullptr, picture ? d_pic : nullptr, info, s,
                                strength));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
    if (B > 1) HIPCHECK(hipMemcpy(unc.data(), d_unc, unc.size() * 4, hipMemcpyDeviceToHost));   // (one member: nothing was written)
    if (depth) HIPCHECK(hipMemcpy(u16.data(), d_u16, u16.size() * 2, hipMemcpyDeviceToHost));
    if (picture) HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
    const std::string pre = prefix + "." + std::to_string(k);
    if (!write_file(pre + ".f32", nullptr, pred.data(), pred.size() * 4)) return 1;
    if (B > 1 && !write_file(pre + ".unc.f32", nullptr, unc.data(), n_unc * 4)) return 1;
    if (depth) {
      std::vector<uint8_t> be(2 * n_out);   // PGM's 16-bit samples: most significant byte first
      for (size_t j = 0; j < n_out; ++j) {
        be[2 * j] = (uint8_t)(u16[j] >> 8);
        be[2 * j + 1] = (uint8_t)(u16[j] & 0xff);
      }
      snprintf(head, sizeof(head), "P5\n%d %d\n65535\n", Win, Hin);
      if (!write_file(pre + ".pgm", head, be.data(), be.size())) return 1;
    }
    if (picture) {
      snprintf(head, sizeof(head), "P6\n%d %d\n255\n", Win, Hin);
      if (!write_file(pre + ".ppm", head, pic.data(), pic.size())) return 1;
    }
    double sum = 0;
    for (size_t j = 0; j < pred.size(); ++j) sum += pred[j];
    printf("frame %d: %s map %dx%dx%d written, mean %.6f%s\n", k, depth ? "depth" : "normals", C, Hin, Win, sum / pred.size(),
           B > 1 ? "; uncertainty" : "");
  }
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_u16));
  HIPCHECK(hipFree(d_pic));
  if (d_lut) HIPCHECK(hipFree(d_lut));
  mg_model_destroy(m);
  return 0;
}
