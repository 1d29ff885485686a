// host_picture.cpp for several pictures in ONE call: raw image bytes and a seed per picture in; per picture the map at the size asked
// for (clipped), the 16-bit depth and the picture out - what map_images(images_per_program=K, match_input_res=True) of the depth /
// normals pipeline returns for a group, from a model image exported with export_model_image(..., images_per_program=K):
//     mg_model_predict_many = per picture mg_rgb_prepare -> ONE encode -> per picture MG_OP_RANDN -> ONE denoise -> ONE decode
//                             -> per picture: ensemble [-> MG_OP_RESIZE to out_h x out_w] -> the output stage
// Build (gfx950 box):  hipcc -O2 examples/host_many.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_many
// Run:                 ./host_many model.mgimg Hin Win out_prefix [out_h out_w [out_mode [table.lut]]] -- image0.u8 seed0 image1.u8 seed1 ...
//   image<i>.u8       raw uint8 [Hin][Win][3] (what PIL holds), one size for all; 1 <= pictures <= K of the model image
//   out_h out_w, out_mode, table.lut: as in host_picture.cpp, for every picture
//   out_prefix.<i>.f32 / .unc.f32 / .pgm / .ppm: the files host_picture.cpp writes, for picture i
// The Python pipelines give the same arrays and pictures, bit for bit, with generators=[marigold_amd.NativeNoise(seed_i)]
// (tests/test_gpu_predict_many_c_host.py builds and runs this program and compares).
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
  int sep = -1;
  for (int i = 1; i < argc && sep < 0; ++i)
    if (!strcmp(argv[i], "--")) sep = i;
  const int n = sep < 0 ? 0 : (argc - sep - 1) / 2;
  if ((sep != 5 && sep != 7 && sep != 8 && sep != 9) || n < 1 || (argc - sep - 1) % 2) {
    fprintf(stderr, "usage: %s model.mgimg Hin Win out_prefix [out_h out_w [out_mode [table.lut]]] -- image0.u8 seed0 [image1.u8 seed1 ...]\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[2]), Win = atoi(argv[3]);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[2], argv[3]);
    return 2;
  }
  const std::string prefix = argv[4];
  mg_output_opts out = MG_OUTPUT_OPTS_DEFAULT;
  if (sep >= 7) {
    out.out_h = atoi(argv[5]);
    out.out_w = atoi(argv[6]);
    if (out.out_h <= 0 || out.out_w <= 0) {
      fprintf(stderr, "bad output size %s x %s\n", argv[5], argv[6]);
      return 2;
    }
  }
  if (sep >= 8) out.out_mode = atoi(argv[7]);
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int B = cfg[MG_CFG_MEMBERS], H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH], steps = cfg[MG_CFG_STEPS], C = cfg[MG_CFG_CHANNELS];
  const int post = cfg[MG_CFG_POST], Ho = cfg[MG_CFG_OUT_H], Wo = cfg[MG_CFG_OUT_W], K = MG_CFG_PICTURES_OF(cfg);
  const bool depth = post == MG_POST_DEPTH;
  const int oh = out.out_h ? out.out_h : Ho, ow = out.out_w ? out.out_w : Wo;
  printf("model image: %d picture(s) per call, %d member(s) each, %dx%d, %d steps, %.1f MB on the device\n", K, B, H, W, steps,
         mg_model_device_bytes(m) / 1e6);
  uint8_t* d_lut = nullptr;
  if (sep == 9) {
    uint8_t table[768];
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[8]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
    out.lut256x3 = d_lut;
  }
  // the pictures: one device buffer, one pointer and one seed each
  const size_t in_bytes = (size_t)Hin * Win * 3;
  std::vector<uint8_t> bytes(in_bytes);
  std::vector<const uint8_t*> rgb(n);
  std::vector<uint64_t> seeds(n);
  uint8_t* d_rgb;
  HIPCHECK(hipMalloc(&d_rgb, in_bytes * n));
  for (int i = 0; i < n; ++i) {
    const char* path = argv[sep + 1 + 2 * i];
    FILE* f = fopen(path, "rb");
    if (!f || fread(bytes.data(), 1, in_bytes, f) != in_bytes) {
      fprintf(stderr, "cannot read %zu bytes from %s\n", in_bytes, path);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMemcpy(d_rgb + i * in_bytes, bytes.data(), in_bytes, hipMemcpyHostToDevice));
    rgb[i] = d_rgb + i * in_bytes;
    seeds[i] = strtoull(argv[sep + 2 + 2 * i], nullptr, 0);
  }
  const bool picture = depth ? d_lut != nullptr : true;
  const size_t n_out = (size_t)oh * ow, n_unc = (size_t)Ho * Wo;
  std::vector<float> pred(n * C * n_out), unc(n * n_unc);
  std::vector<uint16_t> u16(n * n_out);
  std::vector<uint8_t> pic(n * 3 * n_out);
  std::vector<double> info(4 * n);
  uint8_t* d_pic;
  uint16_t* d_u16;
  float *d_pred, *d_unc;
  HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
  HIPCHECK(hipMalloc(&d_unc, unc.size() * 4));
  HIPCHECK(hipMalloc(&d_u16, u16.size() * 2));
  HIPCHECK(hipMalloc(&d_pic, pic.size()));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise
  const int reciprocal = Hin != H || Win != W;
  CHECK(mg_model_predict_many(m, n, rgb.data(), 1, Hin, Win, out.out_mode, reciprocal, seeds.data(), nullptr, &out, d_pred, d_unc,
                              depth ? d_u16 : nullptr, picture ? d_pic : nullptr, info.data(), s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
  if (B > 1) HIPCHECK(hipMemcpy(unc.data(), d_unc, unc.size() * 4, hipMemcpyDeviceToHost));   // (one member: nothing was written)
  if (depth) HIPCHECK(hipMemcpy(u16.data(), d_u16, u16.size() * 2, hipMemcpyDeviceToHost));
  if (picture) HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
  char head[64];
  for (int i = 0; i < n; ++i) {
    const std::string pre = prefix + "." + std::to_string(i);
    const float* p = pred.data() + (size_t)i * C * n_out;
    if (!write_file(pre + ".f32", nullptr, p, (size_t)C * n_out * 4)) return 1;
    if (B > 1 && !write_file(pre + ".unc.f32", nullptr, unc.data() + i * n_unc, n_unc * 4)) return 1;
    if (depth) {
      std::vector<uint8_t> be(2 * n_out);   // PGM's 16-bit samples: most significant byte first
      for (size_t j = 0; j < n_out; ++j) {
        be[2 * j] = (uint8_t)(u16[i * n_out + j] >> 8);
        be[2 * j + 1] = (uint8_t)(u16[i * n_out + j] & 0xff);
      }
      snprintf(head, sizeof(head), "P5\n%d %d\n65535\n", ow, oh);
      if (!write_file(pre + ".pgm", head, be.data(), be.size())) return 1;
    }
    if (picture) {
      snprintf(head, sizeof(head), "P6\n%d %d\n255\n", ow, oh);
      if (!write_file(pre + ".ppm", head, pic.data() + (size_t)i * 3 * n_out, 3 * n_out)) return 1;
    }
    double sum = 0;
    for (size_t j = 0; j < (size_t)C * n_out; ++j) sum += p[j];
    printf("picture %d: %s map %dx%dx%d written, mean %.6f%s%s; alignment: cost %.6g, %d evaluations, %d iterations, status %d\n", i,
           depth ? "depth" : "normals", C, oh, ow, sum / (C * n_out), B > 1 ? "; uncertainty" : "", picture ? "; picture" : "", info[4 * i],
           (int)info[4 * i + 1], (int)info[4 * i + 2], (int)info[4 * i + 3]);
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
