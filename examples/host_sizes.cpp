// host_picture.cpp for pictures of DIFFERENT sizes through ONE model image: an image exported for several configurations
// (export_model_image(pipe, path, configs=[...])) holds the programs of each size once and the weights once; per picture the host
//     mg_processed_size    the size the pipeline feeds the VAE for a picture of Hin x Win at processing_res
//     mg_model_find_config the configuration of that size (and of the members asked for) - refused by name if the image has none
//     mg_model_select      from here on every call acts on it; nothing is launched, nothing is uploaded
//     mg_model_predict_out the pipeline's output at the picture's own size (match_input_res): map, 16-bit depth, picture
// Build (gfx950 box):  hipcc -O2 examples/host_sizes.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_sizes
// Run:                 ./host_sizes model.mgimg members out_prefix [table.lut] -- image0.u8 H0 W0 res0 seed0 [image1.u8 H1 W1 res1 seed1 ...]
//   members           the ensemble size to run, -1 = the first configuration of the picture's size
//   image<i>.u8       raw uint8 [Hi][Wi][3] (what PIL holds); res<i>: the processing resolution, 0 = the picture as it is
//   table.lut         the colour table of a depth model's pictures (export_color_table), as in host_picture.cpp
//   out_prefix.<i>.f32 / .unc.f32 / .pgm / .ppm: the files host_picture.cpp writes, for picture i, at Hi x Wi
// The Python pipelines give the same arrays and pictures, bit for bit, with pipe(image, processing_res=res, match_input_res=True,
// generator=marigold_amd.NativeNoise(seed)) (tests/test_gpu_model_configs.py builds and runs this program and compares).
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
  const int n = sep < 0 ? 0 : (argc - sep - 1) / 5;
  if ((sep != 4 && sep != 5) || n < 1 || (argc - sep - 1) % 5) {
    fprintf(stderr, "usage: %s model.mgimg members out_prefix [table.lut] -- image0.u8 H0 W0 res0 seed0 [image1.u8 H1 W1 res1 seed1 ...]\n", argv[0]);
    return 2;
  }
  const int members = atoi(argv[2]);
  const std::string prefix = argv[3];
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  printf("model image: %d configuration(s), %.1f MB of shared weights, %.1f MB of its own on the device\n", mg_model_num_configs(m),
         mg_model_shared_bytes(m) / 1e6, mg_model_device_bytes(m) / 1e6);
  mg_output_opts out = MG_OUTPUT_OPTS_DEFAULT;
  uint8_t* d_lut = nullptr;
  if (sep == 5) {
    uint8_t table[768];
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[4]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
    out.lut256x3 = d_lut;
  }
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  for (int i = 0; i < n; ++i) {
    char** a = argv + sep + 1 + 5 * i;
    const int Hin = atoi(a[1]), Win = atoi(a[2]), res = atoi(a[3]);
    const uint64_t seed = strtoull(a[4], nullptr, 0);
    // the configuration for this picture
    int H, W, cfg[MG_CFG_WORDS];
    CHECK(mg_processed_size(Hin, Win, res, &H, &W));
    const int index = mg_model_find_config(m, H, W, members, -1, 1);
    if (index < 0) {
      fprintf(stderr, "picture %d (%d x %d, processed at %d x %d): %s\n", i, Hin, Win, H, W, mg_last_error());
      return 1;
    }
    CHECK(mg_model_select(m, index));
    CHECK(mg_model_info(m, cfg));
    const int B = cfg[MG_CFG_MEMBERS], C = cfg[MG_CFG_CHANNELS], Ho = cfg[MG_CFG_OUT_H], Wo = cfg[MG_CFG_OUT_W];
    const bool depth = cfg[MG_CFG_POST] == MG_POST_DEPTH, picture = depth ? d_lut != nullptr : true;
    // the picture in, the outputs at its own size
    const size_t in_bytes = (size_t)Hin * Win * 3, n_out = (size_t)Hin * Win, n_unc = (size_t)Ho * Wo;
    std::vector<uint8_t> bytes(in_bytes), pic(3 * n_out);
    std::vector<float> pred(C * n_out), unc(n_unc);
    std::vector<uint16_t> u16(n_out);
    FILE* f = fopen(a[0], "rb");
    if (!f || fread(bytes.data(), 1, in_bytes, f) != in_bytes) {
      fprintf(stderr, "cannot read %zu bytes from %s\n", in_bytes, a[0]);
      return 1;
    }
    fclose(f);
    uint8_t *d_rgb, *d_pic;
    uint16_t* d_u16;
    float *d_pred, *d_unc;
    HIPCHECK(hipMalloc(&d_rgb, in_bytes));
    HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
    HIPCHECK(hipMalloc(&d_unc, unc.size() * 4));
    HIPCHECK(hipMalloc(&d_u16, u16.size() * 2));
    HIPCHECK(hipMalloc(&d_pic, pic.size()));
    HIPCHECK(hipMemcpy(d_rgb, bytes.data(), in_bytes, hipMemcpyHostToDevice));
    out.out_h = Hin;
    out.out_w = Win;
    double info[4];
    // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise
    const int reciprocal = Hin != H || Win != W;
    CHECK(mg_model_predict_out(m, d_rgb, 1, Hin, Win, 0, reciprocal, seed, nullptr, &out, d_pred, d_unc, depth ? d_u16 : nullptr,
                               picture ? d_pic : nullptr, info, s));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
    if (B > 1) HIPCHECK(hipMemcpy(unc.data(), d_unc, unc.size() * 4, hipMemcpyDeviceToHost));   // (one member: nothing was written)
    if (depth) HIPCHECK(hipMemcpy(u16.data(), d_u16, u16.size() * 2, hipMemcpyDeviceToHost));
    if (picture) HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
    const std::string pre = prefix + "." + std::to_string(i);
    char head[64];
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
    for (float v : pred) sum += v;
    printf("picture %d: %d x %d -> configuration %d (%d x %d, %d member(s), %d steps): %s map %dx%dx%d written, mean %.6f%s%s\n", i, Hin, Win,
           index, H, W, B, cfg[MG_CFG_STEPS], depth ? "depth" : "normals", C, Hin, Win, sum / pred.size(), B > 1 ? "; uncertainty" : "",
           picture ? "; picture" : "");
    HIPCHECK(hipFree(d_rgb));
    HIPCHECK(hipFree(d_pred));
    HIPCHECK(hipFree(d_unc));
    HIPCHECK(hipFree(d_u16));
    HIPCHECK(hipFree(d_pic));
  }
  HIPCHECK(hipStreamDestroy(s));
  if (d_lut) HIPCHECK(hipFree(d_lut));
  mg_model_destroy(m);
  return 0;
}
