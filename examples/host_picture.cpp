// host_map.cpp carried on to what the pipelines return and the command line writes: raw image bytes and a seed in, the map at the
// size asked for (clipped), the 16-bit depth and the picture out - __call__ of the reference's depth / normals pipeline with
// match_input_res (marigold/marigold_depth_pipeline.py:154-338, marigold_normals_pipeline.py:139-308) and script/depth/run.py's 16-bit
// PNG values as ONE call of libmarigold_hip.so (include/marigold_hip.h):
//     mg_model_predict_out = mg_rgb_prepare -> encode -> MG_OP_RANDN (the latents) -> denoise -> decode -> ensemble
//                            [-> MG_OP_RESIZE to out_h x out_w] -> the output stage (MG_OP_COLORIZE / mg_normals_finish)
// Build (gfx950 box):  hipcc -O2 examples/host_picture.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_picture
// Run:                 ./host_picture model.mgimg image.u8 Hin Win seed out_prefix [out_h out_w [out_mode [table.lut]]]
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds); resampled to the model's size when it differs (in out_mode)
//   out_h out_w       the pipeline's match_input_res: the size of everything written; default: the decoded size
//   out_mode          0 bilinear (default), 1 bicubic, 2 nearest-exact - the pipelines' resample_method, for both resizes
//   table.lut         768 bytes, the colour map's 256 x RGB table (marigold_amd.image.export_color_table); depth: no table, no .ppm
//   out_prefix.f32        raw fp32 [channels][out_h][out_w], clipped to [0, 1] (depth) / [-1, 1] (normals)
//   out_prefix.unc.f32    raw fp32 [H'][W'] at the decoded size, written when the model runs more than one member
//   out_prefix.pgm        depth: 16-bit binary PGM (big endian), uint16(depth * 65535)
//   out_prefix.ppm        the picture, binary PPM
// The Python pipelines give the same arrays and pictures, bit for bit, with generator=marigold_amd.NativeNoise(seed)
// (tests/test_gpu_predict_out_c_host.py builds and runs this program and compares).
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

static bool write_file(const std::string& path, const char* head, const void* data, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && (!head || fputs(head, f) >= 0) && fwrite(data, 1, bytes, f) == bytes;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "cannot write %s\n", path.c_str());
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 7 && (argc < 9 || argc > 11)) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed out_prefix [out_h out_w [out_mode [table.lut]]]\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[3], argv[4]);
    return 2;
  }
  mg_output_opts out = MG_OUTPUT_OPTS_DEFAULT;
  if (argc >= 9) {
    out.out_h = atoi(argv[7]);
    out.out_w = atoi(argv[8]);
    if (out.out_h <= 0 || out.out_w <= 0) {
      fprintf(stderr, "bad output size %s x %s\n", argv[7], argv[8]);
      return 2;
    }
  }
  if (argc >= 10) out.out_mode = atoi(argv[9]);
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
  const int oh = out.out_h ? out.out_h : Ho, ow = out.out_w ? out.out_w : Wo;
  printf("model image: %d member(s) of %dx%d, %d steps, %.1f MB on the device\n", B, H, W, steps, mg_model_device_bytes(m) / 1e6);
  std::vector<uint8_t> bytes((size_t)Hin * Win * 3);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", bytes.size(), argv[2]);
    return 1;
  }
  fclose(f);
  uint8_t* d_lut = nullptr;
  if (argc == 11) {
    uint8_t table[768];
    f = fopen(argv[10], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[10]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
    out.lut256x3 = d_lut;
  }
  const bool picture = depth ? d_lut != nullptr : true;
  const size_t n_out = (size_t)oh * ow;
  std::vector<float> pred((size_t)C * n_out), unc((size_t)Ho * Wo);
  std::vector<uint16_t> u16(n_out);
  std::vector<uint8_t> pic(3 * n_out);
  uint8_t *d_rgb, *d_pic;
  uint16_t* d_u16;
  float *d_pred, *d_unc;
  HIPCHECK(hipMalloc(&d_rgb, bytes.size()));
  HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
  HIPCHECK(hipMalloc(&d_unc, unc.size() * 4));
  HIPCHECK(hipMalloc(&d_u16, u16.size() * 2));
  HIPCHECK(hipMalloc(&d_pic, pic.size()));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  HIPCHECK(hipMemcpy(d_rgb, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise
  const int reciprocal = Hin != H || Win != W;
  double info[4];
  CHECK(mg_model_predict_out(m, d_rgb, 1, Hin, Win, out.out_mode, reciprocal, seed, nullptr, &out, d_pred, d_unc, depth ? d_u16 : nullptr,
                             picture ? d_pic : nullptr, info, s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
  const std::string prefix = argv[6];
  if (!write_file(prefix + ".f32", nullptr, pred.data(), pred.size() * 4)) return 1;
  if (B > 1) {   // a single member has no uncertainty: nothing was written to d_unc
    HIPCHECK(hipMemcpy(unc.data(), d_unc, unc.size() * 4, hipMemcpyDeviceToHost));
    if (!write_file(prefix + ".unc.f32", nullptr, unc.data(), unc.size() * 4)) return 1;
  }
  char head[64];
  if (depth) {
    HIPCHECK(hipMemcpy(u16.data(), d_u16, u16.size() * 2, hipMemcpyDeviceToHost));
    std::vector<uint8_t> be(2 * n_out);   // PGM's 16-bit samples: most significant byte first
    for (size_t i = 0; i < n_out; ++i) {
      be[2 * i] = (uint8_t)(u16[i] >> 8);
      be[2 * i + 1] = (uint8_t)(u16[i] & 0xff);
    }
    snprintf(head, sizeof(head), "P5\n%d %d\n65535\n", ow, oh);
    if (!write_file(prefix + ".pgm", head, be.data(), be.size())) return 1;
  }
  if (picture) {
    HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
    snprintf(head, sizeof(head), "P6\n%d %d\n255\n", ow, oh);
    if (!write_file(prefix + ".ppm", head, pic.data(), pic.size())) return 1;
  }
  double sum = 0;
  for (float v : pred) sum += v;
  printf("%s map %dx%dx%d written, mean %.6f%s%s; alignment: cost %.6g, %d evaluations, %d iterations, status %d\n", depth ? "depth" : "normals",
         C, oh, ow, sum / pred.size(), B > 1 ? "; uncertainty" : "", picture ? "; picture" : "", info[0], (int)info[1], (int)info[2], (int)info[3]);
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_u16));
  HIPCHECK(hipFree(d_pic));
  if (d_lut) HIPCHECK(hipFree(d_lut));
  mg_model_destroy(m);
  return 0;
}
