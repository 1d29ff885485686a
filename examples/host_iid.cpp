// The intrinsic-image counterpart of host_map.cpp: raw image bytes and a seed in, the ensembled appearance / lighting targets and
// their pictures out - the reference's MarigoldIIDPipeline call with fill_outputs (marigold/marigold_iid_pipeline.py:239-411) as ONE
// call of libmarigold_hip.so (include/marigold_hip.h):
//     mg_model_predict_iid = mg_rgb_prepare -> encode -> MG_OP_RANDN (the latents) -> denoise -> decode -> MG_OP_ENS_IID
//                            [-> MG_OP_RESIZE to out_h x out_w] -> MG_OP_IID_VIS
// Build (gfx950 box):  hipcc -O2 examples/host_iid.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_iid
// Run:                 ./host_iid model.mgimg image.u8 Hin Win seed out_prefix [linear_bits up_to_scale_bits [out_h out_w]]
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds); resampled to the model's size when it differs (bilinear)
//   linear_bits       bit t: target t is predicted in linear space (target_properties[name]["prediction_space"] == "linear")
//   up_to_scale_bits  bit t: target t is up to scale (target_properties[name]["up_to_scale"]); the lighting model: 7 and 6
//   out_h out_w       the pipeline's match_input_res: the prediction resampled (bilinear) to this size; default: the decoded size
//   out_prefix.f32        raw fp32 [3 n_targets][out_h][out_w] in [0, 1], target after target
//   out_prefix.unc.f32    raw fp32 [3 n_targets][H'][W'] at the decoded size, written when the model runs more than one member
//   out_prefix.<t>.ppm    the picture of target t, binary PPM
// The Python pipeline gives the same arrays, uncertainties and pictures, bit for bit, with generator=marigold_amd.NativeNoise(seed)
// (tests/test_gpu_iid_c_host.py builds and runs this program and compares).
// A model image with the tiny autoencoder (export_model_image(..., tiny_vae=True), a version-3 file, MG_CFG_VAE = MG_VAE_TINY) runs through this
// program unchanged: every size it uses comes from cfg16, where the latent and decoded sizes follow that VAE's ceiling rule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "marigold_hip.h"

static_assert(sizeof(mg_iid_opts) == 6 * sizeof(int), "mg_iid_opts: six ints, no padding (marigold_amd/_lib.py::MgIidOpts mirrors it)");

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
  if (argc != 7 && argc != 9 && argc != 11) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed out_prefix [linear_bits up_to_scale_bits [out_h out_w]]\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[3], argv[4]);
    return 2;
  }
  mg_iid_opts opts = MG_IID_OPTS_DEFAULT;
  if (argc >= 9) {
    opts.linear_bits = (int)strtol(argv[7], nullptr, 0);
    opts.up_to_scale_bits = (int)strtol(argv[8], nullptr, 0);
  }
  if (argc == 11) {
    opts.out_h = atoi(argv[9]);
    opts.out_w = atoi(argv[10]);
    if (opts.out_h <= 0 || opts.out_w <= 0) {
      fprintf(stderr, "bad output size %s x %s\n", argv[9], argv[10]);
      return 2;
    }
  }
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int B = cfg[MG_CFG_MEMBERS], H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH], steps = cfg[MG_CFG_STEPS];
  const int C = cfg[MG_CFG_CHANNELS], n = cfg[MG_CFG_MODALITIES], Ho = cfg[MG_CFG_OUT_H], Wo = cfg[MG_CFG_OUT_W];
  const int oh = opts.out_h ? opts.out_h : Ho, ow = opts.out_w ? opts.out_w : Wo;
  printf("model image: %d member(s) of %dx%d, %d steps, %d target(s), %.1f MB on the device\n", B, H, W, steps, n,
         mg_model_device_bytes(m) / 1e6);
  std::vector<uint8_t> bytes((size_t)Hin * Win * 3);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", bytes.size(), argv[2]);
    return 1;
  }
  fclose(f);
  const size_t n_pic = (size_t)(n > 0 ? n : 1) * oh * ow * 3;
  std::vector<float> pred((size_t)C * oh * ow), unc((size_t)C * Ho * Wo);
  std::vector<uint8_t> pics(n_pic);
  uint8_t *d_rgb, *d_pics;
  float *d_pred, *d_unc;
  HIPCHECK(hipMalloc(&d_rgb, bytes.size()));
  HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
  HIPCHECK(hipMalloc(&d_unc, unc.size() * 4));
  HIPCHECK(hipMalloc(&d_pics, pics.size()));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  HIPCHECK(hipMemcpy(d_rgb, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise
  const int reciprocal = Hin != H || Win != W;
  CHECK(mg_model_predict_iid(m, d_rgb, 1, Hin, Win, /*bilinear*/ 0, reciprocal, seed, &opts, d_pred, d_unc, d_pics, s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(pics.data(), d_pics, pics.size(), hipMemcpyDeviceToHost));
  const std::string prefix = argv[6];
  if (!write_file(prefix + ".f32", nullptr, pred.data(), pred.size() * 4)) return 1;
  if (B > 1) {   // a single member has no uncertainty: nothing was written to d_unc
    HIPCHECK(hipMemcpy(unc.data(), d_unc, unc.size() * 4, hipMemcpyDeviceToHost));
    if (!write_file(prefix + ".unc.f32", nullptr, unc.data(), unc.size() * 4)) return 1;
  }
  for (int t = 0; t < n; ++t) {
    char head[64];
    snprintf(head, sizeof(head), "P6\n%d %d\n255\n", ow, oh);
    if (!write_file(prefix + "." + std::to_string(t) + ".ppm", head, pics.data() + (size_t)t * oh * ow * 3, (size_t)oh * ow * 3)) return 1;
  }
  double sum = 0;
  for (float v : pred) sum += v;
  printf("%d target(s) of 3x%dx%d written, mean %.6f%s\n", n, oh, ow, sum / pred.size(), B > 1 ? "; uncertainty written" : "");
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_pics));
  mg_model_destroy(m);
  return 0;
}
