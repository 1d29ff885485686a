// A LARGE picture through a model image in ONE call: raw image bytes, a seed, the tile size and the overlap in; the stitched map at the
// size asked for (clipped), the stitched uncertainty, the 16-bit depth and the picture out - what pipe.predict_tiled(match_input_res=True)
// of the depth / normals pipeline returns, from a model image of several configurations (export_model_image(configs=[...])): one of
// the tile size with K tiles per call, and for depth one of the guide's processed size with one picture per call:
//     mg_model_predict_tiled = mg_tile_plan -> [depth: the guide, the chain of mg_model_predict] -> per group of K tiles: mg_tile_crop
//                              -> the chain of mg_model_predict_many -> [depth: mg_tile_fit] -> mg_tile_blend (map, uncertainty)
//                              [-> MG_OP_RESIZE to out_h x out_w] -> the output stage
// Build (gfx950 box):  hipcc -O2 examples/host_tiled.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_tiled
// Run:                 ./host_tiled model.mgimg image.u8 Hin Win seed th tw overlap_y overlap_x guide_res out_prefix [out_h out_w [out_mode [table.lut]]]
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds), Hin and Win multiples of 8
//   th tw             the tile size: the image's configuration of that size with the most tiles per call runs the tiles
//   (the short last group of n mod K tiles runs on the configuration of that many tiles per call, if the image holds one)
//   guide_res         depth: the guide is the prediction of the configuration of mg_processed_size(Hin, Win, guide_res), with the
//                     tiles' members and steps, one picture per call (normals: not used, pass 0)
//   out_h out_w, out_mode, table.lut: as in host_picture.cpp (default: the picture's size)
//   out_prefix.f32 / .unc.f32 (several members) / .pgm (depth) / .ppm: the files host_picture.cpp writes; .unc.f32 is [Hin][Win]
// The Python pipelines give the same arrays and pictures, bit for bit, with generator=marigold_amd.NativeNoise(seed), in_flight=1 and
// tiles_per_program=K (tests/test_gpu_predict_tiled_c_host.py builds and runs this program and compares).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "marigold_hip.h"

static_assert(sizeof(mg_tiled_opts) == 20, "mg_tiled_opts: five ints");

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
  if (argc != 12 && argc != 14 && argc != 15 && argc != 16) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed th tw overlap_y overlap_x guide_res out_prefix [out_h out_w [out_mode [table.lut]]]\n",
            argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]), th = atoi(argv[6]), tw = atoi(argv[7]), guide_res = atoi(argv[10]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  if (Hin <= 0 || Win <= 0 || th <= 0 || tw <= 0 || guide_res < 0) {
    fprintf(stderr, "bad sizes: picture %s x %s, tiles %s x %s, guide_res %s\n", argv[3], argv[4], argv[6], argv[7], argv[10]);
    return 2;
  }
  mg_tiled_opts tiled = {-1, -1, atoi(argv[8]), atoi(argv[9]), -1};
  const std::string prefix = argv[11];
  mg_output_opts out = MG_OUTPUT_OPTS_DEFAULT;
  if (argc >= 14) {
    out.out_h = atoi(argv[12]);
    out.out_w = atoi(argv[13]);
    if (out.out_h <= 0 || out.out_w <= 0) {
      fprintf(stderr, "bad output size %s x %s\n", argv[12], argv[13]);
      return 2;
    }
  }
  if (argc >= 15) out.out_mode = atoi(argv[14]);
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  // the tile configuration: of the tile size, the most tiles per call
  int cfg[MG_CFG_WORDS], K = 0;
  for (int c = 0; c < mg_model_num_configs(m); ++c) {
    CHECK(mg_model_config_info(m, c, cfg));
    const int k = MG_CFG_PICTURES_OF(cfg);
    if (cfg[MG_CFG_HEIGHT] == th && cfg[MG_CFG_WIDTH] == tw && k > K) {
      tiled.tile_config = c;
      K = k;
    }
  }
  if (tiled.tile_config < 0) {
    fprintf(stderr, "the model image holds no configuration of %d x %d\n", th, tw);
    return 1;
  }
  CHECK(mg_model_config_info(m, tiled.tile_config, cfg));
  const int B = cfg[MG_CFG_MEMBERS], steps = cfg[MG_CFG_STEPS], C = cfg[MG_CFG_CHANNELS], post = cfg[MG_CFG_POST];
  const bool depth = post == MG_POST_DEPTH;
  int Hg = 0, Wg = 0;
  if (depth) {
    CHECK(mg_processed_size(Hin, Win, guide_res, &Hg, &Wg));
    tiled.guide_config = mg_model_find_config(m, Hg, Wg, B, steps, 1);
    if (tiled.guide_config < 0) {
      fprintf(stderr, "no guide configuration: %s\n", mg_last_error());
      return 1;
    }
  }
  const int oh = out.out_h ? out.out_h : Hin, ow = out.out_w ? out.out_w : Win;
  printf("model image: tiles %dx%d, %d per call, %d member(s) each, %d steps; guide %dx%d\n", th, tw, K, B, steps, Hg, Wg);
  uint8_t* d_lut = nullptr;
  if (argc == 16) {
    uint8_t table[768];
    FILE* f = fopen(argv[15], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[15]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
    out.lut256x3 = d_lut;
  }
  const size_t in_bytes = (size_t)Hin * Win * 3;
  std::vector<uint8_t> bytes(in_bytes);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(bytes.data(), 1, in_bytes, f) != in_bytes) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", in_bytes, argv[2]);
    return 1;
  }
  fclose(f);
  // the number of tiles, for the flags: the plan the call makes
  int starts[MG_TILE_MAX_PER_AXIS];
  const int ny = mg_tile_plan(Hin, th, tiled.overlap_y, starts, MG_TILE_MAX_PER_AXIS);
  const int nx = mg_tile_plan(Win, tw, tiled.overlap_x, starts, MG_TILE_MAX_PER_AXIS);
  if (ny < 1 || nx < 1) {
    fprintf(stderr, "%s\n", mg_last_error());
    return 1;
  }
  const int n = ny * nx;
  // the short last group runs on a configuration of exactly that many tiles per call where the image holds one (what map_images
  // does: predict_tiled's bits); else the call pads it
  if (n % K) {
    tiled.tail_config = mg_model_find_config(m, th, tw, B, steps, n % K);
    if (tiled.tail_config >= 0) {
      int tail[MG_CFG_WORDS];
      CHECK(mg_model_config_info(m, tiled.tail_config, tail));
      if (tail[MG_CFG_CHANNELS] != C || tail[MG_CFG_POST] != post) tiled.tail_config = -1;
    }
  }
  const bool picture = depth ? d_lut != nullptr : true;
  const size_t n_out = (size_t)oh * ow, n_unc = (size_t)Hin * Win;
  std::vector<float> pred(C * n_out), unc(n_unc);
  std::vector<uint16_t> u16(n_out);
  std::vector<uint8_t> pic(3 * n_out);
  std::vector<int> flags(n, 0);
  double info[4];
  uint8_t *d_rgb, *d_pic;
  uint16_t* d_u16;
  float *d_pred, *d_unc;
  int* d_flags;
  HIPCHECK(hipMalloc(&d_rgb, in_bytes));
  HIPCHECK(hipMemcpy(d_rgb, bytes.data(), in_bytes, hipMemcpyHostToDevice));
  HIPCHECK(hipMalloc(&d_pred, pred.size() * 4));
  HIPCHECK(hipMalloc(&d_unc, unc.size() * 4));
  HIPCHECK(hipMalloc(&d_u16, u16.size() * 2));
  HIPCHECK(hipMalloc(&d_pic, pic.size()));
  HIPCHECK(hipMalloc(&d_flags, flags.size() * sizeof(int)));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  // the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides by 255 otherwise (the guide)
  const int reciprocal = depth && (Hin != Hg || Win != Wg);
  CHECK(mg_model_predict_tiled(m, d_rgb, 1, Hin, Win, out.out_mode, reciprocal, seed, &tiled, nullptr, &out, d_pred, d_unc, depth ? d_u16 : nullptr,
                               picture ? d_pic : nullptr, info, depth ? d_flags : nullptr, s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(pred.data(), d_pred, pred.size() * 4, hipMemcpyDeviceToHost));
  if (B > 1) HIPCHECK(hipMemcpy(unc.data(), d_unc, unc.size() * 4, hipMemcpyDeviceToHost));   // (one member: nothing was written)
  if (depth) HIPCHECK(hipMemcpy(u16.data(), d_u16, u16.size() * 2, hipMemcpyDeviceToHost));
  if (depth) HIPCHECK(hipMemcpy(flags.data(), d_flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (picture) HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
  char head[64];
  if (!write_file(prefix + ".f32", nullptr, pred.data(), pred.size() * 4)) return 1;
  if (B > 1 && !write_file(prefix + ".unc.f32", nullptr, unc.data(), unc.size() * 4)) return 1;
  if (depth) {
    std::vector<uint8_t> be(2 * n_out);   // PGM's 16-bit samples: most significant byte first
    for (size_t j = 0; j < n_out; ++j) {
      be[2 * j] = (uint8_t)(u16[j] >> 8);
      be[2 * j + 1] = (uint8_t)(u16[j] & 0xff);
    }
    snprintf(head, sizeof(head), "P5\n%d %d\n65535\n", ow, oh);
    if (!write_file(prefix + ".pgm", head, be.data(), be.size())) return 1;
  }
  if (picture) {
    snprintf(head, sizeof(head), "P6\n%d %d\n255\n", ow, oh);
    if (!write_file(prefix + ".ppm", head, pic.data(), pic.size())) return 1;
  }
  double sum = 0;
  for (float v : pred) sum += v;
  int degenerate = 0;
  for (int v : flags) degenerate += v;
  printf("%s map %dx%dx%d from %d tiles written, mean %.6f%s%s; degenerate tiles: %d; device memory %.1f MB\n", depth ? "depth" : "normals", C, oh, ow, n,
         sum / (double)pred.size(), B > 1 ? "; uncertainty" : "", picture ? "; picture" : "", degenerate, mg_model_device_bytes(m) / 1e6);
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_u16));
  HIPCHECK(hipFree(d_pic));
  HIPCHECK(hipFree(d_flags));
  if (d_lut) HIPCHECK(hipFree(d_lut));
  mg_model_destroy(m);
  return 0;
}
