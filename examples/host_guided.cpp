// Edge-guided upsampling from a C host: a depth or normals prediction at the model's size, enlarged to the picture's size by joint
// bilateral upsampling against the picture itself - pipe(image, guided_upsample=dict(radius=R, sigma=s)) of the Python pipelines as
// four calls of libmarigold_hip.so (include/marigold_hip.h), composed by the host because guided output is no out_mode of the one-call
// predictions:
//     mg_model_predict          the ensembled map at the decoded size, unclipped
//     mg_resize (uint8)         the picture's planes brought to that size: the low-resolution guide
//     mg_guided_upsample        the map enlarged to Hin x Win
//     mg_depth_visualize | mg_normals_finish   the pipelines' output stage: the clip, the 16-bit depth, the picture
// Build (gfx950 box):  hipcc -O2 examples/host_guided.cpp -Iinclude -Lmarigold_amd -lmarigold_hip -Wl,-rpath,$PWD/marigold_amd -o host_guided
// Run:                 ./host_guided model.mgimg image.u8 Hin Win seed out_prefix [radius sigma [table.lut]]
//   image.u8          raw uint8 [Hin][Win][3] (what PIL holds); resampled (bilinear) to the model's size when it differs
//   radius sigma      of mg_guided_upsample; default 2 and 0.1
//   table.lut         768 bytes, the colour map's 256 x RGB table (marigold_amd.image.export_color_table); depth: no table, no .ppm
//   out_prefix.f32    raw fp32 [channels][Hin][Win], clipped to [0, 1] (depth) / [-1, 1] (normals)
//   out_prefix.pgm    depth: 16-bit binary PGM (big endian), uint16(depth * 65535)
//   out_prefix.ppm    the picture, binary PPM
// The Python pipelines give the same arrays and pictures, bit for bit, with generator=marigold_amd.NativeNoise(seed)
// (tests/test_gpu_guided_pipeline.py builds and runs this program and compares).  The uncertainty of an ensemble is not guided and
// not written here (examples/host_picture.cpp writes it).
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
  if (argc != 7 && argc != 9 && argc != 10) {
    fprintf(stderr, "usage: %s model.mgimg image.u8 Hin Win seed out_prefix [radius sigma [table.lut]]\n", argv[0]);
    return 2;
  }
  const int Hin = atoi(argv[3]), Win = atoi(argv[4]);
  const uint64_t seed = strtoull(argv[5], nullptr, 0);
  if (Hin <= 0 || Win <= 0) {
    fprintf(stderr, "bad image size %s x %s\n", argv[3], argv[4]);
    return 2;
  }
  const int radius = argc >= 9 ? atoi(argv[7]) : 2;
  const float sigma = argc >= 9 ? (float)atof(argv[8]) : 0.1f;
  mg_model* m = mg_model_load(argv[1], 0);
  if (!m) {
    fprintf(stderr, "mg_model_load: %s\n", mg_last_error());
    return 1;
  }
  int cfg[MG_CFG_WORDS];
  CHECK(mg_model_info(m, cfg));
  const int H = cfg[MG_CFG_HEIGHT], W = cfg[MG_CFG_WIDTH], C = cfg[MG_CFG_CHANNELS], post = cfg[MG_CFG_POST];
  const int h = cfg[MG_CFG_OUT_H], w = cfg[MG_CFG_OUT_W];   // the decoded size: the prediction's
  if (post != MG_POST_DEPTH && post != MG_POST_NORMALS) {
    fprintf(stderr, "a depth or normals model image is expected\n");
    return 2;
  }
  const bool depth = post == MG_POST_DEPTH;
  const size_t n_in = (size_t)Hin * Win, n_lo = (size_t)h * w;
  std::vector<uint8_t> bytes(3 * n_in), planes(3 * n_in);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    fprintf(stderr, "cannot read %zu bytes from %s\n", bytes.size(), argv[2]);
    return 1;
  }
  fclose(f);
  for (size_t p = 0; p < n_in; ++p)   // mg_resize reads planes; every call below takes the picture as [3][Hin][Win]
    for (int c = 0; c < 3; ++c) planes[c * n_in + p] = bytes[3 * p + c];
  uint8_t* d_lut = nullptr;
  if (argc == 10) {
    uint8_t table[768];
    f = fopen(argv[9], "rb");
    if (!f || fread(table, 1, sizeof(table), f) != sizeof(table)) {
      fprintf(stderr, "cannot read the 768 bytes of a colour table from %s\n", argv[9]);
      return 1;
    }
    fclose(f);
    HIPCHECK(hipMalloc(&d_lut, sizeof(table)));
    HIPCHECK(hipMemcpy(d_lut, table, sizeof(table), hipMemcpyHostToDevice));
  }
  const bool picture = depth ? d_lut != nullptr : true;
  uint8_t *d_rgb, *d_lo, *d_pic;
  uint16_t* d_u16;
  float *d_pred, *d_unc, *d_tmp, *d_out;
  HIPCHECK(hipMalloc(&d_rgb, planes.size()));
  HIPCHECK(hipMalloc(&d_lo, 3 * n_lo));
  HIPCHECK(hipMalloc(&d_tmp, (size_t)3 * Hin * w * 4));
  HIPCHECK(hipMalloc(&d_pred, C * n_lo * 4));
  HIPCHECK(hipMalloc(&d_unc, n_lo * 4));
  HIPCHECK(hipMalloc(&d_out, C * n_in * 4));
  HIPCHECK(hipMalloc(&d_u16, n_in * 2));
  HIPCHECK(hipMalloc(&d_pic, 3 * n_in));
  hipStream_t s;
  HIPCHECK(hipStreamCreate(&s));
  HIPCHECK(hipMemcpy(d_rgb, planes.data(), planes.size(), hipMemcpyHostToDevice));
  // 1. the prediction; the pipelines' input stage multiplies by fp32(1 / 255) after a resample on the device and divides otherwise
  const int reciprocal = Hin != H || Win != W;
  double info[4];
  CHECK(mg_model_predict(m, d_rgb, 0, Hin, Win, 0, reciprocal, seed, nullptr, d_pred, d_unc, info, s));
  // 2. the low-resolution guide (a picture of the prediction's size is its own)
  const uint8_t* guide_lo = d_rgb;
  if (Hin != h || Win != w) {
    CHECK(mg_resize(d_rgb, d_lo, d_tmp, 3, Hin, Win, h, w, 0, 1, s));
    guide_lo = d_lo;
  }
  // 3. the enlargement, 4. the output stage, clipping in place
  CHECK(mg_guided_upsample(d_pred, C, h, w, guide_lo, d_rgb, 0, Hin, Win, radius, sigma, d_out, s));
  if (depth) CHECK(mg_depth_visualize(d_out, d_lut, (int64_t)n_in, d_out, d_u16, picture ? d_pic : nullptr, s));
  else CHECK(mg_normals_finish(d_out, Hin, Win, d_out, d_pic, s));
  HIPCHECK(hipStreamSynchronize(s));
  std::vector<float> pred(C * n_in);
  HIPCHECK(hipMemcpy(pred.data(), d_out, pred.size() * 4, hipMemcpyDeviceToHost));
  const std::string prefix = argv[6];
  if (!write_file(prefix + ".f32", nullptr, pred.data(), pred.size() * 4)) return 1;
  char head[64];
  if (depth) {
    std::vector<uint16_t> u16(n_in);
    HIPCHECK(hipMemcpy(u16.data(), d_u16, u16.size() * 2, hipMemcpyDeviceToHost));
    std::vector<uint8_t> be(2 * n_in);   // PGM's 16-bit samples: most significant byte first
    for (size_t i = 0; i < n_in; ++i) {
      be[2 * i] = (uint8_t)(u16[i] >> 8);
      be[2 * i + 1] = (uint8_t)(u16[i] & 0xff);
    }
    snprintf(head, sizeof(head), "P5\n%d %d\n65535\n", Win, Hin);
    if (!write_file(prefix + ".pgm", head, be.data(), be.size())) return 1;
  }
  if (picture) {
    std::vector<uint8_t> pic(3 * n_in);
    HIPCHECK(hipMemcpy(pic.data(), d_pic, pic.size(), hipMemcpyDeviceToHost));
    snprintf(head, sizeof(head), "P6\n%d %d\n255\n", Win, Hin);
    if (!write_file(prefix + ".ppm", head, pic.data(), pic.size())) return 1;
  }
  double sum = 0;
  for (float v : pred) sum += v;
  printf("%s map %dx%dx%d from %dx%d, guided with radius %d and sigma %g, mean %.6f%s\n", depth ? "depth" : "normals", C, Hin, Win, h, w, radius,
         (double)sigma, sum / pred.size(), picture ? "; picture" : "");
  HIPCHECK(hipFree(d_rgb));
  HIPCHECK(hipFree(d_lo));
  HIPCHECK(hipFree(d_tmp));
  HIPCHECK(hipFree(d_pred));
  HIPCHECK(hipFree(d_unc));
  HIPCHECK(hipFree(d_out));
  HIPCHECK(hipFree(d_u16));
  HIPCHECK(hipFree(d_pic));
  if (d_lut) HIPCHECK(hipFree(d_lut));
  mg_model_destroy(m);
  return 0;
}
