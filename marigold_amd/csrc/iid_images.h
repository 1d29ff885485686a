// The two images of an intrinsic-image score as every score kernel sees them (evalscore.hip: PSNR, SSIM; lpips.hip: the first
// convolution's staging and the range count): gamma, the (s, q) brightness mapping of MG_OP_IIDSCORE_PREP and the mask are applied
// on every load - nothing mapped is ever stored - and the part of the MG_OP_IIDSCORE_* workspace layout that both files address.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.h"

constexpr int EV_BLOCKS = 512;    // rows of a partial table
constexpr int EV_THREADS = 256;
constexpr int II_N = 5;           // S p*g, S p*p, valid elements, brightness pixels, NaN brightness values

// head of the workspace layout of the MG_OP_IIDSCORE_* ops (bytes); the rest is evalscore.hip's
constexpr size_t WS_II_PART = 0;
constexpr size_t WS_II_STATE = WS_II_PART + (size_t)EV_BLOCKS * II_N * 8;   // SelState
constexpr size_t WS_II_MAP = WS_II_STATE + 64;                              // IidMap: survives from PREP to the score ops

// what PREP leaves for the score kernels: pred <- clamp(q * (s * pred), 0, 1), gt <- clamp(q * gt, 0, 1)
struct IidMap {
  float s, q;
};

// the conversions of script/iid/eval.py:166-174 in fp32: bit 0 = x^2.2 (a target scored in linear space), bit 1 = x^(1/2.2) (Hypersim
// albedo); both = one after the other, in that order
__device__ __forceinline__ float iid_gamma(float x, int mode) {
  if (mode & 1) x = powf(x, 2.2f);
  if (mode & 2) x = powf(x, (float)(1.0 / 2.2));
  return x;
}

// the two images as the scores see them: recomputed from (s, q) on every load, never stored
struct IidImages {
  const float *pred, *gt;
  const uint8_t* mask;   // [3][HW] | NULL
  const IidMap* map;     // NULL: a plain target
  int gamma;
  __device__ __forceinline__ bool valid(long long e) const { return !mask || mask[e]; }
  __device__ __forceinline__ void load(long long e, float s, float q, float& p, float& g) const {
    p = iid_gamma(pred[e], gamma);
    g = iid_gamma(gt[e], gamma);
    if (map) {
      p = clip_keep_nan(q * (s * p), 0.f, 1.f);
      g = clip_keep_nan(q * g, 0.f, 1.f);
    }
  }
  // element e of one image alone (which = 0: the prediction, 1: the ground truth): the same operations as load(), the same bits
  __device__ __forceinline__ float load_one(long long e, float s, float q, int which) const {
    float x = iid_gamma(which ? gt[e] : pred[e], gamma);
    if (map) x = clip_keep_nan(which ? q * x : q * (s * x), 0.f, 1.f);
    return x;
  }
};
