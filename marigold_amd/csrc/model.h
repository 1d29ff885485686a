// What csrc/model.hip (the model image: its file format, loader and stage entry points) and csrc/predict.hip (the one-call
// predictions over a loaded image) share: the handle and the types it is made of.  Private to the two files.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.h"

namespace mg_image {

struct Plan;        // what the file says (model.hip)
struct SharedMem;   // the weights every handle over one image reads (model.hip)

// A configuration's 16 words (enum mg_cfg) as what they mean; K: the pictures per call, already 1 where the file says 0
struct Cfg { int B, H, W, h, w, steps, C, post, n_noise, n_mod, Ho, Wo, K, vae; };

struct Slot { std::string name; char* ptr; uint64_t nbytes; };
struct Prog {
  std::string name;
  mg_program* prog = nullptr;
  std::vector<Slot> slots;
  const Slot* slot(const char* n) const {
    for (const Slot& s : slots)
      if (s.name == n) return &s;
    return nullptr;
  }
};
struct Config {
  Cfg cfg;
  const uint32_t* words = nullptr;   // the plan's 16 words as the file has them (mg_model_info)
  Prog enc, den, dec;
};

inline uint64_t r256(uint64_t b) { return (b + 255) / 256 * 256; }

// A temporary of the handle: at least `need` bytes behind p after grow(need) - allocated at the first call that needs it, replaced
// when a later call needs more.  mg_model_device_bytes counts `bytes`; the handle's destruction frees.
struct Tmp {
  void* p = nullptr;
  uint64_t bytes = 0;
  Tmp() = default;
  Tmp(const Tmp&) = delete;
  ~Tmp() { (void)release(); }
  hipError_t release() {
    const hipError_t e = p ? hipFree(p) : hipSuccess;   // (hipFree waits for the work that still uses it)
    p = nullptr;
    bytes = 0;
    return e;
  }
  int grow(uint64_t need) {
    if (bytes >= need) return 0;
    MG_CHECK_HIP(release());
    MG_CHECK_HIP(hipMalloc(&p, need));
    bytes = need;
    return 0;
  }
};

// The parts of a temporary, asked for in ONE sequence that both sizes and carves it (lay_out): the sizing pass (base null) ends with
// `at` the total, each part rounded up to 256 bytes; the carving pass hands out the addresses.  A part of 0 bytes is null, no room.
struct Arena {
  char* base = nullptr;
  uint64_t at = 0;
  template <class T>
  void part(T** p, uint64_t part_bytes) {
    *p = base && part_bytes ? (T*)(base + at) : nullptr;
    at += r256(part_bytes);
  }
};
template <class Parts>
int lay_out(Tmp& t, Parts parts) {
  Arena sizes;
  parts(sizes);
  if (int rc = t.grow(sizes.at)) return rc;
  Arena carve = {(char*)t.p, 0};
  parts(carve);
  return 0;
}

enum { TMP_INPUT, TMP_OUTPUT, TMP_SEQUENCE, TMP_TILED, TMP_COUNT };

int copy_dd(void* dst, const void* src, uint64_t n, hipStream_t s);
int run_encode(const mg_model* m, void* stream);
int run_decode(const mg_model* m, void* stream);

}  // namespace mg_image

struct mg_model {
  std::shared_ptr<const mg_image::Plan> plan;
  std::shared_ptr<mg_image::SharedMem> shared;   // the shared weights (a version-1 image: none)
  bool host_only = false;
  int device = -1;
  char* arena = nullptr;       // the handle's private allocation: every configuration's constants and zeroed state, then ONE scratch
                               // region every configuration's scratch is laid over (host-only: a fake base address, never touched)
  uint64_t arena_bytes = 0;
  std::vector<char*> bufs;
  std::vector<mg_image::Config> configs;
  mg_tiny_vae tiny_net = {};   // a tiny image: the network in the shared weights
  int sel = 0;                 // the selected configuration: what every entry point acts on
  const mg_image::Config& cur() const { return configs[sel]; }
  // The temporaries, grown on demand.  TMP_INPUT: the one-call predictions' input resampling (fp32 [3][Hin][W]: the pictures of a call
  // pass through it in turn); TMP_OUTPUT: their output temporaries (predict_resized); TMP_SEQUENCE: the denoised latent of the frame
  // before (the bytes of the x slot; mg_model_predict_next); TMP_TILED: mg_model_predict_tiled's.
  mg_image::Tmp tmp[mg_image::TMP_COUNT];
  bool seq_carried = false;    // tmp[TMP_SEQUENCE] holds a frame of the selected configuration
};
