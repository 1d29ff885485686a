// Module-level entry points: a MODEL IMAGE (marigold_amd/image.py::export_model_image - the pipeline's three native programs
// for one problem shape, their kernel-ready weights and a memory plan) loaded and run from C, no Python at run time.
// These are the seams the reference's single_infer calls (marigold/marigold_depth_pipeline.py:396-477):
//   mg_model_vae_encode  = encode_rgb            (:479-496: vae.encoder -> quant_conv -> mean -> x 0.18215)
//   mg_model_denoise     = the T-step loop       (:455-468: unet(cat(rgb_latent, x), t, ctx) + scheduler.step, all steps)
//   mg_model_vae_decode  = decode_depth / _normals (:498-516 + :473-475: post_quant_conv -> decoder -> channel mean / clip / shift)
// File layout (little endian; written by image.py with struct.pack - the two sides are kept in step by tests/test_host.py):
//   header "MGIMG1", version, ABI, counts, cfg[16] | buffer table | program table (+ named slots) | blobs (64-byte aligned)
// Version 2 holds several CONFIGURATIONS (problem shapes) of one model: header | configurations, scratch region | configuration
// table (cfg[16] + three programs each) | buffer table | blobs.  The packed weights are stored once (kind 3, shared); every other
// buffer names its configuration.  A handle = the shared weights (reference-counted: mg_model_replica makes another handle over
// them) + a private arena; mg_model_select picks the configuration the entry points act on.  A version-1 file is one configuration.
// Version 3 is version 2 with the TINY autoencoder (csrc/tinyvae.hip) where the AutoencoderKL programs stand, cfg[14] = 1: the two VAE
// entries of a configuration hold no ops, only named slots (rgb, latent, ws | latent, pred, ws - all scratch of that configuration); behind
// the buffer table lies one table more, the members of struct mg_tiny_vae as (shared buffer, byte offset).  The encode and decode
// stages of such an image are mg_tiny_vae_encode / mg_tiny_vae_decode on those slots.
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "common.h"

extern "C" int mg_ens_align_minimize(const mg_op* reg_op, void* stream, int E, int affine, int reduction, double lam, const double* mean,
                                     const double* C, float* st_host, const float* mm_host, double* x, double gtol, int maxiter,
                                     double* fval, int* nit, int* nfev, int* status);

namespace {

#pragma pack(push, 1)
struct ImgHeader {
  char magic[8];
  uint32_t version, abi, n_buffers, n_programs;
  uint32_t cfg[16];   // B, H, W, h, w, steps, prediction channels, post, step noises, sizeof(mg_op), modalities, Hout, Wout,
                      // pictures per call (0 = 1: images written before the field; B is then the members of EACH picture)
                      // (version 2: the words of configuration 0)
};
struct ImgBuffer {
  uint64_t nbytes, file_off;   // file_off of a version-2 scratch buffer: its place in the scratch region
  uint32_t kind, cfg;          // 0 scratch, 1 zeroed state, 2 data (constants; version 1: weights too), 3 shared (the weights of a
                               // version-2 image, stored once); cfg: the configuration a version-2 buffer of kind 0..2 belongs to
};
struct ImgSlot {
  char name[24];
  uint32_t buf, pad;
  uint64_t off, nbytes;
};
struct ImgProgram {
  char name[32];
  uint32_t n_ops, n_relocs;
  uint64_t ops_off, relocs_off;
  uint32_t n_slots, pad;
  ImgSlot slots[16];
};
struct ImgReloc {
  uint32_t op, slot, buf, pad;
  uint64_t off;
};
struct ImgV2 {   // version 2, after the header; then the configuration table, then the buffer table
  uint32_t n_configs, pad;
  uint64_t scratch_bytes;   // the scratch region: the largest configuration's scratch
};
struct ImgConfig {
  uint32_t cfg[16];
  ImgProgram prog[3];
};
struct ImgTinyMember {   // version 3, after the buffer table: one per pointer of struct mg_tiny_vae, in the struct's order
  uint32_t buf, pad;     // buf 0xffffffff: a NULL member (the bias of a bias-free layer)
  uint64_t off;
};
#pragma pack(pop)

enum { VAE_KL = 0, VAE_TINY = 1 };   // cfg[14]
constexpr int TINY_MEMBERS = (int)(sizeof(mg_tiny_vae) / sizeof(void*));
constexpr int TINY_HALF = 4 + 2 * MG_TINY_VAE_LAYERS;
constexpr uint32_t TINY_ABSENT = 0xffffffffu;
static_assert(TINY_MEMBERS == 2 * TINY_HALF && sizeof(mg_tiny_vae) == TINY_MEMBERS * sizeof(void*), "mg_tiny_vae: two halves of pointers");

// Member k of struct mg_tiny_vae (in_w, in_b, w[33], b[33], out_w, out_b of the encoder, then of the decoder): the bytes its layout
// implies (include/marigold_hip.h), and whether it is the bias of a bias-free layer (encoder 3, 13, 23, decoder 9, 19, 29: NULL)
uint64_t tiny_member_bytes(int k, bool* absent) {
  const int half = k / TINY_HALF, j = k % TINY_HALF, cin = half ? 4 : 3, plain = half ? 9 : 3;
  *absent = false;
  if (j == 0) return 9ull * cin * 64 * 4;
  if (j == 1) return 64 * 4;
  if (j < 2 + MG_TINY_VAE_LAYERS) return 9ull * 64 * 64 * 2;
  if (j < 2 + 2 * MG_TINY_VAE_LAYERS) {
    const int l = j - 2 - MG_TINY_VAE_LAYERS;
    *absent = l >= plain && (l - plain) % 10 == 0;
    return 64 * 4;
  }
  return j == TINY_HALF - 2 ? 9ull * 64 * 4 * 4 : 4 * 4;
}

uint32_t ceil8(uint32_t n) {   // the tiny encoder's latent size: a ceiling per stride-2 layer
  for (int k = 0; k < 3; ++k) n = (n - 1) / 2 + 1;
  return n;
}

enum { KIND_SCRATCH = 0, KIND_ZERO = 1, KIND_DATA = 2, KIND_SHARED = 3 };

// What the file says, parsed and checked once on the host; a handle and its replicas read it, nobody writes it after the load.
struct PlanBuf {
  uint64_t nbytes, file_off;
  uint32_t kind, cfg;
  bool shared;    // lies in the shared weights (else in the handle's private arena)
  uint64_t off;   // its place there
};
struct PlanProg {
  std::string name;
  std::vector<mg_op> ops;   // device pointers still null
  std::vector<ImgReloc> rel;
  std::vector<ImgSlot> slots;
  const ImgSlot* slot(const char* n) const {
    for (const ImgSlot& s : slots)
      if (strnlen(s.name, sizeof(s.name)) == strlen(n) && memcmp(s.name, n, strlen(n)) == 0) return &s;
    return nullptr;
  }
};
struct PlanConfig {
  uint32_t cfg[16];
  PlanProg prog[3];
};
struct Plan {
  uint32_t version = 1;
  bool tiny = false;                   // version 3: the VAE stages are the tiny autoencoder's calls
  ImgTinyMember tiny_net[TINY_MEMBERS] = {};   // (checked by parse_image)
  std::vector<PlanBuf> bufs;
  std::vector<PlanConfig> cfgs;
  uint64_t shared_bytes = 0, private_bytes = 0;
};

// The weights every handle over one image reads: freed with the last handle (std::shared_ptr counts, thread-safe)
struct SharedMem {
  char* base = nullptr;
  bool host_only = false;
  ~SharedMem() {
    if (base && !host_only) (void)hipFree(base);
  }
};

struct Slot {
  std::string name;
  char* ptr;
  uint64_t nbytes;
};
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
  const uint32_t* cfg = nullptr;   // the plan's 16 words
  Prog enc, den, dec;
  int K = 1;                       // pictures per call (cfg[13], 0 = 1)
};

}  // namespace

struct mg_model {
  std::shared_ptr<const Plan> plan;
  std::shared_ptr<SharedMem> shared;   // the shared weights (a version-1 image: none)
  bool host_only = false;
  int device = -1;
  char* arena = nullptr;       // the handle's private allocation: every configuration's constants and zeroed state, then ONE scratch
                               // region every configuration's scratch is laid over (host-only: a fake base address, never touched)
  uint64_t arena_bytes = 0;
  std::vector<char*> bufs;
  std::vector<Config> configs;
  mg_tiny_vae tiny_net = {};   // a tiny image: the network in the shared weights
  int sel = 0;                 // the selected configuration: what every entry point below acts on
  const Config& cur() const { return configs[sel]; }
  void* predict_tmp = nullptr;       // the one-call predictions' input resampling temporary (fp32 [3][Hin][W], one picture's: the
                                     // pictures of a call pass through it one after the other), grown on demand
  uint64_t predict_tmp_bytes = 0;
  void* out_tmp = nullptr;           // the one-call predictions' output temporaries (see out_tmp_layout), grown on demand
  uint64_t out_tmp_bytes = 0;
  void* seq_latent = nullptr;        // image sequences: the denoised latent of the frame before (the bytes of the x slot), allocated at the
                                     // first mg_model_predict_next
  uint64_t seq_bytes = 0;
  bool seq_carried = false;          // seq_latent holds a frame of the selected configuration
  const float* seq_call = nullptr;   // the strength, while mg_model_predict_next runs its prediction on this handle
  void* tiled_tmp = nullptr;         // mg_model_predict_tiled's temporaries (see TiledTmp), grown on demand
  uint64_t tiled_tmp_bytes = 0;
};

namespace {

bool read_at(FILE* f, uint64_t off, void* dst, size_t n) {
  return fseek(f, (long)off, SEEK_SET) == 0 && fread(dst, 1, n, f) == n;
}

uint64_t r256(uint64_t b) { return (b + 255) / 256 * 256; }

// May configuration `c` point into buffer `b`?  Its own buffers and the shared weights only.
bool owns(const Plan& p, uint32_t c, uint32_t b) { return p.version == 1 || p.bufs[b].kind == KIND_SHARED || p.bufs[b].cfg == c; }

int parse_program(FILE* f, uint64_t file_bytes, const ImgProgram& ip, const Plan& p, uint32_t c, bool no_ops, PlanProg* out) {
  out->name = std::string(ip.name, strnlen(ip.name, sizeof(ip.name)));
  const char* nm = out->name.c_str();
  MG_REQUIRE((no_ops ? ip.n_ops == 0 && ip.n_relocs == 0 : ip.n_ops > 0) && ip.n_slots <= 16, "mg_model_load: corrupt program table (%s)", nm);
  MG_REQUIRE(ip.ops_off <= file_bytes && (uint64_t)ip.n_ops * sizeof(mg_op) <= file_bytes - ip.ops_off &&
                 ip.relocs_off <= file_bytes && (uint64_t)ip.n_relocs * sizeof(ImgReloc) <= file_bytes - ip.relocs_off,
             "mg_model_load: corrupt image - the ops or relocations of %s lie outside the %llu-byte file", nm, (unsigned long long)file_bytes);
  out->ops.resize(ip.n_ops);
  MG_REQUIRE(ip.n_ops == 0 || read_at(f, ip.ops_off, out->ops.data(), sizeof(mg_op) * ip.n_ops), "mg_model_load: short read (ops of %s)", nm);
  out->rel.resize(ip.n_relocs);
  MG_REQUIRE(ip.n_relocs == 0 || read_at(f, ip.relocs_off, out->rel.data(), sizeof(ImgReloc) * ip.n_relocs),
             "mg_model_load: short read (relocations of %s)", nm);
  for (const ImgReloc& r : out->rel) {
    MG_REQUIRE(r.op < ip.n_ops && r.buf < p.bufs.size(), "mg_model_load: relocation out of range (%s)", nm);
    MG_REQUIRE(owns(p, c, r.buf), "mg_model_load: corrupt image - a relocation of %s (configuration %u) points into buffer %u of configuration %u",
               nm, c, r.buf, p.bufs[r.buf].cfg);
    MG_REQUIRE(r.off < p.bufs[r.buf].nbytes, "mg_model_load: corrupt image - a relocation of %s points %llu bytes into buffer %u of %llu bytes",
               nm, (unsigned long long)r.off, r.buf, (unsigned long long)p.bufs[r.buf].nbytes);
    // (slot 100: the address pair of MG_OP_IGEMM's row-statistics tickets)
    MG_REQUIRE(r.slot < 16 || (r.slot == 100 && out->ops[r.op].kind == MG_OP_IGEMM), "mg_model_load: unknown relocation slot %u", r.slot);
  }
  for (uint32_t k = 0; k < ip.n_slots; ++k) {
    const ImgSlot& s = ip.slots[k];
    MG_REQUIRE(s.buf < p.bufs.size(), "mg_model_load: slot out of range (%s)", nm);
    MG_REQUIRE(owns(p, c, s.buf), "mg_model_load: corrupt image - slot %u of %s (configuration %u) lies in buffer %u of configuration %u", k, nm, c,
               s.buf, p.bufs[s.buf].cfg);
    MG_REQUIRE(s.off <= p.bufs[s.buf].nbytes && s.nbytes <= p.bufs[s.buf].nbytes - s.off,
               "mg_model_load: corrupt image - slot %u of %s spans [%llu, +%llu) of a %llu-byte buffer", k, nm, (unsigned long long)s.off,
               (unsigned long long)s.nbytes, (unsigned long long)p.bufs[s.buf].nbytes);
    out->slots.push_back(s);
  }
  return 0;
}

// The whole file but the stored bytes of the buffers, checked: nothing below touches a device.
int parse_image(FILE* f, Plan* p) {
  ImgHeader h;
  MG_REQUIRE(read_at(f, 0, &h, sizeof(ImgHeader)), "mg_model_load: short read (header)");
  MG_REQUIRE(memcmp(h.magic, "MGIMG1\0\0", 8) == 0 && h.version >= 1 && h.version <= 3, "mg_model_load: not a model image (or an unknown version)");
  MG_REQUIRE(h.abi == MG_ABI_VERSION && h.cfg[9] == sizeof(mg_op),
             "mg_model_load: the image was written for ABI %u / %u-byte ops, this library is ABI %d / %zu", h.abi, h.cfg[9], MG_ABI_VERSION, sizeof(mg_op));
  p->version = h.version;
  p->tiny = h.version == 3;
  const bool multi = h.version >= 2;   // the layout of several configurations
  ImgV2 v2 = {1, 0, 0};
  if (multi) {
    MG_REQUIRE(read_at(f, sizeof(ImgHeader), &v2, sizeof(ImgV2)), "mg_model_load: short read (header)");
    MG_REQUIRE(v2.n_configs >= 1 && v2.n_configs <= 4096 && v2.scratch_bytes < (1ull << 40), "mg_model_load: corrupt header");
  }
  MG_REQUIRE(h.n_programs == 3 * v2.n_configs && h.n_buffers > 0 && h.n_buffers < (1u << 24), "mg_model_load: corrupt header");
  // the file's own size bounds every stored buffer (a truncated / corrupt table must not size a staging buffer or a copy)
  MG_REQUIRE(fseek(f, 0, SEEK_END) == 0, "mg_model_load: cannot seek");
  const long fsz = ftell(f);
  MG_REQUIRE(fsz > 0, "mg_model_load: cannot size the image");
  const uint64_t file_bytes = (uint64_t)fsz;
  // version 1: header | buffer table | three programs; version 2: header | ImgV2 | configuration table | buffer table
  std::vector<ImgConfig> ct(v2.n_configs);
  uint64_t buf_at = sizeof(ImgHeader);
  if (multi) {
    MG_REQUIRE(read_at(f, sizeof(ImgHeader) + sizeof(ImgV2), ct.data(), sizeof(ImgConfig) * v2.n_configs),
               "mg_model_load: short read (configuration table)");
    buf_at += sizeof(ImgV2) + sizeof(ImgConfig) * v2.n_configs;
  }
  std::vector<ImgBuffer> bt(h.n_buffers);
  MG_REQUIRE(read_at(f, buf_at, bt.data(), sizeof(ImgBuffer) * h.n_buffers), "mg_model_load: short read (buffer table)");
  if (h.version == 1) {
    memcpy(ct[0].cfg, h.cfg, sizeof(h.cfg));
    MG_REQUIRE(read_at(f, buf_at + sizeof(ImgBuffer) * h.n_buffers, ct[0].prog, sizeof(ImgProgram) * 3), "mg_model_load: short read (program table)");
  }
  // ---- the buffers and where a handle places them.  Version 1: everything in the private arena, in the table's order.  Version 2:
  // the shared weights in an allocation of their own; in the arena every configuration's constants and zeroed state, then the scratch
  // region, where a configuration's scratch buffers lie at the offsets the file gives them (configurations never run at the same time
  // on one handle, and no program reads scratch it has not written: tests/test_gpu_scratch_independence.py)
  p->bufs.resize(h.n_buffers);
  std::vector<uint64_t> scratch_end(v2.n_configs, 0);
  uint64_t shared = 0, priv = 0;
  for (uint32_t i = 0; i < h.n_buffers; ++i) {
    const ImgBuffer& b = bt[i];
    MG_REQUIRE(b.nbytes > 0 && b.nbytes < (1ull << 40), "mg_model_load: corrupt image - buffer %u has %llu bytes", i, (unsigned long long)b.nbytes);
    MG_REQUIRE(b.kind <= (multi ? KIND_SHARED : KIND_DATA), "mg_model_load: corrupt image - buffer %u is of unknown kind %u", i, b.kind);
    if (b.kind == KIND_DATA || b.kind == KIND_SHARED)
      MG_REQUIRE(b.file_off <= file_bytes && b.nbytes <= file_bytes - b.file_off,
                 "mg_model_load: corrupt image - buffer %u lies at [%llu, +%llu) of a %llu-byte file", i, (unsigned long long)b.file_off,
                 (unsigned long long)b.nbytes, (unsigned long long)file_bytes);
    PlanBuf& pb = p->bufs[i];
    pb.nbytes = b.nbytes;
    pb.file_off = b.file_off;
    pb.kind = b.kind;
    pb.cfg = multi && b.kind != KIND_SHARED ? b.cfg : 0;
    pb.shared = b.kind == KIND_SHARED;
    MG_REQUIRE(pb.cfg < v2.n_configs, "mg_model_load: corrupt image - buffer %u belongs to configuration %u of %u", i, pb.cfg, v2.n_configs);
    if (pb.shared) {
      pb.off = shared;
      shared += r256(b.nbytes);
    } else if (h.version == 1 || b.kind != KIND_SCRATCH) {
      pb.off = priv;
      priv += r256(b.nbytes);
    }
  }
  if (multi) {
    for (uint32_t i = 0; i < h.n_buffers; ++i) {
      PlanBuf& pb = p->bufs[i];
      if (pb.kind != KIND_SCRATCH) continue;
      // (in the table a configuration's scratch buffers come in the order of their places: they cannot overlap each other)
      MG_REQUIRE(pb.file_off % 256 == 0 && pb.file_off >= scratch_end[pb.cfg] && pb.file_off <= v2.scratch_bytes &&
                     pb.nbytes <= v2.scratch_bytes - pb.file_off,
                 "mg_model_load: corrupt image - scratch buffer %u of configuration %u lies at [%llu, +%llu) of a scratch region of %llu bytes", i,
                 pb.cfg, (unsigned long long)pb.file_off, (unsigned long long)pb.nbytes, (unsigned long long)v2.scratch_bytes);
      scratch_end[pb.cfg] = pb.file_off + pb.nbytes;
      pb.off = priv + pb.file_off;
    }
    priv += r256(v2.scratch_bytes);
  }
  p->shared_bytes = shared;
  p->private_bytes = priv;
  // ---- version 3: the tiny network, every member inside a shared buffer with the bytes its layout implies
  if (p->tiny) {
    MG_REQUIRE(read_at(f, buf_at + sizeof(ImgBuffer) * h.n_buffers, p->tiny_net, sizeof(p->tiny_net)), "mg_model_load: short read (tiny VAE table)");
    for (int k = 0; k < TINY_MEMBERS; ++k) {
      const ImgTinyMember& t = p->tiny_net[k];
      bool absent;
      const uint64_t need = tiny_member_bytes(k, &absent);
      MG_REQUIRE((t.buf == TINY_ABSENT) == absent,
                 "mg_model_load: corrupt image - member %d of the tiny VAE is %s (the bias-free layers are encoder 3, 13, 23 and decoder 9, 19, 29)", k,
                 absent ? "present where the layer has no bias" : "absent");
      if (absent) continue;
      MG_REQUIRE(t.buf < h.n_buffers && p->bufs[t.buf].kind == KIND_SHARED, "mg_model_load: corrupt image - member %d of the tiny VAE names buffer %u, not a shared one",
                 k, t.buf);
      MG_REQUIRE(t.off % 16 == 0, "mg_model_load: corrupt image - member %d of the tiny VAE lies at byte %llu of its buffer, not 16-byte aligned", k,
                 (unsigned long long)t.off);
      MG_REQUIRE(t.off <= p->bufs[t.buf].nbytes && need <= p->bufs[t.buf].nbytes - t.off,
                 "mg_model_load: corrupt image - member %d of the tiny VAE spans [%llu, +%llu) of a %llu-byte buffer", k, (unsigned long long)t.off,
                 (unsigned long long)need, (unsigned long long)p->bufs[t.buf].nbytes);
    }
  }
  // ---- the configurations
  p->cfgs.resize(v2.n_configs);
  static const char* const want[3] = {"vae.encode", "denoise", "vae.decode"};
  for (uint32_t c = 0; c < v2.n_configs; ++c) {
    PlanConfig& pc = p->cfgs[c];
    memcpy(pc.cfg, ct[c].cfg, sizeof(pc.cfg));
    MG_REQUIRE(pc.cfg[9] == sizeof(mg_op), "mg_model_load: configuration %u was written for %u-byte ops, this library has %zu", c, pc.cfg[9], sizeof(mg_op));
    for (int k = 0; k < 3; ++k) {
      if (int rc = parse_program(f, file_bytes, ct[c].prog[k], *p, c, p->tiny && k != 1, &pc.prog[k])) return rc;
      MG_REQUIRE(pc.prog[k].name == want[k], "mg_model_load: program %d is '%s', expected '%s'", k, pc.prog[k].name.c_str(), want[k]);
    }
    const ImgSlot *e_in = pc.prog[0].slot("rgb"), *e_out = pc.prog[0].slot("latent"), *rl = pc.prog[1].slot("rgb_latent"), *xs = pc.prog[1].slot("x");
    const ImgSlot *d_in = pc.prog[2].slot("latent"), *d_out = pc.prog[2].slot("pred");
    MG_REQUIRE(e_in && e_out && rl && xs && d_in && d_out, "mg_model_load: a program lacks its input / output slots");
    // the three programs hand K pictures of B members on to each other: [K,3,H,W] -> [K,4,h,w]; [K B,...] -> the decoder -> [K B,C,Ho,Wo]
    const uint32_t* g = pc.cfg;
    const uint64_t K = g[13] ? g[13] : 1;
    MG_REQUIRE(K < (1u << 20) && e_in->nbytes == K * 3 * g[1] * g[2] * 4 && e_out->nbytes == rl->nbytes && xs->nbytes == d_in->nbytes &&
                   xs->nbytes % (4 * K) == 0 && d_out->nbytes == K * g[0] * g[6] * g[11] * g[12] * 4,
               "mg_model_load: the image's slots do not chain for %d picture(s) of %u member(s) per call", (int)K, g[0]);
    MG_REQUIRE(g[14] == (p->tiny ? VAE_TINY : VAE_KL), "mg_model_load: configuration %u names VAE %u in cfg[14]: a version-%u image carries %s", c, g[14],
               h.version, p->tiny ? "the tiny autoencoder (1)" : "an AutoencoderKL (0)");
    if (p->tiny) {
      // the calls' arguments: K pictures [K,3,H,W] -> [K,4,h,w] (a ceiling per stride-2 layer); K B n members [.,4,h,w] -> [.,C,8h,8w]
      const uint64_t n = g[10], members = K * g[0] * n, cpred = g[7] == MG_POST_DEPTH ? 1 : 3;
      MG_REQUIRE(g[1] >= 1 && g[2] >= 1 && g[1] <= (1u << 16) && g[2] <= (1u << 16) && g[0] >= 1 && n >= 1 && members < (1u << 20) &&
                     (g[7] == MG_POST_NONE || g[7] == MG_POST_DEPTH || g[7] == MG_POST_NORMALS || g[7] == MG_POST_UNIT) &&
                     g[3] == ceil8(g[1]) && g[4] == ceil8(g[2]) && g[11] == 8 * g[3] && g[12] == 8 * g[4] && g[6] == cpred * n &&
                     e_out->nbytes == K * 4 * g[3] * g[4] * 4 && d_in->nbytes == members * 4 * g[3] * g[4] * 4,
                 "mg_model_load: the image's slots do not chain for %d picture(s) of %u member(s) through the tiny VAE (%u x %u -> latent %u x %u -> %u x %u)",
                 (int)K, g[0], g[1], g[2], g[3], g[4], g[11], g[12]);
      const ImgSlot *e_ws = pc.prog[0].slot("ws"), *d_ws = pc.prog[2].slot("ws");
      MG_REQUIRE(e_ws && d_ws, "mg_model_load: a tiny VAE entry lacks its workspace slot");
      const long long e_need = mg_tiny_vae_workspace_bytes(0, (int)K, (int)g[1], (int)g[2]);
      const long long d_need = mg_tiny_vae_workspace_bytes(1, (int)members, (int)g[3], (int)g[4]);
      MG_REQUIRE(e_need > 0 && d_need > 0, "mg_model_load: configuration %u is beyond the tiny VAE's sizes (%s)", c, mg_last_error());
      MG_REQUIRE(e_ws->nbytes >= (uint64_t)e_need && d_ws->nbytes >= (uint64_t)d_need,
                 "mg_model_load: corrupt image - the tiny VAE's workspaces of configuration %u hold %llu and %llu bytes, the calls need %lld and %lld", c,
                 (unsigned long long)e_ws->nbytes, (unsigned long long)d_ws->nbytes, e_need, d_need);
      // every slot of the two entries is scratch of this configuration, 16-byte aligned (buffers lie on 256-byte boundaries)
      for (int k = 0; k < 3; k += 2)
        for (const ImgSlot& sl : pc.prog[k].slots)
          MG_REQUIRE(p->bufs[sl.buf].kind == KIND_SCRATCH && sl.off % 16 == 0, "mg_model_load: corrupt image - slot %.24s of %s is not aligned scratch",
                     sl.name, pc.prog[k].name.c_str());
    }
  }
  return 0;
}

// The handle's buffers are placed (m->arena, m->shared): their addresses, then every configuration's programs patched to them
int instantiate(mg_model* m) {
  const Plan& p = *m->plan;
  m->bufs.resize(p.bufs.size());
  for (size_t i = 0; i < p.bufs.size(); ++i) m->bufs[i] = (p.bufs[i].shared ? m->shared->base : m->arena) + p.bufs[i].off;
  if (p.tiny) {
    const void** member = (const void**)&m->tiny_net;
    for (int k = 0; k < TINY_MEMBERS; ++k) member[k] = p.tiny_net[k].buf == TINY_ABSENT ? nullptr : m->bufs[p.tiny_net[k].buf] + p.tiny_net[k].off;
  }
  m->configs.resize(p.cfgs.size());
  for (size_t c = 0; c < p.cfgs.size(); ++c) {
    Config& cf = m->configs[c];
    cf.cfg = p.cfgs[c].cfg;
    cf.K = cf.cfg[13] ? (int)cf.cfg[13] : 1;
    Prog* dst[3] = {&cf.enc, &cf.den, &cf.dec};
    for (int k = 0; k < 3; ++k) {
      const PlanProg& pp = p.cfgs[c].prog[k];
      std::vector<mg_op> ops = pp.ops;
      for (const ImgReloc& r : pp.rel) {   // (checked by parse_program)
        char* q = m->bufs[r.buf] + r.off;
        if (r.slot < 16) {
          ops[r.op].p[r.slot] = q;
        } else {
          const uint64_t a = (uint64_t)(uintptr_t)q;
          ops[r.op].i[MG_IGEMM_I_TICKETS_LO] = (int32_t)(uint32_t)(a & 0xffffffffu);
          ops[r.op].i[MG_IGEMM_I_TICKETS_HI] = (int32_t)(uint32_t)(a >> 32);
        }
      }
      dst[k]->name = pp.name;
      if (!ops.empty()) {   // (a tiny image's VAE entries: slots only)
        dst[k]->prog = mg_program_create(ops.data(), (int)ops.size());
        MG_REQUIRE(dst[k]->prog, "mg_model_load: mg_program_create failed (%s)", pp.name.c_str());
      }
      for (const ImgSlot& s : pp.slots)
        dst[k]->slots.push_back(Slot{std::string(s.name, strnlen(s.name, sizeof(s.name))), m->bufs[s.buf] + s.off, s.nbytes});
    }
  }
  return 0;
}

// Fake addresses of a host-only handle, for the contract checks only (nothing is dereferenced): the shared weights at 4 GiB, every
// handle's arena in a 1 TiB window of its own
char* fake_arena() {
  static std::atomic<uint64_t> n{0};
  return (char*)(uintptr_t)((2 + n.fetch_add(1)) << 40);
}

// The private arena of a handle whose plan and shared weights are set: allocated, its zeroed state zeroed; its constants from the
// file (f) or, a replica's, from `parent` device to device; scratch as allocated.
int make_arena(mg_model* m, FILE* f, const mg_model* parent) {
  const Plan& p = *m->plan;
  m->arena_bytes = p.private_bytes;
  if (m->host_only) {
    m->arena = fake_arena();
    return 0;
  }
  MG_CHECK_HIP(hipMalloc((void**)&m->arena, p.private_bytes ? p.private_bytes : 256));
  std::vector<char> stage;
  for (size_t i = 0; i < p.bufs.size(); ++i) {
    const PlanBuf& b = p.bufs[i];
    if (b.shared) continue;
    char* dst = m->arena + b.off;
    if (b.kind == KIND_DATA && parent) {
      MG_CHECK_HIP(hipMemcpy(dst, parent->arena + b.off, b.nbytes, hipMemcpyDeviceToDevice));
    } else if (b.kind == KIND_DATA) {
      stage.resize(b.nbytes);
      MG_REQUIRE(read_at(f, b.file_off, stage.data(), b.nbytes), "mg_model_load: short read (buffer %zu)", i);
      MG_CHECK_HIP(hipMemcpy(dst, stage.data(), b.nbytes, hipMemcpyHostToDevice));
    } else if (b.kind == KIND_ZERO) {
      MG_CHECK_HIP(hipMemset(dst, 0, b.nbytes));
    }
  }
  return 0;
}

int load_into(mg_model* m, FILE* f, int device) {
  auto plan = std::make_shared<Plan>();
  if (int rc = parse_image(f, plan.get())) return rc;
  m->plan = plan;
  m->host_only = device < 0;
  m->device = device;
  m->shared = std::make_shared<SharedMem>();
  m->shared->host_only = m->host_only;
  if (m->host_only) {
    m->shared->base = (char*)(uintptr_t)0x100000000ull;
  } else {
    MG_REQUIRE(mg_init(device) == 0, "mg_model_load: %s", mg_last_error());
    if (plan->shared_bytes) {
      MG_CHECK_HIP(hipMalloc((void**)&m->shared->base, plan->shared_bytes));
      std::vector<char> stage;
      for (size_t i = 0; i < plan->bufs.size(); ++i) {
        const PlanBuf& b = plan->bufs[i];
        if (!b.shared) continue;
        stage.resize(b.nbytes);
        MG_REQUIRE(read_at(f, b.file_off, stage.data(), b.nbytes), "mg_model_load: short read (buffer %zu)", i);
        MG_CHECK_HIP(hipMemcpy(m->shared->base + b.off, stage.data(), b.nbytes, hipMemcpyHostToDevice));
      }
    }
  }
  if (int rc = make_arena(m, f, nullptr)) return rc;
  return instantiate(m);
}

int replicate_into(mg_model* r, const mg_model* m) {
  r->plan = m->plan;
  r->shared = m->shared;
  r->host_only = m->host_only;
  r->device = m->device;
  r->sel = m->sel;
  if (!r->host_only) MG_REQUIRE(mg_init(r->device) == 0, "mg_model_replica: %s", mg_last_error());   // (binds the calling thread to the device)
  if (int rc = make_arena(r, nullptr, m)) return rc;
  return instantiate(r);
}

int copy_dd(void* dst, const void* src, uint64_t n, hipStream_t s) {
  MG_CHECK_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, s));
  return 0;
}

// The encode and the decode stage of the selected configuration, slot to slot on the caller's stream: the program of an AutoencoderKL
// image; the plain calls of a tiny one (mg_model_load checked their arguments against the slots) - all K B n members in ONE decode
int run_encode(const mg_model* m, void* stream) {
  const Config& c = m->cur();
  if (!m->plan->tiny) return mg_program_run(c.enc.prog, stream);
  const Slot* ws = c.enc.slot("ws");
  return mg_tiny_vae_encode(&m->tiny_net, (const float*)c.enc.slot("rgb")->ptr, (float*)c.enc.slot("latent")->ptr, c.K, (int)c.cfg[1], (int)c.cfg[2],
                            ws->ptr, (long long)ws->nbytes, stream);
}

int run_decode(const mg_model* m, void* stream) {
  const Config& c = m->cur();
  if (!m->plan->tiny) return mg_program_run(c.dec.prog, stream);
  const Slot* ws = c.dec.slot("ws");
  return mg_tiny_vae_decode(&m->tiny_net, (const float*)c.dec.slot("latent")->ptr, (float*)c.dec.slot("pred")->ptr,
                            c.K * (int)c.cfg[0] * (int)c.cfg[10], (int)c.cfg[3], (int)c.cfg[4], (int)c.cfg[7], ws->ptr, (long long)ws->nbytes, stream);
}

}  // namespace

extern "C" {

mg_model* mg_model_load(const char* path, int device) {
  if (!path) {
    mg_set_error("mg_model_load: null path");
    return nullptr;
  }
  FILE* f = fopen(path, "rb");
  if (!f) {
    mg_set_error("mg_model_load: cannot open %s", path);
    return nullptr;
  }
  mg_model* m = new mg_model();
  int rc;
  try {   // (std::vector / std::string allocations: nothing may unwind across the C boundary)
    rc = load_into(m, f, device);
  } catch (const std::exception& e) {
    mg_set_error("mg_model_load: %s while reading %s (corrupt image?)", e.what(), path);
    rc = 2;
  }
  fclose(f);
  if (rc) {
    mg_model_destroy(m);
    return nullptr;
  }
  return m;
}

mg_model* mg_model_replica(const mg_model* m) {
  if (!m) {
    mg_set_error("mg_model_replica: null model");
    return nullptr;
  }
  mg_model* r = new mg_model();
  int rc;
  try {
    rc = replicate_into(r, m);
  } catch (const std::exception& e) {
    mg_set_error("mg_model_replica: %s", e.what());
    rc = 2;
  }
  if (rc) {
    mg_model_destroy(r);
    return nullptr;
  }
  return r;
}

void mg_model_destroy(mg_model* m) {
  if (!m) return;
  for (Config& c : m->configs)
    for (Prog* p : {&c.enc, &c.den, &c.dec})
      if (p->prog) mg_program_destroy(p->prog);
  if (m->arena && !m->host_only) (void)hipFree(m->arena);
  if (m->predict_tmp) (void)hipFree(m->predict_tmp);
  if (m->out_tmp) (void)hipFree(m->out_tmp);
  if (m->seq_latent) (void)hipFree(m->seq_latent);
  if (m->tiled_tmp) (void)hipFree(m->tiled_tmp);
  delete m;   // (the shared weights go with the last handle over them)
}

int mg_model_info(const mg_model* m, int* cfg16) {
  MG_REQUIRE(m && cfg16, "mg_model_info: null argument");
  for (int i = 0; i < 16; ++i) cfg16[i] = (int)m->cur().cfg[i];
  return 0;
}

int mg_model_num_configs(const mg_model* m) { return m ? (int)m->configs.size() : 0; }

int mg_model_config_info(const mg_model* m, int index, int* cfg16) {
  MG_REQUIRE(m && cfg16, "mg_model_config_info: null argument");
  MG_REQUIRE(index >= 0 && index < (int)m->configs.size(), "mg_model_config_info: configuration %d of %d", index, (int)m->configs.size());
  for (int i = 0; i < 16; ++i) cfg16[i] = (int)m->configs[index].cfg[i];
  return 0;
}

int mg_model_find_config(const mg_model* m, int H, int W, int E, int steps, int K) {
  if (!m) {
    mg_set_error("mg_model_find_config: null model");
    return -1;
  }
  std::string have;
  for (size_t c = 0; c < m->configs.size(); ++c) {
    const uint32_t* g = m->configs[c].cfg;
    const int k = m->configs[c].K;
    if ((H < 0 || H == (int)g[1]) && (W < 0 || W == (int)g[2]) && (E < 0 || E == (int)g[0]) && (steps < 0 || steps == (int)g[5]) && (K < 0 || K == k))
      return (int)c;
    char one[96];
    snprintf(one, sizeof(one), "%s%u x %u (E %u, %u steps, K %d)", c ? ", " : "", g[1], g[2], g[0], g[5], k);
    if (have.size() < 600) have += one;
  }
  mg_set_error("mg_model_find_config: no configuration for %d x %d, E %d, %d steps, K %d (-1 = any); the image holds %s", H, W, E, steps, K, have.c_str());
  return -1;
}

int mg_model_select(mg_model* m, int index) {
  MG_REQUIRE(m, "mg_model_select: null model");
  MG_REQUIRE(index >= 0 && index < (int)m->configs.size(), "mg_model_select: configuration %d of %d", index, (int)m->configs.size());
  m->sel = index;
  m->seq_carried = false;   // a sequence does not outlive its configuration
  return 0;
}

int mg_processed_size(int Hin, int Win, int processing_res, int* H, int* W) {
  MG_REQUIRE(H && W && Hin > 0 && Win > 0 && processing_res >= 0, "mg_processed_size: bad arguments (%d x %d, processing_res %d)", Hin, Win, processing_res);
  *H = Hin;
  *W = Win;
  if (processing_res > 0) {   // util/image_util.py::max_res_size: Python's float arithmetic is this double arithmetic, int() truncates
    const double fw = (double)processing_res / (double)Win, fh = (double)processing_res / (double)Hin;
    const double factor = fw < fh ? fw : fh;
    *W = (int)((double)Win * factor);
    *H = (int)((double)Hin * factor);
  }
  return 0;
}

long long mg_model_device_bytes(const mg_model* m) { return m ? (long long)(m->arena_bytes + m->predict_tmp_bytes + m->out_tmp_bytes + m->seq_bytes + m->tiled_tmp_bytes) : 0; }

long long mg_model_shared_bytes(const mg_model* m) { return m ? (long long)m->plan->shared_bytes : 0; }

int mg_model_validate(mg_model* m) {
  MG_REQUIRE(m, "mg_model_validate: null model");
  const Config& c = m->cur();
  if (m->plan->tiny) {   // the tiny calls check every argument before their first launch; dry, they launch nothing
    g_dry_run = true;
    int rc = run_encode(m, nullptr);
    if (!rc) rc = run_decode(m, nullptr);
    g_dry_run = false;
    return rc ? rc : mg_program_validate(c.den.prog);
  }
  for (const Prog* p : {&c.enc, &c.den, &c.dec})
    if (int rc = mg_program_validate(p->prog)) return rc;
  return 0;
}

int mg_model_scratch_fill(mg_model* m, int byte, void* stream) {
  MG_REQUIRE(m && !m->host_only && byte >= 0 && byte <= 255, "mg_model_scratch_fill: bad arguments (or a host-only model)");
  const Plan& p = *m->plan;
  for (size_t i = 0; i < p.bufs.size(); ++i)   // (the configurations' scratch buffers overlay each other: some bytes are set twice)
    if (p.bufs[i].kind == KIND_SCRATCH) MG_CHECK_HIP(hipMemsetAsync(m->bufs[i], byte, p.bufs[i].nbytes, (hipStream_t)stream));
  // (the temporaries of a tiled prediction are scratch of the same kind: everything in them is written before it is read)
  if (m->tiled_tmp) MG_CHECK_HIP(hipMemsetAsync(m->tiled_tmp, byte, m->tiled_tmp_bytes, (hipStream_t)stream));
  return 0;
}

int mg_model_vae_encode(mg_model* m, const float* rgb, float* latent, void* stream) {
  MG_REQUIRE(m && !m->host_only && rgb && latent, "mg_model_vae_encode: bad arguments (or a host-only model)");
  const hipStream_t s = (hipStream_t)stream;
  const Config& c = m->cur();
  const Slot *in = c.enc.slot("rgb"), *out = c.enc.slot("latent");
  if (int rc = copy_dd(in->ptr, rgb, in->nbytes, s)) return rc;
  if (int rc = run_encode(m, stream)) return rc;
  return copy_dd(latent, out->ptr, out->nbytes, s);
}

int mg_model_denoise(mg_model* m, const float* rgb_latent, float* x, const float* step_noise, void* stream) {
  MG_REQUIRE(m && !m->host_only && rgb_latent && x, "mg_model_denoise: bad arguments (or a host-only model)");
  const hipStream_t s = (hipStream_t)stream;
  const Config& c = m->cur();
  const Slot *rl = c.den.slot("rgb_latent"), *xs = c.den.slot("x");
  if (int rc = copy_dd(rl->ptr, rgb_latent, rl->nbytes, s)) return rc;
  if (int rc = copy_dd(xs->ptr, x, xs->nbytes, s)) return rc;
  const int n_noise = (int)c.cfg[8];
  MG_REQUIRE(n_noise == 0 || step_noise, "mg_model_denoise: this scheduler draws noise in %d steps: pass [%d][B][C][h][w] floats", n_noise, n_noise);
  for (int k = 0; k < n_noise; ++k) {
    char nm[24];
    snprintf(nm, sizeof(nm), "noise%d", k);
    const Slot* ns = c.den.slot(nm);
    MG_REQUIRE(ns, "mg_model_denoise: the image lacks slot %s", nm);
    if (int rc = copy_dd(ns->ptr, (const char*)step_noise + (uint64_t)k * ns->nbytes, ns->nbytes, s)) return rc;
  }
  if (int rc = mg_program_run(c.den.prog, stream)) return rc;
  return copy_dd(x, xs->ptr, xs->nbytes, s);
}

int mg_model_vae_decode(mg_model* m, const float* latent, float* pred, void* stream) {
  MG_REQUIRE(m && !m->host_only && latent && pred, "mg_model_vae_decode: bad arguments (or a host-only model)");
  const hipStream_t s = (hipStream_t)stream;
  const Config& c = m->cur();
  const Slot *in = c.dec.slot("latent"), *out = c.dec.slot("pred");
  if (int rc = copy_dd(in->ptr, latent, in->nbytes, s)) return rc;
  if (int rc = run_decode(m, stream)) return rc;
  return copy_dd(pred, out->ptr, out->nbytes, s);
}

}  // extern "C"

// ---- ensemble_depth as one call (marigold/util/ensemble.py:39-196; the Python form: marigold_amd/ensemble.py::ensemble_depth) ----
namespace {
struct DevBuf {   // frees on every exit path
  void* p = nullptr;
  bool host = false;
  ~DevBuf() {
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
  }
};
mg_op make_median_op(const float* d, const float* st, float* med, float* mad, float* mm, void* scratch, int E, long long HW, int reduction,
                     int has_shift) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_ENS_DEPTH_MEDIAN;
  op.i[MG_ENS_DEPTH_MEDIAN_I_E] = E;
  op.i[MG_ENS_DEPTH_MEDIAN_I_REDUCTION] = reduction;
  op.i[MG_ENS_DEPTH_MEDIAN_I_HAS_SHIFT] = has_shift;
  op.p[MG_ENS_DEPTH_MEDIAN_P_D] = (void*)d;
  op.p[MG_ENS_DEPTH_MEDIAN_P_ST] = (void*)st;
  op.p[MG_ENS_DEPTH_MEDIAN_P_MED] = med;
  op.p[MG_ENS_DEPTH_MEDIAN_P_MAD] = mad;
  op.p[MG_ENS_DEPTH_MEDIAN_P_MINMAX] = mm;
  op.p[MG_ENS_DEPTH_MEDIAN_P_SCRATCH] = scratch;
  op.l[MG_ENS_DEPTH_MEDIAN_L_HW] = HW;
  return op;
}
}  // namespace

extern "C" int mg_ensemble_depth(const float* preds, int E, int H, int W, int scale_invariant, int shift_invariant, int reduction,
                                 double regularizer_strength, int max_iter, double tol, int max_res, float* depth_out, float* unc_out,
                                 double* info4, void* stream) {
  MG_REQUIRE(preds && depth_out && E >= 1 && H > 0 && W > 0, "ensemble_depth: bad arguments");
  MG_REQUIRE(reduction == 0 || reduction == 1, "Unrecognized reduction method: %d.", reduction);                    // ensemble.py:86-87
  MG_REQUIRE(scale_invariant || !shift_invariant, "Pure shift-invariant ensembling is not supported.");           // :88-89
  MG_REQUIRE(scale_invariant, "Unrecognized alignment.");                                                          // :189-190
  const hipStream_t s = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  const int affine = scale_invariant && shift_invariant;
  DevBuf scratch, st_dev, mm_dev;
  MG_CHECK_HIP(hipMalloc(&scratch.p, 12288));
  MG_CHECK_HIP(hipMalloc(&st_dev.p, sizeof(float) * 2 * E));
  MG_CHECK_HIP(hipMalloc(&mm_dev.p, sizeof(float) * (2 + 2 * E)));
  double fval = 0.0;
  int nit = 0, nfev = 0, status = 0;
  {
    // --- the alignment (compute_param, :154-173) on the members, down-sampled with nearest-exact beyond max_res (:158-161)
    const float* d_align = preds;
    int Ha = H, Wa = W;
    DevBuf small;
    if (max_res > 0 && (H > W ? H : W) > max_res) {
      const double f = (double)max_res / W < (double)max_res / H ? (double)max_res / W : (double)max_res / H;
      Ha = (int)(H * f);
      Wa = (int)(W * f);
      MG_CHECK_HIP(hipMalloc(&small.p, sizeof(float) * (size_t)E * Ha * Wa));
      if (int rc = mg_resize(preds, small.p, nullptr, E, H, W, Ha, Wa, /* nearest-exact */ 2, /* fp32 */ 0, stream)) return rc;
      d_align = (const float*)small.p;
    }
    const long long HWa = (long long)Ha * Wa;
    DevBuf sscratch, stats;
    MG_CHECK_HIP(hipMalloc(&sscratch.p, sizeof(double) * 128 * (size_t)E * (E + 3)));
    MG_CHECK_HIP(hipMalloc(&stats.p, sizeof(double) * (3 * (size_t)E + (size_t)E * E)));
    mg_op so;
    memset(&so, 0, sizeof(so));
    so.kind = MG_OP_ENS_DEPTH_STATS;
    so.i[MG_ENS_DEPTH_STATS_I_E] = E;
    so.p[MG_ENS_DEPTH_STATS_P_D] = (void*)d_align;
    so.p[MG_ENS_DEPTH_STATS_P_SCRATCH] = sscratch.p;
    so.p[MG_ENS_DEPTH_STATS_P_OUT] = stats.p;
    so.l[MG_ENS_DEPTH_STATS_L_HW] = HWa;
    if (int rc = mg_launch(&so, stream)) return rc;
    std::vector<double> hs(3 * (size_t)E + (size_t)E * E);
    MG_CHECK_HIP(hipMemcpyAsync(hs.data(), stats.p, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, s));
    MG_CHECK_HIP(hipStreamSynchronize(s));
    const double *dmin = hs.data(), *dmax = dmin + E, *mean = dmax + E, *C = mean + E;
    // init_param (:163-168): fp32 arithmetic, as the reference's torch ops
    const int n = affine ? 2 * E : E;
    std::vector<double> x(n), x0;
    for (int i = 0; i < E; ++i) {
      const float lo = (float)dmin[i], hi = (float)dmax[i];
      if (affine) {
        const float rng = hi - lo;
        const float sc = 1.0f / (rng < 1e-6f ? 1e-6f : rng);   // clamp(min=1e-6): a NaN range stays NaN, as in ensemble.py::init_param
        x[i] = (double)sc;
        x[E + i] = (double)(-sc * lo);
      } else {
        x[i] = (double)(1.0f / (hi < 1e-6f ? 1e-6f : hi));
      }
    }
    x0 = x;
    // the regulariser's device pass reads its 2E parameters from, and writes its 2 + 2E results to, host-mapped memory
    DevBuf st_host, mm_host;
    st_host.host = mm_host.host = true;
    MG_CHECK_HIP(hipHostMalloc(&st_host.p, sizeof(float) * 2 * E, hipHostMallocMapped));
    MG_CHECK_HIP(hipHostMalloc(&mm_host.p, sizeof(float) * (2 + 2 * E), hipHostMallocMapped));
    void *st_d = nullptr, *mm_d = nullptr;
    MG_CHECK_HIP(hipHostGetDevicePointer(&st_d, st_host.p, 0));
    MG_CHECK_HIP(hipHostGetDevicePointer(&mm_d, mm_host.p, 0));
    const mg_op reg = make_median_op(d_align, (const float*)st_d, nullptr, nullptr, (float*)mm_d, scratch.p, E, HWa, reduction, affine);
    if (int rc = mg_ens_align_minimize(&reg, stream, E, affine, reduction, regularizer_strength, mean, C, (float*)st_host.p,
                                       (const float*)mm_host.p, x.data(), tol, max_iter, &fval, &nit, &nfev, &status))
      return rc;
    bool finite = status != 3;
    for (double v : x) finite = finite && v == v && v - v == 0.0;
    if (!finite) x = x0;   // the optimiser ended on non-finite parameters: fall back to the starting point (as the Python form)
    std::vector<float> st(2 * (size_t)E, 0.f);
    for (int i = 0; i < E; ++i) {
      st[i] = (float)x[i];
      st[E + i] = affine ? (float)x[E + i] : 0.f;
    }
    MG_CHECK_HIP(hipMemcpyAsync(st_dev.p, st.data(), sizeof(float) * st.size(), hipMemcpyHostToDevice, s));
    MG_CHECK_HIP(hipStreamSynchronize(s));   // (st is a stack-lifetime host buffer)
  }
  // --- align -> lower-middle median (+ MAD) / mean (+ std) -> min / max normalisation (:175-194), all on the device
  const mg_op fin = make_median_op(preds, (const float*)st_dev.p, depth_out, unc_out, (float*)mm_dev.p, scratch.p, E, HW, reduction, affine);
  if (int rc = mg_launch(&fin, stream)) return rc;
  mg_op no;
  memset(&no, 0, sizeof(no));
  no.kind = MG_OP_ENS_DEPTH_NORM;
  no.i[MG_ENS_DEPTH_NORM_I_SHIFT_INVARIANT] = affine;
  no.p[MG_ENS_DEPTH_NORM_P_MED] = depth_out;
  no.p[MG_ENS_DEPTH_NORM_P_MAD] = unc_out;
  no.p[MG_ENS_DEPTH_NORM_P_MINMAX] = mm_dev.p;
  no.l[MG_ENS_DEPTH_NORM_L_HW] = HW;
  if (int rc = mg_launch(&no, stream)) return rc;
  MG_CHECK_HIP(hipStreamSynchronize(s));   // the temporaries above are freed on return
  if (info4) { info4[0] = fval; info4[1] = nfev; info4[2] = nit; info4[3] = status; }
  return 0;
}

// ---- the whole prediction as one call: bytes + seed -> ensembled map (__call__ of the reference's pipelines up to match_input_res:
// marigold/marigold_depth_pipeline.py:229-312, marigold_normals_pipeline.py:215-290; with fill_outputs for the intrinsic-image
// pipeline, marigold_iid_pipeline.py:239-411).  The stages hand their results on inside the model's own program slots; the members
// are ensembled straight out of the decode program's output slot.
namespace {

// A temporary of the model: at least `need` bytes behind *p, allocated at the first call that needs it, replaced when a later call
// needs more (mg_model_device_bytes counts *bytes, mg_model_destroy frees).
int grow_tmp(void** p, uint64_t* bytes, uint64_t need) {
  if (*bytes >= need) return 0;
  if (*p) MG_CHECK_HIP(hipFree(*p));   // (hipFree waits for the work that still uses it)
  *p = nullptr;
  *bytes = 0;
  MG_CHECK_HIP(hipMalloc(p, need));
  *bytes = need;
  return 0;
}

// Stages 1 to 5 of a one-call prediction, the same for every kind of model, for the n <= K pictures of one call: each picture into its
// row of the encoder's input, ONE encode, each picture's noise into its B rows (MG_OP_RANDN of its own seed: stream 0 = the initial
// latents, stream k + 1 = the LCM scheduler's step noise k - what its lone call draws), ONE denoise, ONE decode.  A call with n < K
// feeds picture n - 1 and its seed to the spare rows too, so that nothing in the programs reads what an earlier call left; the
// spare results are never read.  `who` names the entry point in the messages.  On return the K B members lie image-major in the
// decode program's output slot, *preds.  One picture per call is the n = K = 1 case.
int predict_members(mg_model* m, const char* who, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                    const uint64_t* seeds, void* stream, const float** preds) {
  const uint32_t* cfg = m->cur().cfg;
  const int K = m->cur().K, H = (int)cfg[1], W = (int)cfg[2], n_noise = (int)cfg[8];
  MG_REQUIRE(Hin > 0 && Win > 0, "%s: bad input size %d x %d", who, Hin, Win);
  const hipStream_t s = (hipStream_t)stream;
  const Slot *e_in = m->cur().enc.slot("rgb"), *e_out = m->cur().enc.slot("latent"), *rl = m->cur().den.slot("rgb_latent"), *xs = m->cur().den.slot("x");
  const Slot *d_in = m->cur().dec.slot("latent"), *d_out = m->cur().dec.slot("pred");
  // (mg_model_load checked that the slots chain)
  const uint64_t rgb_row = e_in->nbytes / K, x_rows = xs->nbytes / K;   // bytes per picture
  // 1. picture i -> [1,3,H,W] in [-1, 1], row i of the encoder's input slot
  float* tmp = nullptr;
  if (mode != 2 && Hin != H && Win != W) {
    if (int rc = grow_tmp(&m->predict_tmp, &m->predict_tmp_bytes, (uint64_t)3 * Hin * W * 4)) return rc;
    tmp = (float*)m->predict_tmp;
  }
  for (int i = 0; i < K; ++i)
    if (int rc = mg_rgb_prepare(rgb[i < n ? i : n - 1], hwc, Hin, Win, e_in->ptr + i * rgb_row, 0, H, W, mode, reciprocal, tmp, stream)) return rc;
  // 2. encode
  if (int rc = run_encode(m, stream)) return rc;
  if (int rc = copy_dd(rl->ptr, e_out->ptr, rl->nbytes, s)) return rc;
  // 3. the initial latents: stream 0; the LCM scheduler's step noises: stream k + 1
  for (int i = 0; i < K; ++i)
    if (int rc = mg_randn(seeds[i < n ? i : n - 1], 0, 0, (int64_t)(x_rows / 4), xs->ptr + i * x_rows, 0, stream)) return rc;
  // (mg_model_predict_next, K = 1) the frame before, member by member, into the initial latents
  if (m->seq_call && m->seq_carried)
    if (int rc = mg_latent_carry((float*)xs->ptr, (const float*)m->seq_latent, (int64_t)(xs->nbytes / 4), *m->seq_call, stream)) return rc;
  for (int k = 0; k < n_noise; ++k) {
    char nm[24];
    snprintf(nm, sizeof(nm), "noise%d", k);
    const Slot* ns = m->cur().den.slot(nm);
    MG_REQUIRE(ns && ns->nbytes == xs->nbytes, "%s: the image lacks slot %s", who, nm);
    for (int i = 0; i < K; ++i)
      if (int rc = mg_randn(seeds[i < n ? i : n - 1], (uint64_t)k + 1, 0, (int64_t)(x_rows / 4), ns->ptr + i * x_rows, 0, stream)) return rc;
  }
  // 4. denoise, 5. decode (an intrinsic-image model: the latent [B, 4 n, h, w] is the decoder's batch [B n, 4, h, w], the same bytes)
  if (int rc = mg_program_run(m->cur().den.prog, stream)) return rc;
  if (m->seq_call) {   // this frame's denoised latent, for the next one
    if (int rc = copy_dd(m->seq_latent, xs->ptr, xs->nbytes, s)) return rc;
    m->seq_carried = true;
  }
  if (int rc = copy_dd(d_in->ptr, xs->ptr, d_in->nbytes, s)) return rc;
  if (int rc = run_decode(m, stream)) return rc;
  *preds = (const float*)d_out->ptr;
  return 0;
}

}  // namespace

namespace {

// out_h / out_w / out_mode of an entry point's options (0 x 0: the decoded size; max_pixels 0: no bound) -> the size to store
int output_size(const char* who, int out_h, int out_w, int out_mode, long long max_pixels, int Ho, int Wo, int* oh, int* ow) {
  MG_REQUIRE((out_h == 0 && out_w == 0) || (out_h > 0 && out_w > 0 && (!max_pixels || (long long)out_h * out_w <= max_pixels)),
             "%s: bad output size %d x %d", who, out_h, out_w);
  MG_REQUIRE(out_mode >= 0 && out_mode <= 2, "%s: out_mode must be 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)", who);
  *oh = out_h ? out_h : Ho;
  *ow = out_w ? out_w : Wo;
  return 0;
}

// The output temporaries of a one-call prediction, carved out of the model's out_tmp in this order (each part rounded up to 256
// bytes): the ensembled map at the decoded size (several members AND a resize: the resize reads it), the resize's fp32 intermediate
// [planes][Ho][out_w] (modes 0 / 1 when both sizes change), the picture stage's workspace (intrinsic images: [n][MG_IID_VIS_PARTS]
// for a target that is linear and up to scale; depth and normals: none).
struct OutTmp {
  uint64_t ens = 0, rtmp = 0, ws = 0;
  uint64_t total() const { return ens + rtmp + ws; }
};
OutTmp out_tmp_layout(int B, int planes, int Ho, int Wo, int oh, int ow, int out_mode, uint64_t ws_bytes) {
  auto r256 = [](uint64_t b) { return (b + 255) / 256 * 256; };
  OutTmp t;
  const bool resize = oh != Ho || ow != Wo;
  if (resize && B > 1) t.ens = r256((uint64_t)planes * Ho * Wo * 4);
  if (resize && out_mode != 2 && oh != Ho && ow != Wo) t.rtmp = r256((uint64_t)planes * Ho * ow * 4);
  t.ws = r256(ws_bytes);
  return t;
}

// Stages 1 to 7 of a one-call prediction of n pictures: the members (predict_members), then for picture i, one after the other,
// 6. ensemble(i, members, dst) -> int: its B members in the decoder's output slot -> the ensembled map (one member: the pipelines
//    return it as it is, without an uncertainty, and `ensemble` is not called),
// 7. match_input_res (marigold_depth_pipeline.py:306-312, marigold_normals_pipeline.py:282-288, marigold_iid_pipeline.py:378-385):
//    the prediction only, [planes][Ho][Wo] -> row i of pred_out [n][planes][oh][ow],
// 8. finish(i, row i of pred_out) -> int: the entry point's output stage on what was stored.
// The temporaries serve the pictures in turn (the stream orders them).  *ws (may be null): the picture workspace of ws_bytes, valid
// until the model's next prediction.
template <class Ensemble, class Finish>
int predict_resized(mg_model* m, const char* who, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                    const uint64_t* seeds, int planes, int oh, int ow, int out_mode, uint64_t ws_bytes, float* pred_out, float** ws, void* stream,
                    Ensemble ensemble, Finish finish) {
  const int B = (int)m->cur().cfg[0], Ho = (int)m->cur().cfg[11], Wo = (int)m->cur().cfg[12];
  const bool resize = oh != Ho || ow != Wo;
  const OutTmp t = out_tmp_layout(B, planes, Ho, Wo, oh, ow, out_mode, ws_bytes);
  if (int rc = grow_tmp(&m->out_tmp, &m->out_tmp_bytes, t.total())) return rc;
  float* const ens = (float*)m->out_tmp;
  float* const rtmp = t.rtmp ? (float*)((char*)m->out_tmp + t.ens) : nullptr;
  if (ws) *ws = t.ws ? (float*)((char*)m->out_tmp + t.ens + t.rtmp) : nullptr;
  const float* all = nullptr;
  if (int rc = predict_members(m, who, n, rgb, hwc, Hin, Win, mode, reciprocal, seeds, stream, &all)) return rc;
  for (int i = 0; i < n; ++i) {
    const float* preds = all + (uint64_t)i * B * planes * Ho * Wo;
    float* const out = pred_out + (uint64_t)i * planes * oh * ow;
    const float* final_pred = preds;   // at the decoded size
    if (B > 1) {
      float* const dst = resize ? ens : out;
      if (int rc = ensemble(i, preds, dst)) return rc;
      final_pred = dst;
    }
    if (resize) {
      if (int rc = mg_resize(final_pred, out, rtmp, planes, Ho, Wo, oh, ow, out_mode, 0, stream)) return rc;
    } else if (B == 1) {
      if (int rc = copy_dd(out, preds, (uint64_t)planes * Ho * Wo * 4, (hipStream_t)stream)) return rc;
    }
    if (int rc = finish(i, out)) return rc;
  }
  return 0;
}

// Stages 1 to 8 of a depth / normals prediction of n pictures; unc_out [n][Ho][Wo], info4 [n][4], the pictures of the output stage
// (u16_out [n][oh][ow], picture_out [n][oh][ow][3]; `clip`: the output stage runs - mg_model_predict stores the map as it is)
int predict_depth_or_normals(mg_model* m, const char* who, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                             const uint64_t* seeds, const mg_predict_opts* opts_or_null, int oh, int ow, int out_mode, bool clip,
                             const uint8_t* lut256x3, float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null,
                             uint8_t* picture_out_or_null, double* info4_or_null, void* stream) {
  const uint32_t* cfg = m->cur().cfg;
  const int B = (int)cfg[0], C = (int)cfg[6], post = (int)cfg[7], Ho = (int)cfg[11], Wo = (int)cfg[12];
  static const mg_predict_opts defaults = MG_PREDICT_OPTS_DEFAULT;
  const mg_predict_opts& o = opts_or_null ? *opts_or_null : defaults;
  if (info4_or_null)
    for (int i = 0; i < 4 * n; ++i) info4_or_null[i] = 0.0;
  const uint64_t HWo = (uint64_t)Ho * Wo, hw = (uint64_t)oh * ow;
  return predict_resized(
      m, who, n, rgb, hwc, Hin, Win, mode, reciprocal, seeds, C, oh, ow, out_mode, 0, pred_out, nullptr, stream,
      [&](int i, const float* preds, float* dst) {
        float* const unc = unc_out_or_null ? unc_out_or_null + i * HWo : nullptr;
        if (post == MG_POST_DEPTH)
          return mg_ensemble_depth(preds, B, Ho, Wo, o.scale_invariant, o.shift_invariant, o.reduction, o.regularizer_strength, o.max_iter, o.tol,
                                   o.max_res, dst, unc, info4_or_null ? info4_or_null + 4 * i : nullptr, stream);
        MG_REQUIRE(o.normals_reduction == 0 || o.normals_reduction == 1, "Unrecognized reduction method: %d.", o.normals_reduction);
        return mg_ensemble_normals(preds, dst, unc, B, (int64_t)HWo, o.normals_reduction, stream);
      },
      // 8. the output stage on what was stored, in place: the clip (:314-316 / :294), the 16-bit depth (script/depth/run.py), the picture
      [&](int i, float* out) {
        if (!clip) return 0;
        uint8_t* const pic = picture_out_or_null ? picture_out_or_null + i * hw * 3 : nullptr;
        if (post == MG_POST_DEPTH)
          return mg_depth_visualize(out, lut256x3, (int64_t)hw, out, u16_out_or_null ? u16_out_or_null + i * hw : nullptr, pic, stream);
        return mg_normals_finish(out, oh, ow, out, pic, stream);
      });
}

// The output-option refusals of mg_model_predict_out, in `who`'s name, for a model of the kind (post, C) whose stitched or ensembled
// map is Ho x Wo -> the size to store
int check_output_opts(const char* who, int post, int C, const mg_output_opts& q, int Ho, int Wo, const uint16_t* u16_out_or_null,
                      const uint8_t* picture_out_or_null, int* oh, int* ow) {
  const bool depth = post == MG_POST_DEPTH && C == 1;
  MG_REQUIRE(depth || (post == MG_POST_NORMALS && C == 3), "%s: a depth or a normals image is required", who);
  if (int rc = output_size(who, q.out_h, q.out_w, q.out_mode, 1ll << 30, Ho, Wo, oh, ow)) return rc;
  if (depth) {
    MG_REQUIRE(!picture_out_or_null || q.lut256x3, "%s: the picture of a depth model needs out_opts.lut256x3 (the colour table)", who);
  } else {
    MG_REQUIRE(!u16_out_or_null && !q.lut256x3, "%s: u16_out and lut256x3 belong to a depth model, this one predicts normals", who);
  }
  return 0;
}

// mg_model_predict_out and mg_model_predict_many after their own argument checks: the refusals they share (in `who`'s name), then the
// prediction.  One picture is n = 1.
int predict_out_many(mg_model* m, const char* who, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                     const uint64_t* seeds, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out,
                     float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null, void* stream) {
  const uint32_t* cfg = m->cur().cfg;
  const int C = (int)cfg[6], post = (int)cfg[7];
  MG_REQUIRE(post != MG_POST_UNIT && cfg[10] == 1, "%s: an intrinsic-image model goes through mg_model_predict_iid", who);
  static const mg_output_opts out_defaults = MG_OUTPUT_OPTS_DEFAULT;
  const mg_output_opts& q = out_opts_or_null ? *out_opts_or_null : out_defaults;
  int oh, ow;
  if (int rc = check_output_opts(who, post, C, q, (int)cfg[11], (int)cfg[12], u16_out_or_null, picture_out_or_null, &oh, &ow)) return rc;
  return predict_depth_or_normals(m, who, n, rgb, hwc, Hin, Win, mode, reciprocal, seeds, opts_or_null, oh, ow, q.out_mode, true, q.lut256x3,
                                  pred_out, unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null, stream);
}

}  // namespace

// An image of several pictures per call runs through mg_model_predict_many only
#define MG_REQUIRE_ONE_PICTURE(m, who) \
  MG_REQUIRE((m)->cur().K == 1, who ": this image runs %d pictures per call: use mg_model_predict_many", (m)->cur().K)

extern "C" int mg_model_predict(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                const mg_predict_opts* opts_or_null, float* pred_out, float* unc_out_or_null, double* info4_or_null,
                                void* stream) {
  MG_REQUIRE(m && !m->host_only && rgb && pred_out, "mg_model_predict: bad arguments (or a host-only model)");
  MG_REQUIRE_ONE_PICTURE(m, "mg_model_predict");
  const uint32_t* cfg = m->cur().cfg;
  const int C = (int)cfg[6], post = (int)cfg[7];
  MG_REQUIRE(post != MG_POST_UNIT && cfg[10] == 1, "mg_model_predict: intrinsic-image models are not supported yet");
  MG_REQUIRE((post == MG_POST_DEPTH && C == 1) || (post == MG_POST_NORMALS && C == 3), "mg_model_predict: a depth or a normals image is required");
  // the map at the decoded size: no resize, no temporaries
  return predict_depth_or_normals(m, "mg_model_predict", 1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, opts_or_null, (int)cfg[11], (int)cfg[12], 0,
                                  false, nullptr, pred_out, unc_out_or_null, nullptr, nullptr, info4_or_null, stream);
}

extern "C" int mg_model_predict_out(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                    const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out,
                                    float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null,
                                    void* stream) {
  MG_REQUIRE(m && rgb && pred_out, "mg_model_predict_out: null argument (the model, the picture and pred_out are required)");
  MG_REQUIRE(!m->host_only, "mg_model_predict_out: a host-only model cannot predict (load it with device >= 0)");
  MG_REQUIRE_ONE_PICTURE(m, "mg_model_predict_out");
  return predict_out_many(m, "mg_model_predict_out", 1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, opts_or_null, out_opts_or_null, pred_out,
                          unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null, stream);
}

extern "C" int mg_model_seq_reset(mg_model* m) {
  MG_REQUIRE(m, "mg_model_seq_reset: null model");
  m->seq_carried = false;
  return 0;
}

extern "C" int mg_model_predict_next(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                     const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out,
                                     float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null,
                                     void* stream, float strength) {
  MG_REQUIRE(m && rgb && pred_out, "mg_model_predict_next: null argument (the model, the picture and pred_out are required)");
  MG_REQUIRE(!m->host_only, "mg_model_predict_next: a host-only model cannot predict (load it with device >= 0)");
  MG_REQUIRE(m->cur().K == 1, "mg_model_predict_next: this configuration runs %d pictures per call: a sequence runs one frame per call (K = 1)", m->cur().K);
  MG_REQUIRE(strength >= 0.f && strength <= 1.f, "mg_model_predict_next: strength %g is not in [0, 1]", (double)strength);
  const uint32_t* cfg = m->cur().cfg;
  MG_REQUIRE((int)cfg[7] != MG_POST_UNIT && cfg[10] == 1, "mg_model_predict_next: an intrinsic-image model goes through mg_model_predict_iid");
  const uint64_t need = m->cur().den.slot("x")->nbytes;
  if (m->seq_bytes < need) m->seq_carried = false;
  if (int rc = grow_tmp(&m->seq_latent, &m->seq_bytes, need)) return rc;
  m->seq_call = &strength;
  const int rc = predict_out_many(m, "mg_model_predict_next", 1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, opts_or_null, out_opts_or_null, pred_out,
                                  unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null, stream);
  m->seq_call = nullptr;
  if (rc) m->seq_carried = false;   // a frame that failed carries nothing on
  return rc;
}

extern "C" int mg_model_predict_many(mg_model* m, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                                     const uint64_t* seeds, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                                     float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                                     double* info4_or_null, void* stream) {
  MG_REQUIRE(m, "mg_model_predict_many: null model");
  MG_REQUIRE(!m->host_only, "mg_model_predict_many: a host-only model cannot predict (load it with device >= 0)");
  MG_REQUIRE(n >= 1 && n <= m->cur().K, "mg_model_predict_many: %d pictures for an image of %d per call (1 <= n <= %d)", n, m->cur().K, m->cur().K);
  MG_REQUIRE(rgb && seeds && pred_out, "mg_model_predict_many: null argument (the rgb and seeds arrays and pred_out are required)");
  for (int i = 0; i < n; ++i) MG_REQUIRE(rgb[i], "mg_model_predict_many: null picture %d of %d", i, n);
  return predict_out_many(m, "mg_model_predict_many", n, rgb, hwc, Hin, Win, mode, reciprocal, seeds, opts_or_null, out_opts_or_null, pred_out,
                          unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null, stream);
}

// ---- the tiled prediction of a large picture as one call (pipe.predict_tiled): plan -> guide -> tiles, a group of K per
// call of the tile configuration's programs -> fit and blend -> resize -> output stage.  Every stage is the code the calls above and
// csrc/tiles.hip already run; this function only strings them together.
namespace {

// mg_model_predict_tiled's temporaries, carved out of the model's tiled_tmp in this order, each part rounded up to 256 bytes
struct TiledTmp {
  uint64_t crops = 0, maps = 0, unc = 0, fit_ws = 0, coef = 0, coef_unc = 0, flags = 0, guide = 0, canvas = 0, rtmp = 0;
  uint64_t total() const { return crops + maps + unc + fit_ws + coef + coef_unc + flags + guide + canvas + rtmp; }
};

// the handle goes back to the configuration it was on, on every way out
struct Reselect {
  mg_model* m;
  int sel;
  ~Reselect() { m->sel = sel; }
};

}  // namespace

extern "C" int mg_model_predict_tiled(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                      const mg_tiled_opts* tiled, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                                      float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                                      double* info4_or_null, int* degenerate_or_null, void* stream) {
  const char* who = "mg_model_predict_tiled";
  MG_REQUIRE(m && rgb && tiled && pred_out, "%s: null argument (the model, the picture, tiled and pred_out are required)", who);
  const int n_cfg = (int)m->configs.size();
  MG_REQUIRE(tiled->tile_config >= 0 && tiled->tile_config < n_cfg, "%s: tile configuration %d of %d", who, tiled->tile_config, n_cfg);
  const Config& tc = m->configs[tiled->tile_config];
  const int B = (int)tc.cfg[0], th = (int)tc.cfg[1], tw = (int)tc.cfg[2], C = (int)tc.cfg[6], post = (int)tc.cfg[7], K = tc.K;
  MG_REQUIRE(post != MG_POST_UNIT && tc.cfg[10] == 1, "%s: an intrinsic-image model is not supported (depth and normals only)", who);
  const bool depth = post == MG_POST_DEPTH && C == 1;
  MG_REQUIRE(depth || (post == MG_POST_NORMALS && C == 3), "%s: a depth or a normals image is required", who);
  MG_REQUIRE(Hin >= 8 && Win >= 8 && Hin % 8 == 0 && Win % 8 == 0, "%s: the picture size %d x %d must be multiples of 8 (the call works at the picture's size)",
             who, Hin, Win);
  MG_REQUIRE((long long)Hin * Win <= (1ll << 28) && Hin <= 65535, "%s: a picture of %d x %d is not supported", who, Hin, Win);
  MG_REQUIRE(th % 8 == 0 && tw % 8 == 0 && (int)tc.cfg[11] == th && (int)tc.cfg[12] == tw && (long long)th * tw <= (1ll << 26),
             "%s: the tile configuration's size %d x %d (decoded %d x %d) must be multiples of 8, decoded at that size", who, th, tw, (int)tc.cfg[11],
             (int)tc.cfg[12]);
  MG_REQUIRE(th <= Hin && tw <= Win, "%s: the tile configuration's size %d x %d exceeds the picture %d x %d", who, th, tw, Hin, Win);
  // 1. the plan
  int ys[MG_TILE_MAX_PER_AXIS], xs[MG_TILE_MAX_PER_AXIS];
  const int ny = mg_tile_plan(Hin, th, tiled->overlap_y, ys, MG_TILE_MAX_PER_AXIS);
  const int nx = ny < 1 ? -1 : mg_tile_plan(Win, tw, tiled->overlap_x, xs, MG_TILE_MAX_PER_AXIS);
  if (nx < 1) {
    const std::string why = mg_last_error();
    mg_set_error("%s: %s", who, why.c_str());
    return 2;
  }
  const int n = ny * nx;
  MG_REQUIRE(n > 1, "%s: the plan is ONE tile (the picture is the tile): use mg_model_predict_out", who);
  int hg = 0, wg = 0;
  if (depth) {
    MG_REQUIRE(tiled->guide_config >= 0 && tiled->guide_config < n_cfg, "%s: guide configuration %d of %d", who, tiled->guide_config, n_cfg);
    const Config& gc = m->configs[tiled->guide_config];
    MG_REQUIRE(gc.K == 1, "%s: the guide configuration runs %d pictures per call, the guide is ONE picture (K = 1)", who, gc.K);
    MG_REQUIRE((int)gc.cfg[0] == B, "%s: the guide configuration has %d members, the tile configuration %d", who, (int)gc.cfg[0], B);
    MG_REQUIRE((int)gc.cfg[7] == post && (int)gc.cfg[6] == C && gc.cfg[10] == 1, "%s: the guide configuration is of another kind than the tile configuration", who);
    hg = (int)gc.cfg[11];
    wg = (int)gc.cfg[12];
    MG_REQUIRE(hg >= 1 && wg >= 1 && (long long)hg * wg <= (1ll << 26), "%s: bad guide size %d x %d", who, hg, wg);
  }
  // the short last group: r tiles, whole on a configuration of r pictures per call, or padded on the tile configuration
  const int r = n % K;
  const bool tail = r != 0 && tiled->tail_config != -1;
  if (tail) {
    MG_REQUIRE(tiled->tail_config >= 0 && tiled->tail_config < n_cfg, "%s: tail configuration %d of %d", who, tiled->tail_config, n_cfg);
    const Config& lc = m->configs[tiled->tail_config];
    MG_REQUIRE(lc.K == r, "%s: the tail configuration runs %d pictures per call, the short last group has %d tiles (%d tiles, %d per call)", who, lc.K,
               r, n, K);
    MG_REQUIRE((int)lc.cfg[0] == B && (int)lc.cfg[7] == post && (int)lc.cfg[6] == C && lc.cfg[10] == 1 && (int)lc.cfg[1] == th && (int)lc.cfg[2] == tw &&
                   (int)lc.cfg[11] == th && (int)lc.cfg[12] == tw,
               "%s: the tail configuration is of another kind, size (%d x %d) or member count (%d) than the tile configuration (%d x %d, %d)", who,
               (int)lc.cfg[1], (int)lc.cfg[2], (int)lc.cfg[0], th, tw, B);
  }
  static const mg_output_opts out_defaults = MG_OUTPUT_OPTS_DEFAULT;
  const mg_output_opts& q = out_opts_or_null ? *out_opts_or_null : out_defaults;
  int oh, ow;
  if (int rc = check_output_opts(who, post, C, q, Hin, Win, u16_out_or_null, picture_out_or_null, &oh, &ow)) return rc;
  MG_REQUIRE((uintptr_t)pred_out % 16 == 0 && (uintptr_t)unc_out_or_null % 16 == 0, "%s: pred_out and unc_out must be 16-byte aligned", who);
  MG_REQUIRE((uintptr_t)degenerate_or_null % 4 == 0, "%s: degenerate must be aligned to its elements", who);
  if (opts_or_null && !depth)
    MG_REQUIRE(opts_or_null->normals_reduction == 0 || opts_or_null->normals_reduction == 1, "%s: Unrecognized reduction method: %d.", who,
               opts_or_null->normals_reduction);
  MG_REQUIRE(!m->host_only, "%s: a host-only model cannot predict (load it with device >= 0)", who);

  // the temporaries
  auto r256 = [](uint64_t b) { return (b + 255) / 256 * 256; };
  const bool with_unc = B > 1 && unc_out_or_null, resize = oh != Hin || ow != Win;
  const uint64_t tile_px = (uint64_t)th * tw;
  TiledTmp t;
  t.crops = r256((uint64_t)K * 3 * tile_px);
  t.maps = r256((uint64_t)n * C * tile_px * 4);
  if (with_unc) t.unc = r256((uint64_t)n * tile_px * 4);
  if (depth) {
    t.fit_ws = r256((uint64_t)mg_tiles_workspace_bytes(n, th, tw));
    t.coef = r256((uint64_t)n * 16);
    if (with_unc) t.coef_unc = r256((uint64_t)n * 16);
    if (!degenerate_or_null) t.flags = r256((uint64_t)n * 4);
    t.guide = r256((uint64_t)hg * wg * 4);
  }
  if (resize) {
    t.canvas = r256((uint64_t)C * Hin * Win * 4);
    if (q.out_mode != 2 && oh != Hin && ow != Win) t.rtmp = r256((uint64_t)C * Hin * ow * 4);
  }
  if (int rc = grow_tmp(&m->tiled_tmp, &m->tiled_tmp_bytes, t.total())) return rc;
  char* at = (char*)m->tiled_tmp;
  auto carve = [&](uint64_t bytes) {
    char* p = bytes ? at : nullptr;
    at += bytes;
    return p;
  };
  uint8_t* const crops = (uint8_t*)carve(t.crops);
  float* const maps = (float*)carve(t.maps);
  float* const uncs = (float*)carve(t.unc);
  void* const fit_ws = carve(t.fit_ws);
  double* const coef = (double*)carve(t.coef);
  double* const coef_unc = (double*)carve(t.coef_unc);
  int* const own_flags = (int*)carve(t.flags);
  int* const flags = degenerate_or_null ? degenerate_or_null : own_flags;
  float* const guide = (float*)carve(t.guide);
  float* const canvas = resize ? (float*)carve(t.canvas) : pred_out;
  float* const rtmp = (float*)carve(t.rtmp);
  const hipStream_t s = (hipStream_t)stream;

  Reselect back = {m, m->sel};
  if (info4_or_null)
    for (int i = 0; i < 4; ++i) info4_or_null[i] = 0.0;
  // 2. the guide: one ordinary prediction of the whole picture at the guide configuration's size, clipped
  if (depth) {
    m->sel = tiled->guide_config;
    if (int rc = predict_depth_or_normals(m, who, 1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, opts_or_null, hg, wg, 0, true, nullptr, guide,
                                          nullptr, nullptr, nullptr, info4_or_null, stream))
      return rc;
  }
  // 3. the tiles, a group of K per call
  std::vector<const uint8_t*> pics((size_t)K);
  std::vector<uint64_t> seeds((size_t)K);
  for (int first = 0; first < n; first += K) {
    const int cnt = n - first < K ? n - first : K;
    m->sel = cnt < K && tail ? tiled->tail_config : tiled->tile_config;
    if (int rc = mg_tile_crop(rgb, hwc, Hin, Win, th, tw, ys, ny, xs, nx, first, cnt, crops, stream)) return rc;
    for (int i = 0; i < cnt; ++i) {
      pics[i] = crops + (uint64_t)i * 3 * tile_px;
      seeds[i] = seed + 1 + (uint64_t)(first + i);   // (mod 2^64)
    }
    if (int rc = predict_depth_or_normals(m, who, cnt, pics.data(), hwc, th, tw, 0, 1, seeds.data(), opts_or_null, th, tw, 0, true, nullptr,
                                          maps + (uint64_t)first * C * tile_px, with_unc ? uncs + (uint64_t)first * tile_px : nullptr, nullptr, nullptr,
                                          nullptr, stream))
      return rc;
  }
  // 4. the stitch
  const int oy = tiled->overlap_y, ox = tiled->overlap_x;
  if (depth) {
    if (int rc = mg_tile_fit(maps, th, tw, ys, ny, xs, nx, Hin, Win, guide, hg, wg, coef, flags, fit_ws, (long long)t.fit_ws, stream)) return rc;
    if (int rc = mg_tile_blend(maps, 1, th, tw, ys, ny, xs, nx, Hin, Win, oy, ox, coef, 0, canvas, stream)) return rc;
    if (with_unc) {   // (s_i, 0): the scales of the fit without its shifts
      MG_CHECK_HIP(hipMemsetAsync(coef_unc, 0, (size_t)n * 16, s));
      MG_CHECK_HIP(hipMemcpy2DAsync(coef_unc, 16, coef, 16, 8, (size_t)n, hipMemcpyDeviceToDevice, s));
      if (int rc = mg_tile_blend(uncs, 1, th, tw, ys, ny, xs, nx, Hin, Win, oy, ox, coef_unc, 0, unc_out_or_null, stream)) return rc;
    }
  } else {
    if (int rc = mg_tile_blend(maps, 3, th, tw, ys, ny, xs, nx, Hin, Win, oy, ox, nullptr, 1, canvas, stream)) return rc;
    if (with_unc)
      if (int rc = mg_tile_blend(uncs, 1, th, tw, ys, ny, xs, nx, Hin, Win, oy, ox, nullptr, 0, unc_out_or_null, stream)) return rc;
  }
  // 5. match_input_res, then the output stage of mg_model_predict_out on what was stored
  if (resize)
    if (int rc = mg_resize(canvas, pred_out, rtmp, C, Hin, Win, oh, ow, q.out_mode, 0, stream)) return rc;
  if (depth) return mg_depth_visualize(pred_out, q.lut256x3, (int64_t)oh * ow, pred_out, u16_out_or_null, picture_out_or_null, stream);
  return mg_normals_finish(pred_out, oh, ow, pred_out, picture_out_or_null, stream);
}

extern "C" int mg_model_predict_iid(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                    const mg_iid_opts* opts_or_null, float* pred_out, float* unc_out_or_null, uint8_t* pictures_out_or_null,
                                    void* stream) {
  MG_REQUIRE(m && !m->host_only && rgb && pred_out, "mg_model_predict_iid: bad arguments (or a host-only model)");
  MG_REQUIRE_ONE_PICTURE(m, "mg_model_predict_iid");
  const uint32_t* cfg = m->cur().cfg;
  const int B = (int)cfg[0], C = (int)cfg[6], post = (int)cfg[7], n_noise = (int)cfg[8], n = (int)cfg[10];
  const int Ho = (int)cfg[11], Wo = (int)cfg[12];
  MG_REQUIRE(post == MG_POST_UNIT && n >= 1 && C == 3 * n,
             "mg_model_predict_iid: an intrinsic-image model is required (a depth or a normals image goes through mg_model_predict)");
  // MarigoldIIDPipeline._check_inference_step (marigold_iid_pipeline.py:443-447) raises on the LCM scheduler: so does its C form
  MG_REQUIRE(n_noise == 0, "mg_model_predict_iid: This pipeline implementation does not support the LCMScheduler (the image draws noise in %d steps)", n_noise);
  static const mg_iid_opts defaults = MG_IID_OPTS_DEFAULT;
  const mg_iid_opts& o = opts_or_null ? *opts_or_null : defaults;
  MG_REQUIRE(o.reduction == 0 || o.reduction == 1, "mg_model_predict_iid: Unrecognized reduction method: %d.", o.reduction);
  int oh, ow;
  if (int rc = output_size("mg_model_predict_iid", o.out_h, o.out_w, o.out_mode, 0, Ho, Wo, &oh, &ow)) return rc;
  MG_REQUIRE(n <= 16 && !((unsigned)(o.linear_bits | o.up_to_scale_bits) >> n), "mg_model_predict_iid: a flag names a target beyond the %d of the model (at most 16)", n);
  const uint64_t ws_bytes = pictures_out_or_null && (o.linear_bits & o.up_to_scale_bits) ? (uint64_t)n * MG_IID_VIS_PARTS * 4 : 0;
  float* ws = nullptr;
  // 6. the ensemble is ensemble_iid (:369-375)
  return predict_resized(
      m, "mg_model_predict_iid", 1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, C, oh, ow, o.out_mode, ws_bytes, pred_out, &ws, stream,
      [&](int, const float* preds, float* dst) { return mg_ensemble_iid(preds, B, (int64_t)C * Ho * Wo, o.reduction, dst, unc_out_or_null, stream); },
      // 8. the pictures of what was stored (fill_outputs -> MarigoldIIDOutput.fill_entry, :117-136, :393-411)
      [&](int, float* out) {
        if (!pictures_out_or_null) return 0;
        return mg_iid_visualize(out, pictures_out_or_null, ws, n, oh, ow, o.linear_bits, o.up_to_scale_bits, stream);
      });
}
