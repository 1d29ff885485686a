// The model image: its file format, loader, handle and stage entry points (csrc/predict.hip holds the one-call predictions over a
// loaded image; csrc/model.h what the two files share).  A MODEL IMAGE (marigold_amd/image.py::export_model_image - the pipeline's three native programs
// for one problem shape, their kernel-ready weights and a memory plan) is loaded and run from C, no Python at run time.
// These are the seams the reference's single_infer calls (marigold/marigold_depth_pipeline.py:396-477):
//   mg_model_vae_encode  = encode_rgb            (:479-496: vae.encoder -> quant_conv -> mean -> x 0.18215)
//   mg_model_denoise     = the T-step loop       (:455-468: unet(cat(rgb_latent, x), t, ctx) + scheduler.step, all steps)
//   mg_model_vae_decode  = decode_depth / _normals (:498-516 + :473-475: post_quant_conv -> decoder -> channel mean / clip / shift)
// File layout (little endian; written by image.py with struct.pack - the two sides are kept in step by tests/test_host.py):
//   header "MGIMG1", version, ABI, counts, the 16 configuration words (enum mg_cfg) | buffer table | program table (+ named slots) | blobs (64-byte aligned)
// Version 2 holds several CONFIGURATIONS (problem shapes) of one model: header | configurations, scratch region | configuration
// table (16 words + three programs each) | buffer table | blobs.  The packed weights are stored once (kind 3, shared); every other
// buffer names its configuration.  A handle = the shared weights (reference-counted: mg_model_replica makes another handle over
// them) + a private arena; mg_model_select picks the configuration the entry points act on.  A version-1 file is one configuration.
// Version 3 is version 2 with the TINY autoencoder (csrc/tinyvae.hip) where the AutoencoderKL programs stand, MG_CFG_VAE = MG_VAE_TINY: the two VAE
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

#include "model.h"

using namespace mg_image;

namespace {

#pragma pack(push, 1)
struct ImgHeader {
  char magic[8];
  uint32_t version, abi, n_buffers, n_programs;
  uint32_t cfg[MG_CFG_WORDS];   // enum mg_cfg (version 2: the words of configuration 0)
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
  uint32_t cfg[MG_CFG_WORDS];
  ImgProgram prog[3];
};
struct ImgTinyMember {   // version 3, after the buffer table: one per pointer of struct mg_tiny_vae, in the struct's order
  uint32_t buf, pad;     // buf 0xffffffff: a NULL member (the bias of a bias-free layer)
  uint64_t off;
};
#pragma pack(pop)

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
  uint32_t words[MG_CFG_WORDS];   // as the file has them
  Cfg cfg;
  PlanProg prog[3];
};

}  // namespace

struct mg_image::Plan {
  uint32_t version = 1;
  bool tiny = false;                   // version 3: the VAE stages are the tiny autoencoder's calls
  ImgTinyMember tiny_net[TINY_MEMBERS] = {};   // (checked by parse_image)
  std::vector<PlanBuf> bufs;
  std::vector<PlanConfig> cfgs;
  uint64_t shared_bytes = 0, private_bytes = 0;
};

// The weights every handle over one image reads: freed with the last handle (std::shared_ptr counts, thread-safe)
struct mg_image::SharedMem {
  char* base = nullptr;
  bool host_only = false;
  ~SharedMem() {
    if (base && !host_only) (void)hipFree(base);
  }
};

namespace {

bool read_at(FILE* f, uint64_t off, void* dst, size_t n) {
  return fseek(f, (long)off, SEEK_SET) == 0 && fread(dst, 1, n, f) == n;
}

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
  MG_REQUIRE(h.abi == MG_ABI_VERSION && h.cfg[MG_CFG_OP_BYTES] == sizeof(mg_op),
             "mg_model_load: the image was written for ABI %u / %u-byte ops, this library is ABI %d / %zu", h.abi, h.cfg[MG_CFG_OP_BYTES], MG_ABI_VERSION,
             sizeof(mg_op));
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
    memcpy(pc.words, ct[c].cfg, sizeof(pc.words));
    // THE place the words are read by position.  The checks below are made on them as the file has them (unsigned: a corrupt word must
    // not wrap into a plausible size); everything after the load reads pc.cfg
    const uint32_t* g = pc.words;
    const uint32_t B = g[MG_CFG_MEMBERS], H = g[MG_CFG_HEIGHT], W = g[MG_CFG_WIDTH], lh = g[MG_CFG_LATENT_H], lw = g[MG_CFG_LATENT_W];
    const uint32_t C = g[MG_CFG_CHANNELS], post = g[MG_CFG_POST], Ho = g[MG_CFG_OUT_H], Wo = g[MG_CFG_OUT_W], vae = g[MG_CFG_VAE];
    const uint64_t K = MG_CFG_PICTURES_OF(g), n = g[MG_CFG_MODALITIES];
    pc.cfg = Cfg{(int)B, (int)H,  (int)W,  (int)lh, (int)lw, (int)g[MG_CFG_STEPS], (int)C, (int)post, (int)g[MG_CFG_STEP_NOISES],
                 (int)n, (int)Ho, (int)Wo, (int)K,  (int)vae};
    MG_REQUIRE(g[MG_CFG_OP_BYTES] == sizeof(mg_op), "mg_model_load: configuration %u was written for %u-byte ops, this library has %zu", c,
               g[MG_CFG_OP_BYTES], sizeof(mg_op));
    for (int k = 0; k < 3; ++k) {
      if (int rc = parse_program(f, file_bytes, ct[c].prog[k], *p, c, p->tiny && k != 1, &pc.prog[k])) return rc;
      MG_REQUIRE(pc.prog[k].name == want[k], "mg_model_load: program %d is '%s', expected '%s'", k, pc.prog[k].name.c_str(), want[k]);
    }
    const ImgSlot *e_in = pc.prog[0].slot("rgb"), *e_out = pc.prog[0].slot("latent"), *rl = pc.prog[1].slot("rgb_latent"), *xs = pc.prog[1].slot("x");
    const ImgSlot *d_in = pc.prog[2].slot("latent"), *d_out = pc.prog[2].slot("pred");
    MG_REQUIRE(e_in && e_out && rl && xs && d_in && d_out, "mg_model_load: a program lacks its input / output slots");
    // the three programs hand K pictures of B members on to each other: [K,3,H,W] -> [K,4,h,w]; [K B,...] -> the decoder -> [K B,C,Ho,Wo]
    MG_REQUIRE(K < (1u << 20) && e_in->nbytes == K * 3 * H * W * 4 && e_out->nbytes == rl->nbytes && xs->nbytes == d_in->nbytes &&
                   xs->nbytes % (4 * K) == 0 && d_out->nbytes == K * B * C * Ho * Wo * 4,
               "mg_model_load: the image's slots do not chain for %d picture(s) of %u member(s) per call", (int)K, B);
    MG_REQUIRE(vae == (uint32_t)(p->tiny ? MG_VAE_TINY : MG_VAE_KL), "mg_model_load: configuration %u names VAE %u in cfg[14]: a version-%u image carries %s",
               c, vae, h.version, p->tiny ? "the tiny autoencoder (1)" : "an AutoencoderKL (0)");
    if (p->tiny) {
      // the calls' arguments: K pictures [K,3,H,W] -> [K,4,h,w] (a ceiling per stride-2 layer); K B n members [.,4,h,w] -> [.,C,8h,8w]
      const uint64_t members = K * B * n, cpred = post == MG_POST_DEPTH ? 1 : 3;
      MG_REQUIRE(H >= 1 && W >= 1 && H <= (1u << 16) && W <= (1u << 16) && B >= 1 && n >= 1 && members < (1u << 20) &&
                     (post == MG_POST_NONE || post == MG_POST_DEPTH || post == MG_POST_NORMALS || post == MG_POST_UNIT) && lh == ceil8(H) &&
                     lw == ceil8(W) && Ho == 8 * lh && Wo == 8 * lw && C == cpred * n && e_out->nbytes == K * 4 * lh * lw * 4 &&
                     d_in->nbytes == members * 4 * lh * lw * 4,
                 "mg_model_load: the image's slots do not chain for %d picture(s) of %u member(s) through the tiny VAE (%u x %u -> latent %u x %u -> %u x %u)",
                 (int)K, B, H, W, lh, lw, Ho, Wo);
      const ImgSlot *e_ws = pc.prog[0].slot("ws"), *d_ws = pc.prog[2].slot("ws");
      MG_REQUIRE(e_ws && d_ws, "mg_model_load: a tiny VAE entry lacks its workspace slot");
      const long long e_need = mg_tiny_vae_workspace_bytes(0, (int)K, (int)H, (int)W);
      const long long d_need = mg_tiny_vae_workspace_bytes(1, (int)members, (int)lh, (int)lw);
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
    cf.words = p.cfgs[c].words;
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

}  // namespace

int mg_image::copy_dd(void* dst, const void* src, uint64_t n, hipStream_t s) {
  MG_CHECK_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, s));
  return 0;
}

// The encode and the decode stage of the selected configuration, slot to slot on the caller's stream: the program of an AutoencoderKL
// image; the plain calls of a tiny one (mg_model_load checked their arguments against the slots) - all K B n members in ONE decode
int mg_image::run_encode(const mg_model* m, void* stream) {
  const Config& c = m->cur();
  if (!m->plan->tiny) return mg_program_run(c.enc.prog, stream);
  const Cfg& g = c.cfg;
  const Slot* ws = c.enc.slot("ws");
  return mg_tiny_vae_encode(&m->tiny_net, (const float*)c.enc.slot("rgb")->ptr, (float*)c.enc.slot("latent")->ptr, g.K, g.H, g.W, ws->ptr,
                            (long long)ws->nbytes, stream);
}

int mg_image::run_decode(const mg_model* m, void* stream) {
  const Config& c = m->cur();
  if (!m->plan->tiny) return mg_program_run(c.dec.prog, stream);
  const Cfg& g = c.cfg;
  const Slot* ws = c.dec.slot("ws");
  return mg_tiny_vae_decode(&m->tiny_net, (const float*)c.dec.slot("latent")->ptr, (float*)c.dec.slot("pred")->ptr, g.K * g.B * g.n_mod, g.h, g.w,
                            g.post, ws->ptr, (long long)ws->nbytes, stream);
}

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
  delete m;   // (its temporaries free themselves; the shared weights go with the last handle over them)
}

int mg_model_info(const mg_model* m, int* cfg16) {
  MG_REQUIRE(m && cfg16, "mg_model_info: null argument");
  for (int i = 0; i < MG_CFG_WORDS; ++i) cfg16[i] = (int)m->cur().words[i];
  return 0;
}

int mg_model_num_configs(const mg_model* m) { return m ? (int)m->configs.size() : 0; }

int mg_model_config_info(const mg_model* m, int index, int* cfg16) {
  MG_REQUIRE(m && cfg16, "mg_model_config_info: null argument");
  MG_REQUIRE(index >= 0 && index < (int)m->configs.size(), "mg_model_config_info: configuration %d of %d", index, (int)m->configs.size());
  for (int i = 0; i < MG_CFG_WORDS; ++i) cfg16[i] = (int)m->configs[index].words[i];
  return 0;
}

int mg_model_find_config(const mg_model* m, int H, int W, int E, int steps, int K) {
  if (!m) {
    mg_set_error("mg_model_find_config: null model");
    return -1;
  }
  std::string have;
  for (size_t c = 0; c < m->configs.size(); ++c) {
    const Cfg& g = m->configs[c].cfg;
    if ((H < 0 || H == g.H) && (W < 0 || W == g.W) && (E < 0 || E == g.B) && (steps < 0 || steps == g.steps) && (K < 0 || K == g.K)) return (int)c;
    char one[96];
    snprintf(one, sizeof(one), "%s%u x %u (E %u, %u steps, K %d)", c ? ", " : "", (unsigned)g.H, (unsigned)g.W, (unsigned)g.B, (unsigned)g.steps, g.K);
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

long long mg_model_device_bytes(const mg_model* m) {
  uint64_t bytes = m ? m->arena_bytes : 0;
  for (int k = 0; m && k < TMP_COUNT; ++k) bytes += m->tmp[k].bytes;
  return (long long)bytes;
}

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
  const Tmp& tiled = m->tmp[TMP_TILED];
  if (tiled.p) MG_CHECK_HIP(hipMemsetAsync(tiled.p, byte, tiled.bytes, (hipStream_t)stream));
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
  const int n_noise = c.cfg.n_noise;
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

