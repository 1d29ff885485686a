// Host runtime of libmarigold_hip: error state, device init, op dispatch, op programs
// (replayed back-to-back on one HIP stream, optionally as a captured hipGraph), per-op
// HIP-event profiling.  This is the native executor behind the Python pipeline: the T-step
// denoising loop of marigold_depth_pipeline.py:455-468 becomes ONE mg_program_run call.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "common.h"
#include "kernel_once.h"

void* g_zero_page = nullptr;
void* g_splitk_ws = nullptr;
unsigned* g_ln_counters = nullptr;
thread_local bool g_dry_run = false;
static thread_local char g_err[512] = "";
static std::mutex g_init_mutex;
static int g_device = -1;
static std::atomic<int> g_cu_count{256};
static mg_kernel_once g_kernel_once;

int mg_cu_count() { return g_cu_count.load(std::memory_order_relaxed); }

// The one place the library sets a kernel attribute (contract: common.h).
int mg_kernel_max_lds(const void* kern, int bytes, bool no_static_lds) {
  return g_kernel_once.raise(kern, bytes, g_dry_run, [no_static_lds](const void* k, int b) {
    if (no_static_lds) {
      hipFuncAttributes fa;
      MG_CHECK_HIP(hipFuncGetAttributes(&fa, k));
      MG_REQUIRE(fa.sharedSizeBytes == 0, "this kernel's dynamic LDS must start at LDS address 0 (static LDS %d bytes)", (int)fa.sharedSizeBytes);
    }
    MG_CHECK_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, b));
    return 0;
  });
}

// The ONE place the library reads the environment.  Tuning switches (tile / kernel choices for A/B runs and sweeps) are honoured
// only under MARIGOLD_TUNING=1; without it every launcher runs its compiled-in default, whatever else the environment holds.
int mg_tuning_int(const char* name, int dflt) {
  static const bool on = [] { const char* e = getenv("MARIGOLD_TUNING"); return e && e[0] == '1'; }();
  if (!on) return dflt;
  const char* e = getenv(name);
  return e && e[0] ? atoi(e) : dflt;
}

void mg_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

struct mg_program {
  std::vector<mg_op> ops;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

static int dispatch(const mg_op* op, hipStream_t s) {
  switch (op->kind) {
    case MG_OP_IGEMM: return mg_launch_igemm(op, s);
    case MG_OP_CONV3X3: return mg_launch_conv_patch(op, s);
    case MG_OP_ROWGEMM: return mg_launch_rowgemm(op, s);
    case MG_OP_GN_STATS:
    case MG_OP_GN_FINALIZE:
    case MG_OP_GN_APPLY:
    case MG_OP_GN_SLAB: return mg_launch_norm(op, s);
    case MG_OP_FLASH_ATTN512: return mg_launch_flash512(op, s);
    case MG_OP_FLASH_ATTN64:
    case MG_OP_SOFTMAX_ROWS: return mg_launch_attention(op, s);
    case MG_OP_SCHED_STEP:
    case MG_OP_LINEAR_SMALL_M:
    case MG_OP_LATENT_1X1:
    case MG_OP_POST_NCHW:
    case MG_OP_IM2COL_SMALL:
    case MG_OP_MEMSET:
    case MG_OP_COPY: return mg_launch_misc(op, s);
    case MG_OP_CONV3X3_HEAD: return mg_launch_head_conv(op, s);
    case MG_OP_ENS_DEPTH_STATS:
    case MG_OP_ENS_DEPTH_MEDIAN:
    case MG_OP_ENS_DEPTH_NORM:
    case MG_OP_ENS_NORMALS:
    case MG_OP_ENS_IID: return mg_launch_ensemble(op, s);
    case MG_OP_RESIZE:
    case MG_OP_COLORIZE:
    case MG_OP_IID_VIS:
    case MG_OP_RGB_PREP:
    case MG_OP_NORMALS_VIS: return mg_launch_resize(op, s);
    case MG_OP_EVAL_DEPTH_LS:
    case MG_OP_EVAL_DEPTH_METRICS:
    case MG_OP_EVAL_NORMALS:
    case MG_OP_IIDSCORE_PREP:
    case MG_OP_IIDSCORE_PSNR:
    case MG_OP_IIDSCORE_SSIM: return mg_launch_evalscore(op, s);
    case MG_OP_RANDN: return mg_launch_randn(op, s);
    default: mg_set_error("mg_launch: unknown op kind %d", op->kind); return 2;
  }
}

extern "C" {

int mg_abi_version(void) { return MG_ABI_VERSION; }
int mg_operand_bits(void) { return MG_F16 ? 1 : 0; }

int mg_geglu_interleave(void) { return 32; }
const char* mg_last_error(void) { return g_err; }

int mg_init(int device) {
  std::lock_guard<std::mutex> lk(g_init_mutex);
  int n = 0;
  MG_CHECK_HIP(hipGetDeviceCount(&n));
  MG_REQUIRE(n > 0, "mg_init: no HIP device visible");
  MG_REQUIRE(device >= 0 && device < n, "mg_init: device %d out of range (%d devices)", device, n);
  hipDeviceProp_t prop;
  MG_CHECK_HIP(hipGetDeviceProperties(&prop, device));
  MG_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
             "mg_init: this library is built for gfx950 (MI355X) only, found %s", prop.gcnArchName);
  MG_CHECK_HIP(hipSetDevice(device));
  if (g_zero_page && g_device == device) return 0;
  MG_REQUIRE(g_device < 0 || g_device == device,
             "mg_init: one process drives one GPU (already bound to device %d)", g_device);
  if (prop.multiProcessorCount > 0) g_cu_count = prop.multiProcessorCount;
  MG_CHECK_HIP(hipMalloc(&g_zero_page, MG_ZERO_BYTES));
  MG_CHECK_HIP(hipMemset(g_zero_page, 0, MG_ZERO_BYTES));
  MG_CHECK_HIP(hipMalloc(&g_splitk_ws, MG_SPLITK_WS_BYTES));
  MG_CHECK_HIP(hipMalloc((void**)&g_ln_counters, MG_LN_COUNTERS * sizeof(unsigned)));
  MG_CHECK_HIP(hipMemset(g_ln_counters, 0, MG_LN_COUNTERS * sizeof(unsigned)));
  g_device = device;
  return 0;
}

int mg_device_info(int* cu_count, int* lds_bytes, int64_t* hbm_bytes, char* arch, int arch_len) {
  int dev = 0;
  MG_CHECK_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  MG_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
  if (cu_count) *cu_count = prop.multiProcessorCount;
  if (lds_bytes) *lds_bytes = (int)prop.maxSharedMemoryPerMultiProcessor;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  if (arch && arch_len > 0) {
    strncpy(arch, prop.gcnArchName, arch_len - 1);
    arch[arch_len - 1] = 0;
  }
  return 0;
}

int mg_launch(const mg_op* op, void* stream) {
  MG_REQUIRE(op != nullptr, "mg_launch: null op");
  return dispatch(op, (hipStream_t)stream);
}

mg_program* mg_program_create(const mg_op* ops, int n_ops) {
  if (!ops || n_ops <= 0) {
    mg_set_error("mg_program_create: empty program");
    return nullptr;
  }
  mg_program* p = new mg_program();
  p->ops.assign(ops, ops + n_ops);
  return p;
}

int mg_program_num_ops(const mg_program* prog) { return prog ? (int)prog->ops.size() : 0; }

int mg_program_run_range(mg_program* prog, int first, int count, void* stream) {
  MG_REQUIRE(prog, "mg_program_run: null program");
  MG_REQUIRE(first >= 0 && count >= 0 && first + count <= (int)prog->ops.size(),
             "mg_program_run_range: [%d,+%d) outside %d ops", first, count, (int)prog->ops.size());
  for (int i = first; i < first + count; ++i) {
    const int rc = dispatch(&prog->ops[i], (hipStream_t)stream);
    if (rc) {
      char msg[400];
      snprintf(msg, sizeof(msg), "%s", g_err);
      mg_set_error("op %d (kind %d): %s", i, prog->ops[i].kind, msg);
      return rc;
    }
  }
  return 0;
}

int mg_program_validate(mg_program* prog) {
  MG_REQUIRE(prog, "mg_program_validate: null program");
  g_dry_run = true;
  const int rc = mg_program_run_range(prog, 0, (int)prog->ops.size(), nullptr);
  g_dry_run = false;
  return rc;
}

int mg_program_run(mg_program* prog, void* stream) {
  MG_REQUIRE(prog, "mg_program_run: null program");
  if (prog->exec) {
    MG_CHECK_HIP(hipGraphLaunch(prog->exec, (hipStream_t)stream));
    return 0;
  }
  return mg_program_run_range(prog, 0, (int)prog->ops.size(), stream);
}

int mg_program_capture(mg_program* prog, void* stream) {
  MG_REQUIRE(prog, "mg_program_capture: null program");
  hipStream_t s = (hipStream_t)stream;
  if (prog->exec) { hipGraphExecDestroy(prog->exec); prog->exec = nullptr; }
  if (prog->graph) { hipGraphDestroy(prog->graph); prog->graph = nullptr; }
  // one eager run first so lazy per-kernel attribute setup happens outside the capture
  int rc = mg_program_run_range(prog, 0, (int)prog->ops.size(), stream);
  if (rc) return rc;
  MG_CHECK_HIP(hipStreamSynchronize(s));
  MG_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  rc = mg_program_run_range(prog, 0, (int)prog->ops.size(), stream);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(s, &g);
  if (rc) { if (g) hipGraphDestroy(g); return rc; }
  MG_REQUIRE(e == hipSuccess && g, "mg_program_capture: hipStreamEndCapture failed: %s", hipGetErrorString(e));
  prog->graph = g;
  MG_CHECK_HIP(hipGraphInstantiate(&prog->exec, g, nullptr, nullptr, 0));
  return 0;
}

int mg_program_profile(mg_program* prog, void* stream, float* ms) {
  MG_REQUIRE(prog && ms, "mg_program_profile: null argument");
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)prog->ops.size();
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) MG_CHECK_HIP(hipEventCreate(&e));
  MG_CHECK_HIP(hipEventRecord(ev[0], s));
  for (int i = 0; i < n; ++i) {
    const int rc = dispatch(&prog->ops[i], s);
    if (rc) return rc;
    MG_CHECK_HIP(hipEventRecord(ev[i + 1], s));
  }
  MG_CHECK_HIP(hipEventSynchronize(ev[n]));
  for (int i = 0; i < n; ++i) MG_CHECK_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
  for (auto& e : ev) hipEventDestroy(e);
  return 0;
}

void mg_program_destroy(mg_program* prog) {
  if (!prog) return;
  if (prog->exec) hipGraphExecDestroy(prog->exec);
  if (prog->graph) hipGraphDestroy(prog->graph);
  delete prog;
}

int mg_conv2d_igemm(const mg_op* conv_desc, void* stream) {
  MG_REQUIRE(conv_desc && conv_desc->kind == MG_OP_IGEMM, "mg_conv2d_igemm: op kind must be MG_OP_IGEMM");
  return mg_launch_igemm(conv_desc, (hipStream_t)stream);
}

int mg_conv3x3_gn_slots(const mg_op* conv_desc) {
  if (!conv_desc || conv_desc->kind != MG_OP_CONV3X3) return 0;
  return mg_conv3x3_gn_slots_of(conv_desc);
}

int mg_conv3x3(const mg_op* conv_desc, void* stream) {
  MG_REQUIRE(conv_desc && conv_desc->kind == MG_OP_CONV3X3, "mg_conv3x3: op kind must be MG_OP_CONV3X3");
  return mg_launch_conv_patch(conv_desc, (hipStream_t)stream);
}

int mg_sched_step(const float* x, const float* model_out, const float* noise, float* out, int64_t n,
                  float cx, float cm, float cn, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_SCHED_STEP;
  op.p[MG_SCHED_STEP_P_X] = (void*)x;
  op.p[MG_SCHED_STEP_P_MODEL_OUT] = (void*)model_out;
  op.p[MG_SCHED_STEP_P_NOISE] = (void*)noise;
  op.p[MG_SCHED_STEP_P_OUT] = out;
  op.l[MG_SCHED_STEP_L_N] = n;
  op.f[MG_SCHED_STEP_F_CX] = cx;
  op.f[MG_SCHED_STEP_F_CM] = cm;
  op.f[MG_SCHED_STEP_F_CN] = cn;
  return mg_launch_misc(&op, (hipStream_t)stream);
}

int mg_ensemble_normals(const float* normals, float* out, float* unc, int E, int64_t hw, int reduction,
                        void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_ENS_NORMALS;
  op.p[MG_ENS_NORMALS_P_NORMALS] = (void*)normals;
  op.p[MG_ENS_NORMALS_P_OUT] = out;
  op.p[MG_ENS_NORMALS_P_UNC] = unc;
  op.i[MG_ENS_NORMALS_I_E] = E;
  op.i[MG_ENS_NORMALS_I_REDUCTION] = reduction;
  op.l[MG_ENS_NORMALS_L_HW] = hw;
  return mg_launch_ensemble(&op, (hipStream_t)stream);
}

int mg_ensemble_iid(const float* preds, int E, int64_t n, int reduction, float* pred_out, float* unc_out_or_null, void* stream) {
  MG_REQUIRE(preds && pred_out, "mg_ensemble_iid: null pointer");
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_ENS_IID;
  op.p[MG_ENS_IID_P_PREDS] = (void*)preds; op.p[MG_ENS_IID_P_PRED] = pred_out; op.p[MG_ENS_IID_P_UNC] = unc_out_or_null;
  op.i[MG_ENS_IID_I_E] = E; op.i[MG_ENS_IID_I_REDUCTION] = reduction;
  op.l[MG_ENS_IID_L_N] = n;
  return mg_launch_ensemble(&op, (hipStream_t)stream);
}

int mg_resize(const void* src, void* dst, float* tmp_or_null, int planes, int Hin, int Win, int Hout, int Wout, int mode, int u8,
              void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_RESIZE;
  op.p[MG_RESIZE_P_SRC] = (void*)src;
  op.p[MG_RESIZE_P_DST] = dst;
  op.p[MG_RESIZE_P_TMP] = tmp_or_null;
  op.i[MG_RESIZE_I_PLANES] = planes;
  op.i[MG_RESIZE_I_HIN] = Hin;
  op.i[MG_RESIZE_I_WIN] = Win;
  op.i[MG_RESIZE_I_HOUT] = Hout;
  op.i[MG_RESIZE_I_WOUT] = Wout;
  op.i[MG_RESIZE_I_MODE] = mode;
  op.i[MG_RESIZE_I_U8] = u8 != 0;
  return mg_launch_resize(&op, (hipStream_t)stream);
}

int mg_colorize(const float* depth, const uint8_t* lut256x3, uint8_t* out_hwc, int64_t n, float min_depth, float max_depth, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_COLORIZE;
  op.p[MG_COLORIZE_P_DEPTH] = (void*)depth;
  op.p[MG_COLORIZE_P_LUT] = (void*)lut256x3;
  op.p[MG_COLORIZE_P_OUT] = out_hwc;
  op.l[MG_COLORIZE_L_N] = n;
  op.f[MG_COLORIZE_F_MIN_DEPTH] = min_depth;
  op.f[MG_COLORIZE_F_MAX_DEPTH] = max_depth;
  return mg_launch_resize(&op, (hipStream_t)stream);
}

int mg_iid_visualize(const float* pred, uint8_t* out_hwc, float* workspace_or_null, int n_targets, int H, int W, int linear_bits,
                     int up_to_scale_bits, void* stream) {
  mg_op op;
  memset(&op, 0, sizeof(op));
  op.kind = MG_OP_IID_VIS;
  op.p[MG_IID_VIS_P_PRED] = (void*)pred;
  op.p[MG_IID_VIS_P_OUT] = out_hwc;
  op.p[MG_IID_VIS_P_WS] = workspace_or_null;
  op.i[MG_IID_VIS_I_N] = n_targets;
  op.i[MG_IID_VIS_I_H] = H;
  op.i[MG_IID_VIS_I_W] = W;
  op.i[MG_IID_VIS_I_LINEAR_BITS] = linear_bits;
  op.i[MG_IID_VIS_I_UP_TO_SCALE_BITS] = up_to_scale_bits;
  return mg_launch_resize(&op, (hipStream_t)stream);
}

// ---- shader clock under matrix-core load (mg_clock_probe; bench.py's calibration block) ----
namespace {
__global__ __launch_bounds__(256) void clock_probe_kernel(unsigned long long* out, const uint4* data, int iters) {
  const bf16x8 a = __builtin_bit_cast(bf16x8, data[threadIdx.x]), b = __builtin_bit_cast(bf16x8, data[threadIdx.x + 256]);
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // two independent accumulator chains: the pipe issues one MFMA per 32 cycles
      asm volatile(MG_MFMA32_ASM " %0, %1, %2, %0" : "+v"(acc0) : "v"(a), "v"(b));
      asm volatile(MG_MFMA32_ASM " %0, %1, %2, %0" : "+v"(acc1) : "v"(a), "v"(b));
    }
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float sink = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) sink += acc0[r] + acc1[r];
  if (sink == 12345.678f) out[2 * gridDim.x] = 1;   // keeps the chains alive
  if (threadIdx.x == 0) { out[blockIdx.x * 2] = c1 - c0; out[blockIdx.x * 2 + 1] = r1 - r0; }
}
}  // namespace

namespace {
struct ClockProbeRes {   // frees on every exit path
  unsigned long long* d_out = nullptr;
  uint4* d_data = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~ClockProbeRes() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_out) (void)hipFree(d_out);
    if (d_data) (void)hipFree(d_data);
  }
};
}  // namespace

int mg_clock_probe(void* stream, int zero_operands, double* mhz, double* tflops) {
  MG_REQUIRE(mhz && tflops, "mg_clock_probe: null output");
  int dev = 0, cus = 0;
  MG_CHECK_HIP(hipGetDevice(&dev));
  MG_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const hipStream_t s = (hipStream_t)stream;
  ClockProbeRes R;
  MG_CHECK_HIP(hipMalloc(&R.d_out, (size_t)(2 * cus + 1) * 8));
  MG_CHECK_HIP(hipMalloc(&R.d_data, 512 * 16));
  unsigned h[2048];
  unsigned seed = 12345u;
  for (int i = 0; i < 2048; ++i) {   // bf16 pairs in (-2, 2), random sign / mantissa
    seed = seed * 1664525u + 1013904223u;
    const unsigned lo = 0x3f00u | ((seed >> 8) & 0x80ffu), hi = 0x3f00u | ((seed >> 20) & 0x80ffu);
    h[i] = zero_operands ? 0u : (lo | (hi << 16));
  }
  MG_CHECK_HIP(hipMemcpyAsync(R.d_data, h, sizeof(h), hipMemcpyHostToDevice, s));
  const int iters = 20000;   // x 8 MFMAs x 32 cycles = 5.1 M cycles, 2-3 ms
  MG_CHECK_HIP(hipEventCreate(&R.e0));
  MG_CHECK_HIP(hipEventCreate(&R.e1));
  float ms = 0.f;
  for (int rep = 0; rep < 2; ++rep) {   // the second launch is the measurement (clocks settled)
    MG_CHECK_HIP(hipEventRecord(R.e0, s));
    hipLaunchKernelGGL(clock_probe_kernel, dim3(cus), dim3(256), 0, s, R.d_out, R.d_data, iters);
    MG_CHECK_HIP(hipEventRecord(R.e1, s));
    MG_CHECK_HIP(hipStreamSynchronize(s));
  }
  MG_CHECK_HIP(hipEventElapsedTime(&ms, R.e0, R.e1));
  std::vector<unsigned long long> r(2 * cus);
  MG_CHECK_HIP(hipMemcpy(r.data(), R.d_out, (size_t)2 * cus * 8, hipMemcpyDeviceToHost));
  double sc = 0.0, rt = 0.0;
  for (int i = 0; i < cus; ++i) { sc += (double)r[2 * i]; rt += (double)r[2 * i + 1]; }
  *mhz = rt > 0.0 ? sc / rt * 100.0 : 0.0;
  *tflops = ms > 0.f ? (double)cus * 4.0 * iters * 8.0 * 2.0 * 32 * 32 * 16 / (ms * 1e-3) / 1e12 : 0.0;
  return 0;
}

// Tuning only: copy the first `bytes` of the split-K workspace (where MARIGOLD_IGEMM_STAMPS=1 launches leave their phase stamps)
// to the host.  Synchronises the device.
int mg_debug_read_workspace(void* host_dst, long long bytes) {
  MG_REQUIRE(host_dst && bytes > 0 && bytes <= MG_SPLITK_WS_BYTES && g_splitk_ws, "mg_debug_read_workspace: bad arguments");
  MG_CHECK_HIP(hipDeviceSynchronize());
  MG_CHECK_HIP(hipMemcpy(host_dst, g_splitk_ws, (size_t)bytes, hipMemcpyDeviceToHost));
  return 0;
}

void* mg_event_create(void) {
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return (void*)e;
}
int mg_event_record(void* ev, void* stream) {
  MG_CHECK_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return 0;
}
int mg_event_elapsed_ms(void* start, void* stop, float* ms) {
  MG_CHECK_HIP(hipEventSynchronize((hipEvent_t)stop));
  MG_CHECK_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return 0;
}
void mg_event_destroy(void* ev) {
  if (ev) hipEventDestroy((hipEvent_t)ev);
}

}  // extern "C"
