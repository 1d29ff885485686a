// The one-call predictions over a loaded model image (csrc/model.hip; csrc/model.h is what the two files share): picture bytes and
// a seed in, the ensembled map and its pictures out - one picture, several, the next frame of a sequence, a large picture in tiles,
// an intrinsic-image model - and mg_ensemble_depth, the depth ensembling they call.
#include <stdio.h>
#include <string.h>

#include "model.h"

using namespace mg_image;

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

// What a prediction is made from: n pictures (uint8, hwc or planar, one size Hin x Win; mode / reciprocal: the input resampling of
// mg_rgb_prepare) and a seed each.  carry: the strength of mg_model_predict_next, null in every other call.
struct PredictIn {
  int n;
  const uint8_t* const* rgb;
  int hwc, Hin, Win, mode, reciprocal;
  const uint64_t* seeds;
  const float* carry;
};
struct PredictOut {   // where it goes, picture-major; all but pred may be null
  float *pred, *unc;
  uint16_t* u16;
  uint8_t* picture;
  double* info4;
};

// Stages 1 to 5 of a one-call prediction, the same for every kind of model, for the n <= K pictures of one call: each picture into its
// row of the encoder's input, ONE encode, each picture's noise into its B rows (MG_OP_RANDN of its own seed: stream 0 = the initial
// latents, stream k + 1 = the LCM scheduler's step noise k - what its lone call draws), ONE denoise, ONE decode.  A call with n < K
// feeds picture n - 1 and its seed to the spare rows too, so that nothing in the programs reads what an earlier call left; the
// spare results are never read.  `who` names the entry point in the messages.  On return the K B members lie image-major in the
// decode program's output slot, *preds.  One picture per call is the n = K = 1 case.
int predict_members(mg_model* m, const char* who, const PredictIn& in, void* stream, const float** preds) {
  const Cfg& g = m->cur().cfg;
  const int K = g.K, H = g.H, W = g.W, n = in.n, Hin = in.Hin, Win = in.Win;
  MG_REQUIRE(Hin > 0 && Win > 0, "%s: bad input size %d x %d", who, Hin, Win);
  const hipStream_t s = (hipStream_t)stream;
  const Slot *e_in = m->cur().enc.slot("rgb"), *e_out = m->cur().enc.slot("latent"), *rl = m->cur().den.slot("rgb_latent"), *xs = m->cur().den.slot("x");
  const Slot *d_in = m->cur().dec.slot("latent"), *d_out = m->cur().dec.slot("pred");
  // (mg_model_load checked that the slots chain)
  const uint64_t rgb_row = e_in->nbytes / K, x_rows = xs->nbytes / K;   // bytes per picture
  // 1. picture i -> [1,3,H,W] in [-1, 1], row i of the encoder's input slot
  float* tmp = nullptr;
  if (in.mode != 2 && Hin != H && Win != W) {
    if (int rc = m->tmp[TMP_INPUT].grow((uint64_t)3 * Hin * W * 4)) return rc;
    tmp = (float*)m->tmp[TMP_INPUT].p;
  }
  for (int i = 0; i < K; ++i)
    if (int rc = mg_rgb_prepare(in.rgb[i < n ? i : n - 1], in.hwc, Hin, Win, e_in->ptr + i * rgb_row, 0, H, W, in.mode, in.reciprocal, tmp, stream))
      return rc;
  // 2. encode
  if (int rc = run_encode(m, stream)) return rc;
  if (int rc = copy_dd(rl->ptr, e_out->ptr, rl->nbytes, s)) return rc;
  // 3. the initial latents: stream 0; the LCM scheduler's step noises: stream k + 1
  for (int i = 0; i < K; ++i)
    if (int rc = mg_randn(in.seeds[i < n ? i : n - 1], 0, 0, (int64_t)(x_rows / 4), xs->ptr + i * x_rows, 0, stream)) return rc;
  // (mg_model_predict_next, K = 1) the frame before, member by member, into the initial latents
  float* const seq_latent = (float*)m->tmp[TMP_SEQUENCE].p;
  if (in.carry && m->seq_carried)
    if (int rc = mg_latent_carry((float*)xs->ptr, seq_latent, (int64_t)(xs->nbytes / 4), *in.carry, stream)) return rc;
  for (int k = 0; k < g.n_noise; ++k) {
    char nm[24];
    snprintf(nm, sizeof(nm), "noise%d", k);
    const Slot* ns = m->cur().den.slot(nm);
    MG_REQUIRE(ns && ns->nbytes == xs->nbytes, "%s: the image lacks slot %s", who, nm);
    for (int i = 0; i < K; ++i)
      if (int rc = mg_randn(in.seeds[i < n ? i : n - 1], (uint64_t)k + 1, 0, (int64_t)(x_rows / 4), ns->ptr + i * x_rows, 0, stream)) return rc;
  }
  // 4. denoise, 5. decode (an intrinsic-image model: the latent [B, 4 n, h, w] is the decoder's batch [B n, 4, h, w], the same bytes)
  if (int rc = mg_program_run(m->cur().den.prog, stream)) return rc;
  if (in.carry) {   // this frame's denoised latent, for the next one
    if (int rc = copy_dd(seq_latent, xs->ptr, xs->nbytes, s)) return rc;
    m->seq_carried = true;
  }
  if (int rc = copy_dd(d_in->ptr, xs->ptr, d_in->nbytes, s)) return rc;
  if (int rc = run_decode(m, stream)) return rc;
  *preds = (const float*)d_out->ptr;
  return 0;
}

// out_h / out_w / out_mode of an entry point's options (0 x 0: the decoded size; max_pixels 0: no bound) -> the size to store
int output_size(const char* who, int out_h, int out_w, int out_mode, long long max_pixels, int Ho, int Wo, int* oh, int* ow) {
  MG_REQUIRE((out_h == 0 && out_w == 0) || (out_h > 0 && out_w > 0 && (!max_pixels || (long long)out_h * out_w <= max_pixels)),
             "%s: bad output size %d x %d", who, out_h, out_w);
  MG_REQUIRE(out_mode >= 0 && out_mode <= 2, "%s: out_mode must be 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)", who);
  *oh = out_h ? out_h : Ho;
  *ow = out_w ? out_w : Wo;
  return 0;
}

// Stages 1 to 7 of a one-call prediction of n pictures: the members (predict_members), then for picture i, one after the other,
// 6. ensemble(i, members, dst) -> int: its B members in the decoder's output slot -> the ensembled map (one member: the pipelines
//    return it as it is, without an uncertainty, and `ensemble` is not called),
// 7. match_input_res (marigold_depth_pipeline.py:306-312, marigold_normals_pipeline.py:282-288, marigold_iid_pipeline.py:378-385):
//    the prediction only, [planes][Ho][Wo] -> row i of pred_out [n][planes][oh][ow],
// 8. finish(i, row i of pred_out) -> int: the entry point's output stage on what was stored.
// The output temporaries, in this order: the ensembled map at the decoded size (several members AND a resize: the resize reads it),
// the resize's fp32 intermediate [planes][Ho][out_w] (modes 0 / 1 when both sizes change), the picture stage's workspace of ws_bytes
// (intrinsic images: [n][MG_IID_VIS_PARTS] for a target that is linear and up to scale; depth and normals: none) -> *ws (may be
// null), valid until the model's next prediction.  They serve the pictures in turn (the stream orders them).
template <class Ensemble, class Finish>
int predict_resized(mg_model* m, const char* who, const PredictIn& in, int planes, int oh, int ow, int out_mode, uint64_t ws_bytes, float* pred_out,
                    float** ws, void* stream, Ensemble ensemble, Finish finish) {
  const Cfg& g = m->cur().cfg;
  const int B = g.B, Ho = g.Ho, Wo = g.Wo;
  const bool resize = oh != Ho || ow != Wo;
  float *ens = nullptr, *rtmp = nullptr, *pic_ws = nullptr;
  if (int rc = lay_out(m->tmp[TMP_OUTPUT], [&](Arena& a) {
        a.part(&ens, resize && B > 1 ? (uint64_t)planes * Ho * Wo * 4 : 0);
        a.part(&rtmp, resize && out_mode != 2 && oh != Ho && ow != Wo ? (uint64_t)planes * Ho * ow * 4 : 0);
        a.part(&pic_ws, ws_bytes);
      }))
    return rc;
  if (ws) *ws = pic_ws;
  const float* all = nullptr;
  if (int rc = predict_members(m, who, in, stream, &all)) return rc;
  for (int i = 0; i < in.n; ++i) {
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

// Stages 1 to 8 of a depth / normals prediction of n pictures; out.unc [n][Ho][Wo], out.info4 [n][4], the pictures of the output stage
// (out.u16 [n][oh][ow], out.picture [n][oh][ow][3]; `clip`: the output stage runs - mg_model_predict stores the map as it is)
int predict_depth_or_normals(mg_model* m, const char* who, const PredictIn& in, const mg_predict_opts* opts_or_null, int oh, int ow, int out_mode,
                             bool clip, const uint8_t* lut256x3, const PredictOut& out, void* stream) {
  const Cfg& g = m->cur().cfg;
  const int B = g.B, post = g.post, Ho = g.Ho, Wo = g.Wo;
  static const mg_predict_opts defaults = MG_PREDICT_OPTS_DEFAULT;
  const mg_predict_opts& o = opts_or_null ? *opts_or_null : defaults;
  if (out.info4)
    for (int i = 0; i < 4 * in.n; ++i) out.info4[i] = 0.0;
  const uint64_t HWo = (uint64_t)Ho * Wo, hw = (uint64_t)oh * ow;
  return predict_resized(
      m, who, in, g.C, oh, ow, out_mode, 0, out.pred, nullptr, stream,
      [&](int i, const float* preds, float* dst) {
        float* const unc = out.unc ? out.unc + i * HWo : nullptr;
        if (post == MG_POST_DEPTH)
          return mg_ensemble_depth(preds, B, Ho, Wo, o.scale_invariant, o.shift_invariant, o.reduction, o.regularizer_strength, o.max_iter, o.tol,
                                   o.max_res, dst, unc, out.info4 ? out.info4 + 4 * i : nullptr, stream);
        MG_REQUIRE(o.normals_reduction == 0 || o.normals_reduction == 1, "Unrecognized reduction method: %d.", o.normals_reduction);
        return mg_ensemble_normals(preds, dst, unc, B, (int64_t)HWo, o.normals_reduction, stream);
      },
      // 8. the output stage on what was stored, in place: the clip (:314-316 / :294), the 16-bit depth (script/depth/run.py), the picture
      [&](int i, float* map) {
        if (!clip) return 0;
        uint8_t* const pic = out.picture ? out.picture + i * hw * 3 : nullptr;
        if (post == MG_POST_DEPTH) return mg_depth_visualize(map, lut256x3, (int64_t)hw, map, out.u16 ? out.u16 + i * hw : nullptr, pic, stream);
        return mg_normals_finish(map, oh, ow, map, pic, stream);
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
int predict_out_many(mg_model* m, const char* who, const PredictIn& in, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                     const PredictOut& out, void* stream) {
  const Cfg& g = m->cur().cfg;
  MG_REQUIRE(g.post != MG_POST_UNIT && g.n_mod == 1, "%s: an intrinsic-image model goes through mg_model_predict_iid", who);
  static const mg_output_opts out_defaults = MG_OUTPUT_OPTS_DEFAULT;
  const mg_output_opts& q = out_opts_or_null ? *out_opts_or_null : out_defaults;
  int oh, ow;
  if (int rc = check_output_opts(who, g.post, g.C, q, g.Ho, g.Wo, out.u16, out.picture, &oh, &ow)) return rc;
  return predict_depth_or_normals(m, who, in, opts_or_null, oh, ow, q.out_mode, true, q.lut256x3, out, stream);
}

// mg_model_predict_tiled: the handle goes back to the configuration it was on, on every way out
struct Reselect {
  mg_model* m;
  int sel;
  ~Reselect() { m->sel = sel; }
};

}  // namespace

// An image of several pictures per call runs through mg_model_predict_many only
#define MG_REQUIRE_ONE_PICTURE(m, who) \
  MG_REQUIRE((m)->cur().cfg.K == 1, who ": this image runs %d pictures per call: use mg_model_predict_many", (m)->cur().cfg.K)

extern "C" int mg_model_predict(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                const mg_predict_opts* opts_or_null, float* pred_out, float* unc_out_or_null, double* info4_or_null,
                                void* stream) {
  MG_REQUIRE(m && !m->host_only && rgb && pred_out, "mg_model_predict: bad arguments (or a host-only model)");
  MG_REQUIRE_ONE_PICTURE(m, "mg_model_predict");
  const Cfg& g = m->cur().cfg;
  MG_REQUIRE(g.post != MG_POST_UNIT && g.n_mod == 1, "mg_model_predict: intrinsic-image models are not supported yet");
  MG_REQUIRE((g.post == MG_POST_DEPTH && g.C == 1) || (g.post == MG_POST_NORMALS && g.C == 3), "mg_model_predict: a depth or a normals image is required");
  // the map at the decoded size: no resize, no temporaries
  return predict_depth_or_normals(m, "mg_model_predict", {1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, nullptr}, opts_or_null, g.Ho, g.Wo, 0, false,
                                  nullptr, {pred_out, unc_out_or_null, nullptr, nullptr, info4_or_null}, stream);
}

extern "C" int mg_model_predict_out(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                    const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out,
                                    float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null,
                                    void* stream) {
  MG_REQUIRE(m && rgb && pred_out, "mg_model_predict_out: null argument (the model, the picture and pred_out are required)");
  MG_REQUIRE(!m->host_only, "mg_model_predict_out: a host-only model cannot predict (load it with device >= 0)");
  MG_REQUIRE_ONE_PICTURE(m, "mg_model_predict_out");
  return predict_out_many(m, "mg_model_predict_out", {1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, nullptr}, opts_or_null, out_opts_or_null,
                          {pred_out, unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null}, stream);
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
  const Cfg& g = m->cur().cfg;
  MG_REQUIRE(g.K == 1, "mg_model_predict_next: this configuration runs %d pictures per call: a sequence runs one frame per call (K = 1)", g.K);
  MG_REQUIRE(strength >= 0.f && strength <= 1.f, "mg_model_predict_next: strength %g is not in [0, 1]", (double)strength);
  MG_REQUIRE(g.post != MG_POST_UNIT && g.n_mod == 1, "mg_model_predict_next: an intrinsic-image model goes through mg_model_predict_iid");
  const uint64_t need = m->cur().den.slot("x")->nbytes;
  if (m->tmp[TMP_SEQUENCE].bytes < need) m->seq_carried = false;
  if (int rc = m->tmp[TMP_SEQUENCE].grow(need)) return rc;
  const int rc = predict_out_many(m, "mg_model_predict_next", {1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, &strength}, opts_or_null, out_opts_or_null,
                                  {pred_out, unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null}, stream);
  if (rc) m->seq_carried = false;   // a frame that failed carries nothing on
  return rc;
}

extern "C" int mg_model_predict_many(mg_model* m, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                                     const uint64_t* seeds, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                                     float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                                     double* info4_or_null, void* stream) {
  MG_REQUIRE(m, "mg_model_predict_many: null model");
  MG_REQUIRE(!m->host_only, "mg_model_predict_many: a host-only model cannot predict (load it with device >= 0)");
  const int K = m->cur().cfg.K;
  MG_REQUIRE(n >= 1 && n <= K, "mg_model_predict_many: %d pictures for an image of %d per call (1 <= n <= %d)", n, K, K);
  MG_REQUIRE(rgb && seeds && pred_out, "mg_model_predict_many: null argument (the rgb and seeds arrays and pred_out are required)");
  for (int i = 0; i < n; ++i) MG_REQUIRE(rgb[i], "mg_model_predict_many: null picture %d of %d", i, n);
  return predict_out_many(m, "mg_model_predict_many", {n, rgb, hwc, Hin, Win, mode, reciprocal, seeds, nullptr}, opts_or_null, out_opts_or_null,
                          {pred_out, unc_out_or_null, u16_out_or_null, picture_out_or_null, info4_or_null}, stream);
}

// ---- the tiled prediction of a large picture as one call (pipe.predict_tiled): plan -> guide -> tiles, a group of K per
// call of the tile configuration's programs -> fit and blend -> resize -> output stage.  Every stage is the code the calls above and
// csrc/tiles.hip already run; this function only strings them together.
extern "C" int mg_model_predict_tiled(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,
                                      const mg_tiled_opts* tiled, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                                      float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                                      double* info4_or_null, int* degenerate_or_null, void* stream) {
  const char* who = "mg_model_predict_tiled";
  MG_REQUIRE(m && rgb && tiled && pred_out, "%s: null argument (the model, the picture, tiled and pred_out are required)", who);
  const int n_cfg = (int)m->configs.size();
  MG_REQUIRE(tiled->tile_config >= 0 && tiled->tile_config < n_cfg, "%s: tile configuration %d of %d", who, tiled->tile_config, n_cfg);
  const Cfg& tc = m->configs[tiled->tile_config].cfg;
  const int B = tc.B, th = tc.H, tw = tc.W, C = tc.C, post = tc.post, K = tc.K;
  MG_REQUIRE(post != MG_POST_UNIT && tc.n_mod == 1, "%s: an intrinsic-image model is not supported (depth and normals only)", who);
  const bool depth = post == MG_POST_DEPTH && C == 1;
  MG_REQUIRE(depth || (post == MG_POST_NORMALS && C == 3), "%s: a depth or a normals image is required", who);
  MG_REQUIRE(Hin >= 8 && Win >= 8 && Hin % 8 == 0 && Win % 8 == 0, "%s: the picture size %d x %d must be multiples of 8 (the call works at the picture's size)",
             who, Hin, Win);
  MG_REQUIRE((long long)Hin * Win <= (1ll << 28) && Hin <= 65535, "%s: a picture of %d x %d is not supported", who, Hin, Win);
  MG_REQUIRE(th % 8 == 0 && tw % 8 == 0 && tc.Ho == th && tc.Wo == tw && (long long)th * tw <= (1ll << 26),
             "%s: the tile configuration's size %d x %d (decoded %d x %d) must be multiples of 8, decoded at that size", who, th, tw, tc.Ho, tc.Wo);
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
    const Cfg& gc = m->configs[tiled->guide_config].cfg;
    MG_REQUIRE(gc.K == 1, "%s: the guide configuration runs %d pictures per call, the guide is ONE picture (K = 1)", who, gc.K);
    MG_REQUIRE(gc.B == B, "%s: the guide configuration has %d members, the tile configuration %d", who, gc.B, B);
    MG_REQUIRE(gc.post == post && gc.C == C && gc.n_mod == 1, "%s: the guide configuration is of another kind than the tile configuration", who);
    hg = gc.Ho;
    wg = gc.Wo;
    MG_REQUIRE(hg >= 1 && wg >= 1 && (long long)hg * wg <= (1ll << 26), "%s: bad guide size %d x %d", who, hg, wg);
  }
  // the short last group: r tiles, whole on a configuration of r pictures per call, or padded on the tile configuration
  const int r = n % K;
  const bool tail = r != 0 && tiled->tail_config != -1;
  if (tail) {
    MG_REQUIRE(tiled->tail_config >= 0 && tiled->tail_config < n_cfg, "%s: tail configuration %d of %d", who, tiled->tail_config, n_cfg);
    const Cfg& lc = m->configs[tiled->tail_config].cfg;
    MG_REQUIRE(lc.K == r, "%s: the tail configuration runs %d pictures per call, the short last group has %d tiles (%d tiles, %d per call)", who, lc.K,
               r, n, K);
    MG_REQUIRE(lc.B == B && lc.post == post && lc.C == C && lc.n_mod == 1 && lc.H == th && lc.W == tw && lc.Ho == th && lc.Wo == tw,
               "%s: the tail configuration is of another kind, size (%d x %d) or member count (%d) than the tile configuration (%d x %d, %d)", who,
               lc.H, lc.W, lc.B, th, tw, B);
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

  // the temporaries: ONE list of parts, in the order they lie
  const bool with_unc = B > 1 && unc_out_or_null, resize = oh != Hin || ow != Win;
  const uint64_t tile_px = (uint64_t)th * tw, fit_bytes = depth ? r256((uint64_t)mg_tiles_workspace_bytes(n, th, tw)) : 0;
  uint8_t* crops = nullptr;
  float *maps = nullptr, *uncs = nullptr, *guide = nullptr, *resized_from = nullptr, *rtmp = nullptr;
  double *coef = nullptr, *coef_unc = nullptr;
  void* fit_ws = nullptr;
  int* own_flags = nullptr;
  if (int rc = lay_out(m->tmp[TMP_TILED], [&](Arena& a) {
        a.part(&crops, (uint64_t)K * 3 * tile_px);
        a.part(&maps, (uint64_t)n * C * tile_px * 4);
        a.part(&uncs, with_unc ? (uint64_t)n * tile_px * 4 : 0);
        a.part(&fit_ws, fit_bytes);
        a.part(&coef, depth ? (uint64_t)n * 16 : 0);
        a.part(&coef_unc, depth && with_unc ? (uint64_t)n * 16 : 0);
        a.part(&own_flags, depth && !degenerate_or_null ? (uint64_t)n * 4 : 0);
        a.part(&guide, depth ? (uint64_t)hg * wg * 4 : 0);
        a.part(&resized_from, resize ? (uint64_t)C * Hin * Win * 4 : 0);
        a.part(&rtmp, resize && q.out_mode != 2 && oh != Hin && ow != Win ? (uint64_t)C * Hin * ow * 4 : 0);
      }))
    return rc;
  int* const flags = degenerate_or_null ? degenerate_or_null : own_flags;
  float* const canvas = resize ? resized_from : pred_out;
  const hipStream_t s = (hipStream_t)stream;

  Reselect back = {m, m->sel};
  if (info4_or_null)
    for (int i = 0; i < 4; ++i) info4_or_null[i] = 0.0;
  // 2. the guide: one ordinary prediction of the whole picture at the guide configuration's size, clipped
  if (depth) {
    m->sel = tiled->guide_config;
    if (int rc = predict_depth_or_normals(m, who, {1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, nullptr}, opts_or_null, hg, wg, 0, true, nullptr,
                                          {guide, nullptr, nullptr, nullptr, info4_or_null}, stream))
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
    const PredictIn group = {cnt, pics.data(), hwc, th, tw, 0, 1, seeds.data(), nullptr};
    const PredictOut group_out = {maps + (uint64_t)first * C * tile_px, with_unc ? uncs + (uint64_t)first * tile_px : nullptr, nullptr, nullptr, nullptr};
    if (int rc = predict_depth_or_normals(m, who, group, opts_or_null, th, tw, 0, true, nullptr, group_out, stream)) return rc;
  }
  // 4. the stitch
  const int oy = tiled->overlap_y, ox = tiled->overlap_x;
  if (depth) {
    if (int rc = mg_tile_fit(maps, th, tw, ys, ny, xs, nx, Hin, Win, guide, hg, wg, coef, flags, fit_ws, (long long)fit_bytes, stream)) return rc;
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
  const Cfg& g = m->cur().cfg;
  const int B = g.B, C = g.C, post = g.post, n_noise = g.n_noise, n = g.n_mod, Ho = g.Ho, Wo = g.Wo;
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
      m, "mg_model_predict_iid", {1, &rgb, hwc, Hin, Win, mode, reciprocal, &seed, nullptr}, C, oh, ow, o.out_mode, ws_bytes, pred_out, &ws, stream,
      [&](int, const float* preds, float* dst) { return mg_ensemble_iid(preds, B, (int64_t)C * Ho * Wo, o.reduction, dst, unc_out_or_null, stream); },
      // 8. the pictures of what was stored (fill_outputs -> MarigoldIIDOutput.fill_entry, :117-136, :393-411)
      [&](int, float* out) {
        if (!pictures_out_or_null) return 0;
        return mg_iid_visualize(out, pictures_out_or_null, ws, n, oh, ow, o.linear_bits, o.up_to_scale_bits, stream);
      });
}
