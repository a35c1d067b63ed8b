// mcm_api.hip — the C ABI of libmcm_hip.so (include/mcm.h): parameter store, workspace,
// the two CLIP towers as sequences of kernel launches on the caller's stream, the fused
// scoring tail, per-kernel HIP-event timing, and operator-level entry points.
//
// Tower structure follows HF modeling_clip.py (the library the reference delegates to):
//   vision  CLIPVisionEmbeddings.forward :202-218 → pre_layrnorm :642 → CLIPEncoderLayer
//           ×L :362-383 → CLS pool + post_layernorm :650-651 → visual_projection :751
//   text    CLIPTextEmbeddings :232-256 → causal CLIPEncoderLayer ×L → final_layer_norm
//           :559 → EOS pool :561-581 → text_projection :713
// and the reference's own tail utils/detection_util.py:226,231-248.
// The residual stream is fp32 in HBM; vision GEMM operands are fp16 or bf16 (cfg.precision; exact fp32 in the
// parity mode), the text tower always runs the exact-fp32 kernels.
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mcm_debug_workspace.h"
#include "../../include/mcm_score_stream.h"
#include "bank_sim.hpp"
#include "common.hpp"

namespace {

thread_local std::string g_create_err;

struct Param {
  std::vector<int64_t> shape;
  int64_t numel = 0;
  float* dev = nullptr;
  bool set = false;
};

struct LayerW {
  void *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;  // operand dtype
  float *bqkv = nullptr;                                               // [3D] packed
  const float *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;               // fp32 masters
};

struct Tower {
  int D = 0, heads = 0, layers = 0, ff = 0;
  int prec = MCM_PREC_BF16;  // operand mode of this tower's GEMMs / attention / LayerNorm output
  std::vector<LayerW> L;
  bool split = false;        // GEMM weights held as W_hi + W_lo (GemmArgs::ksplit; include/mcm.h MCM_WEIGHTS_*)
  int act = MCM_ACT_QUICK_GELU;  // MLP activation (mcm_config.v_hidden_act / t_hidden_act): which fc1 epilogue run_layers asks for
};

struct EvPair {
  hipEvent_t a, b;
  int kc, kc2;  // kc2: a sub-class of kc that also gets this launch (MCM_KC_GEMM_*), -1 = none
};

// A handle without the A/B arms' fields: mcm_handle (below, at the include of the arms) is this and nothing else in the
// shipped library, this plus the arms' workspace in the A/B builds
struct HandleCore {
  mcm_config cfg;
  std::map<std::string, Param> params;
  bool finalized = false;
  Tower vis, txt;
  void* wpatch = nullptr;  // [v_width, kpad] operand dtype ([v_width, 2 kpad] split)
  void* wproj = nullptr;   // visual_projection.weight [proj_dim, v_width] in the vision tower's operand form (the local pass's projection GEMM)
  uint64_t w_inexact = 0;  // vision GEMM-weight elements that are not operand-dtype numbers (mcm_finalize_weights)
  int kpad = 0, np = 0, ntok = 0;
  // workspace
  float* x = nullptr;
  void *ln = nullptr, *qkv = nullptr, *att = nullptr, *hbuf = nullptr, *patches = nullptr;
  float* feat = nullptr;          // [max_batch, proj_dim] scratch for mcm_score
  int32_t *ids_dev = nullptr, *rowidx_dev = nullptr;
  int32_t *ids_pin = nullptr, *rowidx_pin = nullptr;
  // mcm_resize_crop_u8 geometry: a ring of PREP_RING pinned staging buffers (max_batch entries each) so that a call never
  // has to drain the stream before it may write the next batch's geometry; prep_ev[k] = "the copy out of slot k is done"
  static constexpr int PREP_RING = 4;
  PrepImage *prep_pin = nullptr, *prep_dev = nullptr;
  int32_t* prep_coef = nullptr;  // PREP_RING x prep_coef_bytes: the resize kernel's coefficient tables (allocated by the first call)
  // mcm_jpeg_reconstruct: per-image records + quantisation tables through the same kind of ring (allocated by the first
  // call), and the sample-plane workspace (grown on demand; one per handle: the kernels of consecutive calls are stream-ordered)
  char* jpg_pin = nullptr;
  char* jpg_dev = nullptr;
  bool jpg_ready = false;
  hipEvent_t jpg_ev[PREP_RING] = {nullptr, nullptr, nullptr, nullptr};
  unsigned jpg_next = 0;
  uint8_t* jpg_planes = nullptr;
  size_t jpg_planes_bytes = 0;
  hipEvent_t prep_ev[PREP_RING] = {nullptr, nullptr, nullptr, nullptr};
  unsigned prep_next = 0;
  int64_t max_rows = 0;
  int x2_batch = 0;    // largest batch of the split-activation arm (= max_batch on fp16 handles, whose activation buffers are sized for it; 0: not fp16)
  size_t hbuf_bytes = 0;
  size_t x_bytes = 0, ln_bytes = 0, qkv_bytes = 0, att_bytes = 0, patches_bytes = 0;  // allocated sizes (mcm_debug_workspace_fill)
  std::vector<void*> owned;       // every hipMalloc'd pointer
  // profiling
  bool prof = false;
  std::vector<EvPair> ev_pool;
  size_t ev_used = 0;
  double ms_acc[MCM_KC_COUNT] = {0};
  int64_t launches[MCM_KC_COUNT] = {0};
  double flops[MCM_KC_COUNT] = {0};
  bool flip = false;  // walk direction of the next kernel (next_dir)
  unsigned int* sat_dev = nullptr;  // sticky fp16 saturation counter (common.hpp sat_report)
  // sticky kernel-fault word: pinned host memory mapped into the device; a persistent kernel whose wait ran out of its budget
  // stores 1 there (attention.hip attn_ps_kernel) and every later compute call on the handle returns MCM_EHIP (check_ready)
  unsigned int* fault_pin = nullptr;
  unsigned int* fault_dev = nullptr;
  bool sat_on = true;
  std::string err;
};

int fail(HandleCore* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  else g_create_err = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                 \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return fail(h, MCM_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
  } while (0)

// The two argument rules every scoring entry repeats: a temperature is positive and finite, a pixel_format is one of MCM_PIXELS_*
bool bad_temperature(float T) { return !(T > 0.f) || !std::isfinite(T); }
int check_pixel_format(HandleCore* h, int32_t pixel_format) {
  if (pixel_format != MCM_PIXELS_F32_NCHW && pixel_format != MCM_PIXELS_U8_NHWC) return fail(h, MCM_EINVAL, "unknown pixel_format");
  return MCM_OK;
}

void add_param(HandleCore* h, const std::string& name, std::vector<int64_t> shape) {
  Param p;
  p.shape = shape;
  p.numel = 1;
  for (auto d : shape) p.numel *= d;
  h->params[name] = p;
}

void add_layer_params(HandleCore* h, const std::string& pre, int D, int ff) {
  for (const char* pr : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
    add_param(h, pre + ".self_attn." + pr + ".weight", {D, D});
    add_param(h, pre + ".self_attn." + pr + ".bias", {D});
  }
  for (const char* ln : {"layer_norm1", "layer_norm2"}) {
    add_param(h, pre + "." + ln + ".weight", {D});
    add_param(h, pre + "." + ln + ".bias", {D});
  }
  add_param(h, pre + ".mlp.fc1.weight", {ff, D});
  add_param(h, pre + ".mlp.fc1.bias", {ff});
  add_param(h, pre + ".mlp.fc2.weight", {D, ff});
  add_param(h, pre + ".mlp.fc2.bias", {D});
}

int dev_alloc(HandleCore* h, void** out, size_t bytes) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
  if (e != hipSuccess)
    return fail(h, MCM_ENOMEM, "hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
  h->owned.push_back(p);
  *out = p;
  return MCM_OK;
}

const float* W(HandleCore* h, const std::string& name) { return h->params.at(name).dev; }

// ---- profiling wrappers ---------------------------------------------------------------
struct Scope {
  HandleCore* h;
  hipStream_t s;
  int kc;
  EvPair* ev = nullptr;
  Scope(HandleCore* h_, hipStream_t s_, int kc_, double fl, int kc2 = -1) : h(h_), s(s_), kc(kc_) {
    if (!h->prof) return;
    if (h->ev_used == h->ev_pool.size()) {
      EvPair e;
      (void)hipEventCreate(&e.a);
      (void)hipEventCreate(&e.b);
      h->ev_pool.push_back(e);
    }
    ev = &h->ev_pool[h->ev_used++];
    ev->kc = kc;
    ev->kc2 = kc2;
    h->launches[kc] += 1;
    h->flops[kc] += fl;
    if (kc2 >= 0) {
      h->launches[kc2] += 1;
      h->flops[kc2] += fl;
    }
    (void)hipEventRecord(ev->a, s);
  }
  ~Scope() {
    if (ev) (void)hipEventRecord(ev->b, s);
  }
};

// Consecutive kernels of a tower walk their rows in opposite directions: a producer's last rows are
// the ones still in L2 / Infinity Cache, so its consumer starts there (results do not depend on the
// order).  `flip` alternates per launch.  Measured: LayerNorm 2.19 -> 1.99 ms per step (it reads the
// residual stream the previous GEMM just wrote), +0.9 % end to end.
bool next_dir(HandleCore* h) {
  h->flip = !h->flip;
  return h->flip;
}
// rows of a dense activation GEMM as gemm() runs it (whole 256-row tiles when the workspace has them)
int64_t padded_rows(const HandleCore* h, int M) {
  const int64_t mp = ((int64_t)M + 255) / 256 * 256;
  return mp <= h->max_rows ? mp : M;
}

}  // namespace

// ---- the A/B arms ---------------------------------------------------------------------
// Everything the closed experiments need on the host (their switches, workspace, per-call planning and launches) is in
// mcm_api_arms.hpp, which only the A/B builds include, as gemm.hip does with gemm_arms.hpp.  The shipped library has what
// follows in its place: no arm field in the handle, the two switches shipped code reads as constants, and an `Arms` whose
// every answer is a compile-time "no", so that each call site below folds to the shipped launches.
#if defined(MCM_HARNESS) || defined(MCM_LN_FOLD) || defined(MCM_LN_TAIL)
#define MCM_API_ARMS 1
#include "mcm_api_arms.hpp"
#else
struct mcm_handle : HandleCore {};
namespace {
constexpr int g_patch_fold = 1, g_resize_fused_only = 0;
struct Arms {
  template <class... A> Arms(A&&...) {}
  template <class... A> void consumer(A&&...) {}
  template <class... A> static constexpr bool qkv_attention(A&&...) { return false; }
  template <class... A> static constexpr bool resid_ln(A&&...) { return false; }
  template <class... A> static constexpr bool column_blocks(A&&...) { return false; }
  template <class... A> static constexpr bool skip_layernorm(A&&...) { return false; }
  template <class... A> static constexpr int create(A&&...) { return MCM_OK; }
  template <class... A> static constexpr int build_layer(A&&...) { return MCM_OK; }
};
}  // namespace
#endif

namespace {

hipError_t gemm(mcm_handle* h, hipStream_t s, int prec, int epi, const GemmArgs& a_in) {
  hipError_t e = hipSuccess;
  if (Arms::column_blocks(h, s, prec, epi, a_in, e)) return e;
  GemmArgs a = a_in;
  a.rev = next_dir(h) ? 1 : 0;
  a.sat = h->sat_on ? h->sat_dev : nullptr;
  // the four whole-batch shapes of an encoder layer also get a class of their own (out-proj is the HBM-bound one:
  // bench.py roofline_hbm_kernels); small launches (CLS-only last layer, short prompt banks) count in MCM_KC_GEMM only
  int shape = -1;
  if (a.M > 4096)
    shape = (epi == EPI_STORE || epi == EPI_STORE_X2) ? MCM_KC_GEMM_QKV : epi_gelu(epi) ? MCM_KC_GEMM_FC1
          : epi == EPI_RESID ? (a.N == a.K ? MCM_KC_GEMM_OUTPROJ : MCM_KC_GEMM_FC2) : -1;
  Scope sc(h, s, MCM_KC_GEMM, 2.0 * a.M * (double)a.N * a.K, shape);  // algorithmic FLOP: the logical K, split or not
  // Row padding into the workspace: the ping-pong kernel takes problems made of whole 256-row tiles only, so a
  // dense activation GEMM whose M is not a multiple of 256 is run on M rounded up.  The extra rows exist (every
  // activation buffer is allocated in whole 256-row tiles), every output row depends on its own input row only, and
  // the pad rows' results are never read: same bits for the real rows, and batches that are not multiples of 256
  // images (any batch at ViT-L/14's 257 tokens but 256 k; ragged last batches) get the fast kernel.  What the pad rows
  // HOLD is arbitrary: mcm_create zeroes them once, but the towers share the buffers, so a text pass pads into the
  // 16-bit rows the last vision batch left and reads them as fp32, NaN included.  That is harmless for the outputs in
  // every mode; only the fp16 saturation watch could see such rows, which is why vision_front zeroes them per batch.
  // tests/test_gpu_handle_history.py holds both, over a workspace filled with NaN and with near-saturation patterns.
  const bool from_row0 = a.x == h->ln || a.x == h->att || a.x == h->hbuf;  // not a chunk that starts mid-buffer
  if (epi != EPI_PATCH && from_row0 && a.M % 256 != 0 && a.N % 256 == 0 && a.ldx == a.K && a.ldo == a.N)
    a.M = (int)padded_rows(h, a.M);
  if (a.ksplit) a.K *= 2;  // the callers describe the logical problem; the split image has 2 K columns per row
  if (a.xsplit) a.ldx *= 2;           // ... and so have the rows of a split X
  if (epi_x2(epi)) a.ldo *= 2;        // ... and of a split output
  return launch_gemm(prec, epi, a, s);
}
hipError_t lnorm(mcm_handle* h, hipStream_t s, int prec, const float* x, const float* g, const float* b,
                 void* y, int M, int D, bool out_f32, bool split = false) {
  Scope sc(h, s, MCM_KC_LAYERNORM, 8.0 * M * D);
  if (split)
    return launch_layernorm(prec, x, g, b, y, M, D, h->cfg.ln_eps, false, s, 0, 0, next_dir(h),
                            h->sat_on ? h->sat_dev : nullptr, true);
  hipError_t e = hipSuccess;
  if (Arms::skip_layernorm(h, s, prec, M, D, out_f32, e)) return e;
  return launch_layernorm(prec, x, g, b, y, M, D, h->cfg.ln_eps, out_f32, s, 0, 0, next_dir(h),
                          h->sat_on ? h->sat_dev : nullptr);
}
// seq0: first sequence of the launch (a chunk of the batch starts there)
// hd: head_dim (64, or 80 in ViT-H/14's vision tower)
hipError_t attn(mcm_handle* h, hipStream_t s, int prec, int nseq, int L, int heads, int hd, bool causal,
                int qrows = 0, int seq0 = 0, int hm = 0, bool split = false) {
  const int q = qrows > 0 ? qrows : L;
  Scope sc(h, s, MCM_KC_ATTENTION, 4.0 * nseq * heads * (double)q * L * hd * (causal ? 0.5 : 1.0));
  if (split) return launch_attention(prec, h->qkv, h->att, nseq, L, heads, hd, causal, qrows, s, next_dir(h), 0, true);
  const size_t es = prec_esize(prec), D = (size_t)heads * hd, row0 = (size_t)seq0 * L;
  return launch_attention(prec, (const char*)h->qkv + row0 * 3 * D * es, (char*)h->att + row0 * D * es, nseq, L,
                          heads, hd, causal, qrows, s, next_dir(h), hm, false, h->fault_dev);
}
hipError_t lnorm_strided(mcm_handle* h, hipStream_t s, int prec, const float* x, const float* g,
                         const float* b, void* y, int M, int D, size_t xs, size_t ys, bool split = false) {
  Scope sc(h, s, MCM_KC_LAYERNORM, 8.0 * M * D);
  return launch_layernorm(prec, x, g, b, y, M, D, h->cfg.ln_eps, false, s, xs, ys, false,
                          h->sat_on ? h->sat_dev : nullptr, split);
}

// CLIPEncoderLayer.forward ×layers on x [nseq*L, D] (fp32, in place).
// pooled_row0: the caller consumes only row 0 of every sequence (CLS pooling, HF
// modeling_clip.py:649-651).  The last layer then computes K/V for all tokens but Q, the
// attention output, out_proj, LN2 and the MLP for row 0 only — identical results for the
// consumed rows (every op after attention is row-wise), 1/12 less work for a 12-layer tower.
// ln1_of_layer0_done: the caller has already produced layer 0's layer_norm1 output in h->ln (the vision tower fuses it
// with pre_layrnorm, launch_layernorm_pre)
// x2 (fp16 vision tower; the split-activation arm, mcm_score_x2): every activation that feeds an MFMA — LayerNorm outputs,
// q / k / v, the attention output, the QuickGELU output — is carried as a split image (hi + lo, twice the columns) and every
// GEMM runs GemmArgs::xsplit; the residual stream, LayerNorm statistics and softmax are fp32 as always.
// arms: the A/B builds' per-call plan (mcm_api_arms.hpp), asked at three points of a whole-batch layer; in the shipped
// library every answer is "no" and the layer below is all there is.
int run_layers(mcm_handle* h, hipStream_t s, const Tower& t, int nseq, int L, bool causal,
               bool pooled_row0, bool ln1_of_layer0_done = false, bool x2 = false) {
  const int M = nseq * L, D = t.D, P = t.prec;
  const int es = prec_esize(P);
  const int ks = t.split ? 1 : 0;
  const int xs = x2 ? 1 : 0;
  const int hd = D / t.heads;  // 64, or 80 (mcm_create admits nothing else)
  const bool erf = t.act == MCM_ACT_GELU;  // the tower's MLP activation: exact GELU (OpenCLIP-trained) or QuickGELU (OpenAI)
  const int epi_store = x2 ? EPI_STORE_X2 : EPI_STORE;
  const int epi_act = erf ? (x2 ? EPI_GELU_ERF_X2 : EPI_GELU_ERF) : (x2 ? EPI_GELU_X2 : EPI_GELU);
  const size_t wrow = (size_t)D * es * (t.split ? 2 : 1);  // bytes per row of a [*, D] weight image
  Arms arms(h, s, t, nseq, L, pooled_row0, x2);
  int rc = MCM_OK;
  bool ln1_done = ln1_of_layer0_done;  // h->ln already holds this layer's layer_norm1
  for (int l = 0; l < t.layers; ++l) {
    const LayerW& w = t.L[l];
    const bool cls = pooled_row0 && l == t.layers - 1 && L > 1;
    if (!ln1_done) HIP_TRY(h, lnorm(h, s, P, h->x, w.ln1w, w.ln1b, h->ln, M, D, false, x2));
    if (!cls) {
      GemmArgs a{};
      a.x = h->ln; a.w = w.wqkv; a.bias = w.bqkv; a.out = h->qkv;
      a.M = M; a.N = 3 * D; a.K = D; a.ldx = D; a.ldo = 3 * D; a.ksplit = ks; a.xsplit = xs;
      arms.consumer(a, l, false);
      if (!arms.qkv_attention(a, epi_store, causal, rc)) {
        HIP_TRY(h, gemm(h, s, P, epi_store, a));
        HIP_TRY(h, attn(h, s, P, nseq, L, t.heads, hd, causal, 0, 0, 0, x2));
      }
    } else {
      GemmArgs kv{};  // K and V of every token: weight rows [D, 3D), output columns [D, 3D)
      kv.x = h->ln; kv.w = (const char*)w.wqkv + (size_t)D * wrow; kv.bias = w.bqkv + D;
      kv.out = (char*)h->qkv + (size_t)D * es * (1 + xs);  // (split rows: D logical columns are 2 D elements)
      kv.M = M; kv.N = 2 * D; kv.K = D; kv.ldx = D; kv.ldo = 3 * D; kv.ksplit = ks; kv.xsplit = xs;
      HIP_TRY(h, gemm(h, s, P, epi_store, kv));
      GemmArgs q{};   // Q of row 0 of every sequence (row stride L*D in, L*3D out)
      q.x = h->ln; q.w = w.wqkv; q.bias = w.bqkv; q.out = h->qkv;
      q.M = nseq; q.N = D; q.K = D; q.ldx = L * D; q.ldo = L * 3 * D; q.ksplit = ks; q.xsplit = xs;
      HIP_TRY(h, gemm(h, s, P, epi_store, q));
      HIP_TRY(h, attn(h, s, P, nseq, L, t.heads, hd, causal, 1, 0, 0, x2));
    }
    if (rc) return rc;
    const int Mr = cls ? nseq : M;            // rows that continue
    const int rs = cls ? L * D : D;           // their stride in x / att
    GemmArgs o{};
    o.x = h->att; o.w = w.wo; o.bias = w.bo; o.resid = h->x;
    o.M = Mr; o.N = D; o.K = D; o.ldx = rs; o.ldo = rs; o.ksplit = ks; o.xsplit = xs;
    if (cls || !arms.resid_ln(o, l, false, w.ln2w, w.ln2b, rc)) {  // out-proj, then layer_norm2
      HIP_TRY(h, gemm(h, s, P, EPI_RESID, o));
      if (!cls) HIP_TRY(h, lnorm(h, s, P, h->x, w.ln2w, w.ln2b, h->ln, M, D, false, x2));
      else HIP_TRY(h, lnorm_strided(h, s, P, h->x, w.ln2w, w.ln2b, h->ln, Mr, D, (size_t)rs, (size_t)D * (1 + xs), x2));
    }
    if (rc) return rc;
    GemmArgs f1{};
    f1.x = h->ln; f1.w = w.w1; f1.bias = w.b1; f1.out = h->hbuf;
    f1.M = Mr; f1.N = t.ff; f1.K = D; f1.ldx = D; f1.ldo = t.ff; f1.ksplit = ks; f1.xsplit = xs;
    arms.consumer(f1, l, true);
    HIP_TRY(h, gemm(h, s, P, epi_act, f1));
    GemmArgs f2{};
    f2.x = h->hbuf; f2.w = w.w2; f2.bias = w.b2; f2.resid = h->x;
    f2.M = Mr; f2.N = D; f2.K = t.ff; f2.ldx = t.ff; f2.ldo = rs; f2.ksplit = ks; f2.xsplit = xs;
    // fc2; the next layer's layer_norm1 is that layer's first launch unless an arm produces it here
    ln1_done = !cls && l + 1 < t.layers && arms.resid_ln(f2, l, true, t.L[l + 1].ln1w, t.L[l + 1].ln1b, rc);
    if (!ln1_done) HIP_TRY(h, gemm(h, s, P, EPI_RESID, f2));
    if (rc) return rc;
  }
  return MCM_OK;
}

int build_tower(mcm_handle* h, Tower& t, const std::string& tower, hipStream_t s) {
  const int prec = t.prec, D = t.D, ff = t.ff;
  const int es = prec_esize(prec) * (t.split ? 2 : 1);  // bytes per logical weight element
  auto cvt = [&](const float* src, void* dst, int rows, int cols) {
    return t.split ? launch_cvt_weight_split(prec, src, dst, rows, cols, cols, s)
                   : launch_cvt_weight(prec, src, dst, rows, cols, cols, s);
  };
  t.L.resize(t.layers);
  for (int l = 0; l < t.layers; ++l) {
    LayerW& w = t.L[l];
    const std::string pre = tower + ".encoder.layers." + std::to_string(l);
    int rc;
    if ((rc = dev_alloc(h, &w.wqkv, (size_t)3 * D * D * es))) return rc;
    if ((rc = dev_alloc(h, &w.wo, (size_t)D * D * es))) return rc;
    if ((rc = dev_alloc(h, &w.w1, (size_t)ff * D * es))) return rc;
    if ((rc = dev_alloc(h, &w.w2, (size_t)D * ff * es))) return rc;
    if ((rc = dev_alloc(h, (void**)&w.bqkv, (size_t)3 * D * sizeof(float)))) return rc;
    const char* parts[3] = {"q_proj", "k_proj", "v_proj"};
    for (int p = 0; p < 3; ++p) {
      HIP_TRY(h, cvt(W(h, pre + ".self_attn." + parts[p] + ".weight"), (char*)w.wqkv + (size_t)p * D * D * es, D, D));
      HIP_TRY(h, hipMemcpyAsync(w.bqkv + (size_t)p * D, W(h, pre + ".self_attn." + parts[p] + ".bias"),
                                (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(h, cvt(W(h, pre + ".self_attn.out_proj.weight"), w.wo, D, D));
    HIP_TRY(h, cvt(W(h, pre + ".mlp.fc1.weight"), w.w1, ff, D));
    HIP_TRY(h, cvt(W(h, pre + ".mlp.fc2.weight"), w.w2, D, ff));
    if ((rc = Arms::build_layer(h, t, l, pre, s))) return rc;
    w.bo = W(h, pre + ".self_attn.out_proj.bias");
    w.b1 = W(h, pre + ".mlp.fc1.bias");
    w.b2 = W(h, pre + ".mlp.fc2.bias");
    w.ln1w = W(h, pre + ".layer_norm1.weight");
    w.ln1b = W(h, pre + ".layer_norm1.bias");
    w.ln2w = W(h, pre + ".layer_norm2.weight");
    w.ln2b = W(h, pre + ".layer_norm2.bias");
  }
  return MCM_OK;
}

int check_ready(mcm_handle* h) {
  if (!h) return MCM_EINVAL;
  if (!h->finalized) return fail(h, MCM_ENOWEIGHT, "mcm_finalize_weights has not been called");
  if (h->fault_pin && *(volatile unsigned int*)h->fault_pin)
    return fail(h, MCM_EHIP, "a persistent kernel of an earlier call gave up a wait that exceeded its poll budget (attn_ps_kernel): "
                             "that call's results are invalid and the handle is unusable — mcm_kernel_faults");
  return MCM_OK;
}

}  // namespace

extern "C" {

int mcm_abi_version(void) { return MCM_ABI_VERSION; }

const char* mcm_last_error(const mcm_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int mcm_create(const mcm_config* cfg, mcm_handle** out) {
  if (!cfg || !out) return fail(nullptr, MCM_EINVAL, "null argument");
  if (cfg->abi_version != MCM_ABI_VERSION) return fail(nullptr, MCM_EINVAL, "ABI version mismatch");
  const mcm_config& c = *cfg;
  if (c.precision != MCM_PREC_BF16 && c.precision != MCM_PREC_F32 && c.precision != MCM_PREC_F16)
    return fail(nullptr, MCM_EINVAL, "unknown precision");
  if (c.weight_operands < MCM_WEIGHTS_AUTO || c.weight_operands > MCM_WEIGHTS_SPLIT)
    return fail(nullptr, MCM_EINVAL, "unknown weight_operands");
  if ((c.v_hidden_act != MCM_ACT_QUICK_GELU && c.v_hidden_act != MCM_ACT_GELU) ||
      (c.t_hidden_act != MCM_ACT_QUICK_GELU && c.t_hidden_act != MCM_ACT_GELU))
    return fail(nullptr, MCM_EINVAL, "unknown hidden_act (MCM_ACT_QUICK_GELU or MCM_ACT_GELU)");
  if (c.v_heads <= 0 || c.t_heads <= 0 || (c.v_width != c.v_heads * 64 && c.v_width != c.v_heads * 80) ||
      c.t_width != c.t_heads * 64)
    return fail(nullptr, MCM_EINVAL, "head_dim must be 64 or 80 in the vision tower (attn_hd80_kernel) and 64 in the text tower");
  if (c.patch_size <= 0 || c.image_size % c.patch_size)
    return fail(nullptr, MCM_EINVAL, "image_size must be a multiple of patch_size");
  if (c.v_width % 64 || c.t_width % 64 || c.v_mlp % 64 || c.t_mlp % 64 || c.v_width > 1280 ||
      c.t_width > 1024 || c.proj_dim % 4 || c.proj_dim > 1024)
    return fail(nullptr, MCM_EINVAL, "widths must be multiples of 64, v_width <= 1280, t_width <= 1024; proj_dim % 4 == 0, <= 1024");
  if (c.max_batch <= 0 || c.max_prompt_tokens <= 0 || c.max_positions <= 0 ||
      c.max_prompt_tokens < c.max_positions)
    return fail(nullptr, MCM_EINVAL, "bad workspace bounds");
  // a tower without layers is not a CLIP tower: the first layer's LayerNorm is fused into the front of each tower, and the last
  // one is the CLS-only / pooled-row form, so there is no zero-layer path to fall back to
  if (c.v_layers < 1 || c.t_layers < 1) return fail(nullptr, MCM_EINVAL, "v_layers and t_layers must be at least 1");
  // the text tower's attention is the causal fp32 kernel, which keeps K, V and the logits of a head in LDS: a prompt of
  // max_positions tokens has to launch (attention.hip attn_f32_kernel)
  if (c.max_positions > attention_causal_f32_max_len())
    return fail(nullptr, MCM_EINVAL, "max_positions exceeds " + std::to_string(attention_causal_f32_max_len()) +
                                         ", the longest prompt the causal fp32 attention launches");
  {
    const int g = c.image_size / c.patch_size;
    // attention's ceiling (attention.hip LONG_MAX_L): 288 tokens keep K and V of a head in LDS, up to 1025 stream them
    if (g * g + 1 > 1025) return fail(nullptr, MCM_EINVAL, "more than 1025 vision tokens");
  }
  hipError_t e = hipSetDevice(c.device);
  if (e != hipSuccess) return fail(nullptr, MCM_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

  mcm_handle* h = new mcm_handle();
  h->cfg = c;
  const int g = c.image_size / c.patch_size;
  h->np = g * g;
  h->ntok = h->np + 1;
  const int es = prec_esize(c.precision);
  const int kreal = 3 * c.patch_size * c.patch_size;
  const int kalign = 128 / es;
  h->kpad = (kreal + kalign - 1) / kalign * kalign;
  // The text tower always runs in exact fp32 (MCM_PREC_F32 kernels), whatever cfg.precision says: the
  // prompt bank is encoded once per dataset, off the hot loop, and a bank rounded to 16-bit operands
  // is a FIXED perturbation of every cosine of every image — it shifts AUROC / FPR95 systematically
  // instead of averaging out.  cfg.precision selects the vision tower's operand mode.
  h->vis = Tower{c.v_width, c.v_heads, c.v_layers, c.v_mlp, c.precision, {}};
  h->txt = Tower{c.t_width, c.t_heads, c.t_layers, c.t_mlp, MCM_PREC_F32, {}};
  h->vis.act = c.v_hidden_act;
  h->txt.act = c.t_hidden_act;

  // parameter registry (HF state_dict names)
  add_param(h, "vision_model.embeddings.class_embedding", {c.v_width});
  add_param(h, "vision_model.embeddings.patch_embedding.weight", {c.v_width, 3, c.patch_size, c.patch_size});
  add_param(h, "vision_model.embeddings.position_embedding.weight", {h->ntok, c.v_width});
  add_param(h, "vision_model.pre_layrnorm.weight", {c.v_width});
  add_param(h, "vision_model.pre_layrnorm.bias", {c.v_width});
  for (int l = 0; l < c.v_layers; ++l)
    add_layer_params(h, "vision_model.encoder.layers." + std::to_string(l), c.v_width, c.v_mlp);
  add_param(h, "vision_model.post_layernorm.weight", {c.v_width});
  add_param(h, "vision_model.post_layernorm.bias", {c.v_width});
  add_param(h, "visual_projection.weight", {c.proj_dim, c.v_width});
  add_param(h, "text_model.embeddings.token_embedding.weight", {c.vocab_size, c.t_width});
  add_param(h, "text_model.embeddings.position_embedding.weight", {c.max_positions, c.t_width});
  for (int l = 0; l < c.t_layers; ++l)
    add_layer_params(h, "text_model.encoder.layers." + std::to_string(l), c.t_width, c.t_mlp);
  add_param(h, "text_model.final_layer_norm.weight", {c.t_width});
  add_param(h, "text_model.final_layer_norm.bias", {c.t_width});
  add_param(h, "text_projection.weight", {c.proj_dim, c.t_width});

  int rc = MCM_OK;
  for (auto& kv : h->params) {
    if ((rc = dev_alloc(h, (void**)&kv.second.dev, (size_t)kv.second.numel * sizeof(float)))) break;
  }
  // activation workspace
  // activation rows: whole 256-row GEMM tiles (see gemm(): problems are padded up into these rows)
  const int64_t mv = ((int64_t)c.max_batch * h->ntok + 255) / 256 * 256, mt = ((int64_t)c.max_prompt_tokens + 255) / 256 * 256;
  h->max_rows = mv > mt ? mv : mt;
  // shared by both towers: vision rows in the operand dtype of cfg.precision, text rows in fp32
  // fp16 handles: the split-activation arm (mcm_score_x2) carries every such row as hi + lo — twice the width — and runs at the
  // same batch as the fp16 arm, so these buffers are allocated at twice the bytes (B/16, batch 512: +1.5 GB of the part's 288)
  // cfg.x2_max_batch (ABI 4): 0 = the arm runs at the full batch (the buffers at twice the bytes), n > 0 = at most n images per
  // x2 call (the buffers hold max(max_batch rows, 2 x the x2 rows)), < 0 = no split workspace at all
  if (c.precision == MCM_PREC_F16 && c.x2_max_batch >= 0)
    h->x2_batch = c.x2_max_batch == 0 || c.x2_max_batch > c.max_batch ? c.max_batch : c.x2_max_batch;
  const int64_t mvx = ((int64_t)h->x2_batch * h->ntok + 255) / 256 * 256;   // token rows of the largest x2 batch (0: none)
  auto both = [&](int64_t vcols, int64_t tcols) {
    const size_t a = (size_t)mv * vcols * es, ax = (size_t)mvx * vcols * es * 2, b = (size_t)mt * tcols * sizeof(float);
    return std::max(std::max(a, ax), b);
  };
  const int64_t dmax = c.v_width > c.t_width ? c.v_width : c.t_width;
  const size_t xb = (size_t)h->max_rows * dmax * sizeof(float), lnb = both(c.v_width, c.t_width),
               qkvb = both(3 * (int64_t)c.v_width, 3 * (int64_t)c.t_width), attb = both(c.v_width, c.t_width);
  h->x_bytes = xb; h->ln_bytes = lnb; h->qkv_bytes = qkvb; h->att_bytes = attb;
  if (!rc) rc = dev_alloc(h, (void**)&h->x, xb);
  if (!rc) rc = dev_alloc(h, &h->ln, lnb);
  if (!rc) rc = dev_alloc(h, &h->qkv, qkvb);
  if (!rc) rc = dev_alloc(h, &h->att, attb);
  h->hbuf_bytes = both(c.v_mlp, c.t_mlp);
  if (!rc) rc = dev_alloc(h, &h->hbuf, h->hbuf_bytes);
  // zeroed once (a ragged vision batch zeroes its pad rows again: encode_image_impl, "Pad rows")
  if (!rc && (hipMemset(h->x, 0, xb) != hipSuccess || hipMemset(h->ln, 0, lnb) != hipSuccess ||
              hipMemset(h->qkv, 0, qkvb) != hipSuccess || hipMemset(h->att, 0, attb) != hipSuccess ||
              hipMemset(h->hbuf, 0, h->hbuf_bytes) != hipSuccess))
    rc = fail(h, MCM_EHIP, "hipMemset of the activation workspace");
  h->patches_bytes = std::max((size_t)c.max_batch * h->np * h->kpad * es, (size_t)h->x2_batch * h->np * h->kpad * es * 2);
  if (!rc) rc = dev_alloc(h, &h->patches, h->patches_bytes);
  if (!rc) rc = dev_alloc(h, (void**)&h->feat, (size_t)c.max_batch * c.proj_dim * sizeof(float));
  if (!rc) rc = dev_alloc(h, (void**)&h->ids_dev, (size_t)mt * sizeof(int32_t));
  if (!rc) rc = dev_alloc(h, (void**)&h->rowidx_dev, (size_t)mt * sizeof(int32_t));
  if (!rc) rc = dev_alloc(h, &h->wpatch, (size_t)c.v_width * h->kpad * es * 2);  // (x 2: room for the split image)
  if (!rc && hipHostMalloc((void**)&h->ids_pin, (size_t)mt * sizeof(int32_t)) != hipSuccess)
    rc = fail(h, MCM_ENOMEM, "hipHostMalloc ids");
  if (!rc && hipHostMalloc((void**)&h->rowidx_pin, (size_t)mt * sizeof(int32_t)) != hipSuccess)
    rc = fail(h, MCM_ENOMEM, "hipHostMalloc rowidx");
  if (!rc) rc = dev_alloc(h, (void**)&h->prep_dev, (size_t)mcm_handle::PREP_RING * c.max_batch * sizeof(PrepImage));
  if (!rc) rc = Arms::create(h, mv);
  if (!rc) rc = dev_alloc(h, (void**)&h->sat_dev, 16);
  if (!rc && hipMemset(h->sat_dev, 0, 16) != hipSuccess) rc = fail(h, MCM_EHIP, "hipMemset saturation counter");
  if (!rc && hipHostMalloc((void**)&h->fault_pin, 64, hipHostMallocMapped) != hipSuccess) rc = fail(h, MCM_ENOMEM, "hipHostMalloc fault word");
  if (!rc) {
    memset(h->fault_pin, 0, 64);
    if (hipHostGetDevicePointer((void**)&h->fault_dev, h->fault_pin, 0) != hipSuccess) rc = fail(h, MCM_EHIP, "hipHostGetDevicePointer fault word");
  }
  if (!rc && hipHostMalloc((void**)&h->prep_pin, (size_t)mcm_handle::PREP_RING * c.max_batch * sizeof(PrepImage)) != hipSuccess)
    rc = fail(h, MCM_ENOMEM, "hipHostMalloc prep");
  for (int k = 0; !rc && k < mcm_handle::PREP_RING; ++k)
    if (hipEventCreateWithFlags(&h->prep_ev[k], hipEventDisableTiming) != hipSuccess) rc = fail(h, MCM_EHIP, "hipEventCreate prep");
  if (rc) {
    g_create_err = h->err;
    mcm_destroy(h);
    return rc;
  }
  *out = h;
  return MCM_OK;
}

void mcm_destroy(mcm_handle* h) {
  if (!h) return;
  (void)hipDeviceSynchronize();
  for (void* p : h->owned) (void)hipFree(p);
  if (h->ids_pin) (void)hipHostFree(h->ids_pin);
  if (h->rowidx_pin) (void)hipHostFree(h->rowidx_pin);
  if (h->prep_pin) (void)hipHostFree(h->prep_pin);
  if (h->fault_pin) (void)hipHostFree(h->fault_pin);
  if (h->jpg_pin) (void)hipHostFree(h->jpg_pin);
  if (h->jpg_planes) (void)hipFree(h->jpg_planes);
  for (auto& e : h->jpg_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : h->prep_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_pool) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  delete h;
}

namespace {
float half_bits_to_float(uint16_t v) {  // IEEE binary16 -> binary32, exact (host side of mcm_set_weight)
  const uint32_t sign = (uint32_t)(v & 0x8000u) << 16, e = (v >> 10) & 0x1fu, m = v & 0x3ffu;
  uint32_t u;
  if (e == 0) {
    if (m == 0) {
      u = sign;
    } else {  // subnormal: m * 2^-24
      const float f = (float)m * (1.0f / 16777216.0f);
      uint32_t fu;
      memcpy(&fu, &f, 4);
      u = sign | fu;
    }
  } else if (e == 31) {
    u = sign | 0x7f800000u | (m << 13);
  } else {
    u = sign | ((e + 112u) << 23) | (m << 13);
  }
  float out;
  memcpy(&out, &u, 4);
  return out;
}
}  // namespace

int mcm_set_weight(mcm_handle* h, const char* hf_name, const void* host_ptr, int32_t dtype, const int64_t* shape,
                   int32_t ndim) {
  if (!h || !hf_name || !host_ptr || (ndim > 0 && !shape)) return fail(h, MCM_EINVAL, "null argument");
  if (dtype != MCM_DT_F32 && dtype != MCM_DT_F16 && dtype != MCM_DT_BF16) return fail(h, MCM_EINVAL, "unknown dtype");
  auto it = h->params.find(hf_name);
  if (it == h->params.end()) return fail(h, MCM_ENAME, std::string("unknown parameter ") + hf_name);
  Param& p = it->second;
  bool ok = (size_t)ndim == p.shape.size();
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == p.shape[i];
  if (!ok) return fail(h, MCM_ESHAPE, std::string("shape mismatch for ") + hf_name);
  const void* src = host_ptr;
  std::vector<float> wide;
  if (dtype != MCM_DT_F32) {  // the fp32 master is the exact widening of a 16-bit checkpoint value
    wide.resize((size_t)p.numel);
    const uint16_t* q = (const uint16_t*)host_ptr;
    for (int64_t i = 0; i < p.numel; ++i) {
      if (dtype == MCM_DT_F16) {
        wide[(size_t)i] = half_bits_to_float(q[i]);
      } else {
        const uint32_t u = (uint32_t)q[i] << 16;
        memcpy(&wide[(size_t)i], &u, 4);
      }
    }
    src = wide.data();
  }
  HIP_TRY(h, hipMemcpy(p.dev, src, (size_t)p.numel * sizeof(float), hipMemcpyHostToDevice));
  p.set = true;
  h->finalized = false;
  return MCM_OK;
}

int mcm_finalize_weights(mcm_handle* h) {
  if (!h) return MCM_EINVAL;
  for (auto& kv : h->params)
    if (!kv.second.set) return fail(h, MCM_ENOWEIGHT, "parameter never set: " + kv.first);
  if (!h->vis.L.empty()) return fail(h, MCM_EINVAL, "weights already finalized; create a new handle to reload");
  const mcm_config& c = h->cfg;
  // Which vision GEMM weights are NOT numbers of the operand dtype?  (include/mcm.h MCM_WEIGHTS_*: a weight that is one
  // is lossless as a single 16-bit operand; one that is not is rounded - unless the split form carries the remainder.)
  h->w_inexact = 0;
  if (c.precision != MCM_PREC_F32) {
    unsigned long long* cnt = nullptr;
    HIP_TRY(h, hipMalloc((void**)&cnt, sizeof(*cnt)));
    hipError_t e = hipMemset(cnt, 0, sizeof(*cnt));
    for (auto& kv : h->params) {
      const std::string& n = kv.first;
      const bool gemm_w = n.rfind("vision_model.", 0) == 0 && kv.second.shape.size() >= 2 &&
                          (n.find("_proj.weight") != std::string::npos || n.find(".mlp.fc") != std::string::npos ||
                           n.find("patch_embedding.weight") != std::string::npos);
      if (gemm_w && e == hipSuccess)
        e = launch_count_inexact(c.precision, kv.second.dev, (size_t)kv.second.numel, cnt, nullptr);
    }
    unsigned long long v = 0;
    if (e == hipSuccess) e = hipMemcpy(&v, cnt, sizeof(v), hipMemcpyDeviceToHost);
    (void)hipFree(cnt);
    if (e != hipSuccess) return fail(h, MCM_EHIP, std::string("counting inexact weights: ") + hipGetErrorString(e));
    h->w_inexact = v;
  }
  h->vis.split = c.precision != MCM_PREC_F32 &&
                 (c.weight_operands == MCM_WEIGHTS_SPLIT || (c.weight_operands == MCM_WEIGHTS_AUTO && h->w_inexact > 0));
  // operand copies are built from the fp32 masters once (pointers are stable afterwards)
  int rc;
  if ((rc = build_tower(h, h->vis, "vision_model", nullptr))) return rc;
  if ((rc = build_tower(h, h->txt, "text_model", nullptr))) return rc;
  const float* wp = W(h, "vision_model.embeddings.patch_embedding.weight");
  const int kreal = 3 * c.patch_size * c.patch_size;
  if (h->vis.split) HIP_TRY(h, launch_cvt_weight_split(c.precision, wp, h->wpatch, c.v_width, kreal, h->kpad, nullptr));
  else HIP_TRY(h, launch_cvt_weight(c.precision, wp, h->wpatch, c.v_width, kreal, h->kpad, nullptr));
  {  // the projection as a GEMM operand, split where the tower's weights are (mcm_encode_image_local; the pooled rows of
     // every other entry keep reading the fp32 master in launch_pool_project)
    const float* wv = W(h, "visual_projection.weight");
    const size_t wes = (size_t)prec_esize(c.precision) * (h->vis.split ? 2 : 1);
    if ((rc = dev_alloc(h, &h->wproj, (size_t)c.proj_dim * c.v_width * wes))) return rc;
    if (h->vis.split) HIP_TRY(h, launch_cvt_weight_split(c.precision, wv, h->wproj, c.proj_dim, c.v_width, c.v_width, nullptr));
    else HIP_TRY(h, launch_cvt_weight(c.precision, wv, h->wproj, c.proj_dim, c.v_width, c.v_width, nullptr));
  }
  HIP_TRY(h, hipDeviceSynchronize());
  h->finalized = true;
  return MCM_OK;
}

int mcm_weights_operand_exact(mcm_handle* h, uint64_t* inexact_host, int32_t* split_host) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (inexact_host) *inexact_host = h->w_inexact;
  if (split_host) *split_host = h->vis.split ? 1 : 0;
  return MCM_OK;
}

}  // extern "C" (re-opened below)

namespace {
// preprocess constants of the reference (utils/train_eval_util.py:27-28)
const float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
const float kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

// The front of the vision tower, up to the first encoder layer's QKV operand: pixels -> patch GEMM (+ position rows, written
// around the CLS slots of h->x) -> pad rows zeroed -> CLS row, pre_layrnorm (h->x, fp32) and layer 0's layer_norm1 (h->ln) in
// one pass.  stage_last: 1 = all of it (encode_image_impl); 0 = stop behind the patch GEMM (harness: mcm_debug_vision_front).
int vision_front(mcm_handle* h, hipStream_t s, const void* pixels_dev, bool u8, int32_t B, bool x2, int stage_last = 1) {
  const mcm_config& c = h->cfg;
  const int D = c.v_width;

  // fp32 NCHW pixels: the patch GEMM gathers its A operand from the image itself (gemm_p256_kernel, GemmArgs::px) when the
  // geometry allows (B/16, B/32 at batches the persistent kernel takes); otherwise — uint8 ingest, L/14's padded K, small
  // batches — patchify writes the patch matrix first
  const bool from_px = !u8 && !x2 && g_patch_fold &&
                       gemm_patch_takes_pixels(c.precision, B * h->np, D, h->kpad, c.patch_size, c.image_size);
  if (!from_px) {
    Scope sc(h, s, MCM_KC_PATCHIFY, 0.0);
    if (u8)
      HIP_TRY(h, launch_patchify_u8(c.precision, (const uint8_t*)pixels_dev, h->patches, B, c.image_size,
                                    c.patch_size, h->kpad, kClipMean, kClipStd, s, x2));
    else
      HIP_TRY(h, launch_patchify(c.precision, (const float*)pixels_dev, h->patches, B, c.image_size,
                                 c.patch_size, h->kpad, s, x2));
  }
  GemmArgs a{};
  a.px = from_px ? (const float*)pixels_dev : nullptr; a.img = c.image_size; a.patch = c.patch_size;
  a.x = h->patches; a.w = h->wpatch; a.bias = nullptr; a.out = h->x;
  a.pos = W(h, "vision_model.embeddings.position_embedding.weight");
  a.M = B * h->np; a.N = D; a.K = h->kpad; a.ldx = h->kpad; a.ldo = D; a.np = h->np; a.ksplit = h->vis.split ? 1 : 0;
  a.xsplit = x2 ? 1 : 0;
  HIP_TRY(h, gemm(h, s, c.precision, EPI_PATCH, a));
  if (stage_last < 1) return MCM_OK;
  {  // Pad rows.  gemm() runs the dense activation GEMMs on whole 256-row tiles; the rows between B * ntok and the next
     // multiple of 256 are computed and never read.  The buffers they live in are shared with the fp32 text tower, so
     // what they hold is arbitrary.  No output depends on them in any mode; the one thing that could is the fp16
     // saturation watch: fp32 bit patterns read as fp16 decode to large finite values and inf, a GEMM over such rows
     // packs out-of-range results, and the wave that packs them counts (NaN alone would not: the watch's fmaxf skips
     // it).  So a ragged batch zeroes the pad rows of every buffer a padded GEMM READS (x, ln, att, hbuf), and they
     // then only ever carry bias-only values; h->qkv is only ever written by a padded GEMM (attention reads the real
     // rows) and needs none.  bf16 and fp32 handles would return the same bits and counts without the zeroing: with
     // it removed tests/test_gpu_handle_history.py fails on fp16 handles alone, by the count, under the 0x7B fill.
    const int64_t M = (int64_t)B * h->ntok, mp = padded_rows(h, (int)M);
    if (mp > M) {
      const size_t es = (size_t)prec_esize(c.precision) * (x2 ? 2 : 1), pad = (size_t)(mp - M);
      // One kernel, not four hipMemsetAsync (ZeroSpans, common.hpp).  Observed with the memsets, on a fresh fp16 `tiny`
      // handle, whose pad rows mcm_create zeroed and no route writes: behind a GraphedScorer replay on the default stream
      // the pad rows of h->att, then of h->ln, held a non-zero pattern (|v| up to 55 136 as fp16) — the replayed memset
      // nodes had written it —, the next replay's fc1 packed rows 51 ... 255 of h->hbuf up to 65 056, and the count was 7
      // to 112 for a fresh handle's 0, the outputs untouched.  Rows and buffers are read back from the device; that the
      // runtime's memset nodes are at fault, and not this code, is supposed from the kernel in their place counting 0.
      const ZeroSpans z{{h->x + M * D, (char*)h->ln + (size_t)M * D * es, (char*)h->att + (size_t)M * D * es,
                         (char*)h->hbuf + (size_t)M * c.v_mlp * es},
                        {pad * D * sizeof(float) / 8, pad * D * es / 8, pad * D * es / 8, pad * c.v_mlp * es / 8}};
      HIP_TRY(h, launch_zero_spans(z, 4, s));
    }
  }
  // the CLS row of every image (class_embedding + position_embedding[0], HF :212-217) is produced inside the
  // LayerNorm pass below instead of by a launch of its own
  {  // pre_layrnorm (fp32, in place) and layer 0's layer_norm1 in one pass over x; a 1-layer tower whose only
     // layer is the CLS-only one still works: its layer_norm1 is over all rows either way
    Scope sc(h, s, MCM_KC_LAYERNORM, 16.0 * B * h->ntok * D);
    HIP_TRY(h, launch_layernorm_pre(c.precision, h->x, W(h, "vision_model.pre_layrnorm.weight"),
                                    W(h, "vision_model.pre_layrnorm.bias"), h->vis.L[0].ln1w, h->vis.L[0].ln1b,
                                    h->ln, B * h->ntok, D, c.ln_eps, s, next_dir(h),
                                    h->sat_on ? h->sat_dev : nullptr,
                                    W(h, "vision_model.embeddings.class_embedding"), a.pos, h->ntok, x2));
  }
  return MCM_OK;
}

// the argument checks of every image entry point
int check_image_call(mcm_handle* h, const void* pixels_dev, const void* out_dev, int32_t B, bool x2) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!pixels_dev || !out_dev) return fail(h, MCM_EINVAL, "null pointer");
  if (x2 && h->x2_batch <= 0) return fail(h, MCM_EINVAL, "the split-activation arm needs an fp16 handle created with a split-activation workspace (cfg.x2_max_batch >= 0)");
  if (B <= 0 || B > (x2 ? h->x2_batch : h->cfg.max_batch))
    return fail(h, MCM_ERANGE, x2 ? "batch exceeds mcm_x2_max_batch" : "batch exceeds cfg.max_batch");
  return MCM_OK;
}

// x2: the split-activation arm (include/mcm.h mcm_score_x2) — same weights, same workspace, B <= h->x2_batch
int encode_image_impl(mcm_handle* h, const void* pixels_dev, bool u8, int32_t B, float* out_dev,
                      void* stream, bool normalize = true, bool x2 = false) {
  int rc = check_image_call(h, pixels_dev, out_dev, B, x2);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const mcm_config& c = h->cfg;
  const int D = c.v_width;
  if ((rc = vision_front(h, s, pixels_dev, u8, B, x2))) return rc;
  if ((rc = run_layers(h, s, h->vis, B, h->ntok, false, true, true, x2))) return rc;
  {
    Scope sc(h, s, MCM_KC_POOL_PROJECT, 2.0 * B * D * c.proj_dim);
    HIP_TRY(h, launch_pool_project(h->x, nullptr, h->ntok, B, D,
                                   W(h, "vision_model.post_layernorm.weight"),
                                   W(h, "vision_model.post_layernorm.bias"), c.ln_eps,
                                   W(h, "visual_projection.weight"), c.proj_dim, out_dev, s, normalize));
  }
  return MCM_OK;
}
}  // namespace

extern "C" {

int mcm_encode_image(mcm_handle* h, const float* pixels_dev, int32_t B, float* out_dev, void* stream) {
  return encode_image_impl(h, pixels_dev, false, B, out_dev, stream);
}

int mcm_encode_image_raw(mcm_handle* h, const float* pixels_dev, int32_t B, float* out_dev, void* stream) {
  return encode_image_impl(h, pixels_dev, false, B, out_dev, stream, false);
}

int mcm_encode_image_ex(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B,
                        int32_t normalize, float* out_dev, void* stream) {
  if (int rc = check_pixel_format(h, pixel_format)) return rc;
  return encode_image_impl(h, pixels_dev, pixel_format == MCM_PIXELS_U8_NHWC, B, out_dev, stream,
                           normalize != 0);
}

int mcm_x2_max_batch(const mcm_handle* h) { return h ? h->x2_batch : 0; }

int mcm_kernel_faults(const mcm_handle* h) { return h && h->fault_pin ? (int)*(volatile unsigned int*)h->fault_pin : 0; }

int mcm_encode_image_x2(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, int32_t normalize,
                        float* out_dev, void* stream) {
  if (int rc = check_pixel_format(h, pixel_format)) return rc;
  return encode_image_impl(h, pixels_dev, pixel_format == MCM_PIXELS_U8_NHWC, B, out_dev, stream, normalize != 0, true);
}

int mcm_score_x2(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, const float* text_feat_dev,
                 int32_t K, float T, int32_t kind, float* scores_dev, void* stream) {
  int rc = mcm_encode_image_x2(h, pixels_dev, pixel_format, B, 1, h ? h->feat : nullptr, stream);
  if (rc) return rc;
  return mcm_score_features(h, h->feat, B, text_feat_dev, K, T, kind, scores_dev, stream);
}

int mcm_maha_prepare(mcm_handle* h, const float* means_dev, const float* prec_dev, int32_t C,
                     double* w_dev, double* k_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!means_dev || !prec_dev || !w_dev || !k_dev || C <= 0) return fail(h, MCM_EINVAL, "bad argument");
  HIP_TRY(h, launch_maha_prepare(means_dev, prec_dev, C, h->cfg.proj_dim, w_dev, k_dev, (hipStream_t)stream));
  return MCM_OK;
}

int mcm_maha_score_features(mcm_handle* h, const float* feats_dev, int32_t B, const float* prec_dev,
                            const double* w_dev, const double* k_dev, int32_t C, float* scores_dev,
                            void* stream) {
  if (!h) return MCM_EINVAL;
  if (!feats_dev || !prec_dev || !w_dev || !k_dev || !scores_dev || B <= 0 || C <= 0)
    return fail(h, MCM_EINVAL, "bad argument");
  HIP_TRY(h, launch_maha_score(feats_dev, B, prec_dev, w_dev, k_dev, C, h->cfg.proj_dim, scores_dev,
                               (hipStream_t)stream));
  return MCM_OK;
}

int mcm_maha_fit_accumulate(mcm_handle* h, const float* feats_dev, int32_t B, const float* shift_dev,
                            double* gram_dev, double* sum_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!feats_dev || !gram_dev || !sum_dev || B < 1) return fail(h, MCM_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const double P = h->cfg.proj_dim;
  Scope sc(h, s, MCM_KC_SCORE, (double)B * P * (P + 1.0));  // the upper triangle: B P (P + 1) / 2 fma
  HIP_TRY(h, launch_maha_fit(feats_dev, B, h->cfg.proj_dim, shift_dev, gram_dev, sum_dev, s));
  return MCM_OK;
}

namespace {
// The gate of the four entries of the bank-streamed scores (k-NN, NegLabel), for what they share: the handle, B, the width,
// `splits`, and *S_out = the split count a call over N bank rows runs with.  `own_ok`: the score's own rules.
bool bank_args_ok(const mcm_handle* h, bool own_ok, int32_t B, int64_t N, int32_t splits, int* S_out) {
  if (!h || !own_ok || B < 1 || splits < 0 || splits > MCM_KNN_MAX_SPLITS) return false;
  if (h->cfg.proj_dim < 4 || h->cfg.proj_dim % 4) return false;
  *S_out = splits ? splits : bank_auto_splits(B, N);
  return true;
}

// ... and of the two that launch: what the walk's 16-byte loads and the workspace need (0 = passed)
int bank_buffers(mcm_handle* h, const float* feats_dev, const float* bank_dev, int64_t work_bytes, int64_t need,
                 const char* floor_msg) {
  if (((uintptr_t)feats_dev | (uintptr_t)bank_dev) & 15) return fail(h, MCM_EINVAL, "feats_dev / bank_dev must be 16-byte aligned");
  return work_bytes < need ? fail(h, MCM_EINVAL, floor_msg) : MCM_OK;
}

bool knn_ok(int64_t N, int32_t k) { return N >= 1 && k >= 1 && k <= MCM_KNN_MAX_K; }
int64_t knn_work_bytes(int B, int k, int S) { return (int64_t)S * B * k * (int64_t)sizeof(float); }

bool neglabel_ok(int32_t K, int32_t G, int32_t gs) {
  return K >= 1 && G >= 1 && G <= MCM_NEG_MAX_GROUPS && gs >= 1 && (int64_t)K + (int64_t)G * gs <= INT32_MAX;
}
}  // namespace

int mcm_knn_workspace_bytes(const mcm_handle* h, int32_t B, int64_t N, int32_t k, int32_t splits, int64_t* bytes_out) {
  int S = 0;
  if (!bytes_out || !bank_args_ok(h, knn_ok(N, k), B, N, splits, &S)) return MCM_EINVAL;
  *bytes_out = knn_work_bytes(B, k, S);
  return MCM_OK;
}

int mcm_knn_score_features(mcm_handle* h, const float* feats_dev, int32_t B, const float* bank_dev, int64_t N, int32_t k,
                           int32_t splits, void* work_dev, int64_t work_bytes, float* scores_dev, float* topv_dev,
                           void* stream) {
  if (!h) return MCM_EINVAL;
  int S = 0;
  if (!feats_dev || !bank_dev || !work_dev || !scores_dev || !bank_args_ok(h, knn_ok(N, k), B, N, splits, &S))
    return fail(h, MCM_EINVAL, "bad argument");
  if (int rc = bank_buffers(h, feats_dev, bank_dev, work_bytes, knn_work_bytes(B, k, S),
                            "work_bytes is below mcm_knn_workspace_bytes"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * (double)N * h->cfg.proj_dim);
  HIP_TRY(h, launch_knn(feats_dev, B, bank_dev, N, h->cfg.proj_dim, k, S, (float*)work_dev, scores_dev, topv_dev, s));
  return MCM_OK;
}

int mcm_neglabel_workspace_bytes(const mcm_handle* h, int32_t B, int32_t K, int32_t G, int32_t gs, int32_t splits,
                                 int64_t* bytes_out) {
  int S = 0;
  if (!bytes_out || !bank_args_ok(h, neglabel_ok(K, G, gs), B, (int64_t)K + (int64_t)G * gs, splits, &S)) return MCM_EINVAL;
  *bytes_out = neglabel_work_bytes(B, G, S);
  return MCM_OK;
}

int mcm_neglabel_score_features(mcm_handle* h, const float* feats_dev, int32_t B, const float* bank_dev, int32_t K,
                                int32_t G, int32_t gs, float T, int32_t splits, void* work_dev, int64_t work_bytes,
                                float* scores_dev, float* group_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  int S = 0;
  if (!feats_dev || !bank_dev || !work_dev || !scores_dev ||
      !bank_args_ok(h, neglabel_ok(K, G, gs), B, (int64_t)K + (int64_t)G * gs, splits, &S))
    return fail(h, MCM_EINVAL, "bad argument");
  if (bad_temperature(T)) return fail(h, MCM_EINVAL, "T must be positive and finite");
  if (int rc = bank_buffers(h, feats_dev, bank_dev, work_bytes, neglabel_work_bytes(B, G, S),
                            "work_bytes is below mcm_neglabel_workspace_bytes"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * ((double)K + (double)G * gs) * h->cfg.proj_dim);
  HIP_TRY(h, launch_neglabel(feats_dev, B, bank_dev, K, G, gs, h->cfg.proj_dim, T, S, work_dev, scores_dev, group_dev, s));
  return MCM_OK;
}

// ---- ViM: null-space residual plus energy in one bank walk ----
namespace {
bool vim_ok(int32_t K, int32_t R) { return K >= 1 && R >= 1 && (int64_t)K + (int64_t)R <= INT32_MAX; }
}  // namespace

int mcm_vim_workspace_bytes(const mcm_handle* h, int32_t B, int32_t K, int32_t R, int32_t splits, int64_t* bytes_out) {
  int S = 0;
  if (!bytes_out || !bank_args_ok(h, vim_ok(K, R), B, (int64_t)K + (int64_t)R, splits, &S)) return MCM_EINVAL;
  *bytes_out = vim_work_bytes(B, S);
  return MCM_OK;
}

int mcm_vim_score_features(mcm_handle* h, const float* feats_dev, int32_t B, const float* bank_dev, int32_t K, int32_t R,
                           const double* off_dev, float T, float alpha, int32_t splits, void* work_dev, int64_t work_bytes,
                           float* scores_dev, float* parts_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  int S = 0;
  if (!feats_dev || !bank_dev || !work_dev || !scores_dev ||
      !bank_args_ok(h, vim_ok(K, R), B, (int64_t)K + (int64_t)R, splits, &S))
    return fail(h, MCM_EINVAL, "bad argument");
  if (bad_temperature(T)) return fail(h, MCM_EINVAL, "T must be positive and finite");
  if (!std::isfinite(alpha)) return fail(h, MCM_EINVAL, "alpha must be finite");
  if (((uintptr_t)off_dev | (uintptr_t)work_dev) & 7) return fail(h, MCM_EINVAL, "off_dev / work_dev must be 8-byte aligned");
  if (int rc = bank_buffers(h, feats_dev, bank_dev, work_bytes, vim_work_bytes(B, S),
                            "work_bytes is below mcm_vim_workspace_bytes"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * ((double)K + (double)R) * h->cfg.proj_dim);
  HIP_TRY(h, launch_vim(feats_dev, B, bank_dev, K, R, h->cfg.proj_dim, off_dev, T, alpha, S, work_dev, scores_dev, parts_dev, s));
  return MCM_OK;
}

// ---- the streamed tail of the MCM family (include/mcm_score_stream.h) ----
namespace {
bool score_stream_ok(int64_t K, int32_t kind, int32_t topk) {
  return K >= 1 && K <= INT32_MAX && kind >= 0 && kind <= MCM_SCORE_VAR && topk >= 0 && topk <= MCM_TOPK_MAX;
}
}  // namespace

int mcm_score_stream_workspace_bytes(const mcm_handle* h, int32_t B, int64_t K, int32_t topk, int32_t splits,
                                     int64_t* bytes_out) {
  int S = 0;
  if (!bytes_out || !bank_args_ok(h, score_stream_ok(K, MCM_SCORE_MCM, topk), B, K, splits, &S)) return MCM_EINVAL;
  *bytes_out = score_stream_work_bytes(B, topk, S);
  return MCM_OK;
}

int mcm_score_features_stream(mcm_handle* h, const float* img_feat_dev, int32_t B, const float* text_feat_dev, int64_t K,
                              float T, int32_t kind, int32_t topk, int32_t splits, void* work_dev, int64_t work_bytes,
                              float* scores_dev, float* parts_dev, int32_t* idx_dev, float* prob_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  int S = 0;
  if (!img_feat_dev || !text_feat_dev || !work_dev || !scores_dev ||
      !bank_args_ok(h, score_stream_ok(K, kind, topk), B, K, splits, &S))
    return fail(h, MCM_EINVAL, "bad argument");
  if (topk > 0 && !idx_dev) return fail(h, MCM_EINVAL, "idx_dev is NULL with topk > 0");
  if (bad_temperature(T)) return fail(h, MCM_EINVAL, "T must be positive and finite");
  if ((uintptr_t)work_dev & 7) return fail(h, MCM_EINVAL, "work_dev must be 8-byte aligned");
  if (int rc = bank_buffers(h, img_feat_dev, text_feat_dev, work_bytes, score_stream_work_bytes(B, topk, S),
                            "work_bytes is below mcm_score_stream_workspace_bytes"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * (double)K * h->cfg.proj_dim);
  HIP_TRY(h, launch_score_stream(img_feat_dev, B, text_feat_dev, (int)K, h->cfg.proj_dim, T, kind, topk, S, work_dev,
                                 scores_dev, parts_dev, idx_dev, prob_dev, s));
  return MCM_OK;
}

// ---- GL-MCM: the local score on features, and the local features from the tower ----
namespace {
bool local_args_ok(const mcm_handle* h, int32_t B, int32_t R, int32_t K) {
  return h && B >= 1 && R >= 1 && K >= 1 && (int64_t)B * R <= INT32_MAX && h->cfg.proj_dim >= 4 && h->cfg.proj_dim % 4 == 0;
}

// What a local call needs of the handle beyond an image call's own checks (0 = passed).  The local pass keeps its
// intermediates in buffers that are dead behind launch_pool_project: out_proj's rows in h->x, their post_layernorm in
// h->ln, the projected rows [padded rows, P] fp32 in h->hbuf; mcm_score_glmcm also the compacted rows in h->x again.
int check_local_call(mcm_handle* h, int32_t B) {
  const mcm_config& c = h->cfg;
  if (h->ntok < 2 || c.v_layers < 1) return fail(h, MCM_EINVAL, "the local pass needs patch tokens and an encoder layer");
  if (c.proj_dim % 16) return fail(h, MCM_EINVAL, "the local pass projects by a GEMM: proj_dim % 16 == 0");
  if (c.proj_dim > c.v_width) return fail(h, MCM_EINVAL, "the local pass keeps [B, R, proj_dim] in the residual buffer: proj_dim <= v_width");
  if ((size_t)padded_rows(h, B * h->ntok) * c.proj_dim * sizeof(float) > h->hbuf_bytes)
    return fail(h, MCM_EINVAL, "the MLP buffer does not hold the projected token rows");
  return MCM_OK;
}

// The local pass, behind an unchanged forward of the same B images on the same stream.  The last layer's V of all
// B ntok rows is still in h->qkv, columns [2D, 3D) (run_layers, the `cls` branch; nothing writes h->qkv afterwards):
//   o = W_o v + b_o          the layer's out_proj over every row, fp32 into h->x (zeroed first: the residual epilogue adds)
//   u = post_layernorm(o)    operand dtype, h->ln
//   y = W_proj u             a GEMM over all rows against h->wproj, fp32 into h->hbuf (zeroed first, as above)
//   local = y / |y|          rows 1 .. ntok - 1 of every image, compacted to [B, R, P]
// No attention mixing, no residual, no MLP: MaskCLIP's value path as the GL-MCM paper describes it.
int local_pass(mcm_handle* h, hipStream_t s, int32_t B, float* local_dev) {
  const mcm_config& c = h->cfg;
  const Tower& t = h->vis;
  const int D = c.v_width, P = c.proj_dim, M = B * h->ntok, prec = t.prec, es = prec_esize(prec);
  const LayerW& w = t.L[t.layers - 1];
  HIP_TRY(h, launch_zero_spans(ZeroSpans{{h->x}, {(size_t)M * D * sizeof(float) / 8}}, 1, s));  // (D is even: whole words)
  GemmArgs o{};
  o.x = (const char*)h->qkv + (size_t)2 * D * es; o.w = w.wo; o.bias = w.bo; o.resid = h->x;
  o.M = M; o.N = D; o.K = D; o.ldx = 3 * D; o.ldo = D; o.ksplit = t.split ? 1 : 0;
  HIP_TRY(h, gemm(h, s, prec, EPI_RESID, o));
  HIP_TRY(h, lnorm(h, s, prec, h->x, W(h, "vision_model.post_layernorm.weight"), W(h, "vision_model.post_layernorm.bias"),
                   h->ln, M, D, false));
  // (gemm() runs this one on whole 256-row tiles where the workspace has them: the pad rows of h->ln are zero —
  // vision_front zeroed them for this batch and nothing behind it writes past row M of h->ln —, their products land
  // behind row M of h->hbuf and are never read)
  HIP_TRY(h, launch_zero_spans(ZeroSpans{{h->hbuf}, {(size_t)padded_rows(h, M) * P * sizeof(float) / 8}}, 1, s));  // (256 | rows)
  GemmArgs p{};
  p.x = h->ln; p.w = h->wproj; p.bias = nullptr; p.resid = (float*)h->hbuf;
  p.M = M; p.N = P; p.K = D; p.ldx = D; p.ldo = P; p.ksplit = t.split ? 1 : 0;
  HIP_TRY(h, gemm(h, s, prec, EPI_RESID, p));
  {
    Scope sc(h, s, MCM_KC_POOL_PROJECT, 3.0 * B * (double)(h->ntok - 1) * P);
    HIP_TRY(h, launch_local_compact((const float*)h->hbuf, local_dev, B, h->ntok, P, s));
  }
  return MCM_OK;
}

int encode_image_local_impl(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, float* global_dev,
                            float* local_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (int rc = check_pixel_format(h, pixel_format)) return rc;
  int rc = check_image_call(h, pixels_dev, global_dev, B, false);
  if (rc) return rc;
  if (!local_dev) return fail(h, MCM_EINVAL, "null pointer");
  if ((uintptr_t)local_dev & 15) return fail(h, MCM_EINVAL, "local_dev must be 16-byte aligned");
  if ((rc = check_local_call(h, B))) return rc;
  if ((rc = encode_image_impl(h, pixels_dev, pixel_format == MCM_PIXELS_U8_NHWC, B, global_dev, stream))) return rc;
  return local_pass(h, (hipStream_t)stream, B, local_dev);
}
}  // namespace

int mcm_local_workspace_bytes(const mcm_handle* h, int32_t B, int32_t R, int32_t K, int64_t* bytes_out) {
  if (!bytes_out || !local_args_ok(h, B, R, K)) return MCM_EINVAL;
  *bytes_out = local_work_bytes(B, R);
  return MCM_OK;
}

int mcm_local_score_features(mcm_handle* h, const float* local_dev, int32_t B, int32_t R, const float* text_dev, int32_t K,
                             float T, void* work_dev, int64_t work_bytes, float* local_scores_dev, float* patch_dev,
                             void* stream) {
  if (!h) return MCM_EINVAL;
  if (!local_dev || !text_dev || !work_dev || !local_scores_dev || !local_args_ok(h, B, R, K))
    return fail(h, MCM_EINVAL, "bad argument");
  if (bad_temperature(T)) return fail(h, MCM_EINVAL, "T must be positive and finite");
  if (((uintptr_t)local_dev | (uintptr_t)text_dev) & 15) return fail(h, MCM_EINVAL, "local_dev / text_dev must be 16-byte aligned");
  if (((uintptr_t)work_dev | (uintptr_t)local_scores_dev | (uintptr_t)patch_dev) & 3)
    return fail(h, MCM_EINVAL, "work_dev / local_scores_dev / patch_dev must be 4-byte aligned");
  if (work_bytes < local_work_bytes(B, R)) return fail(h, MCM_EINVAL, "work_bytes is below mcm_local_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * (double)R * (double)K * h->cfg.proj_dim);
  HIP_TRY(h, launch_local_score(local_dev, B, R, text_dev, K, h->cfg.proj_dim, T, work_dev, local_scores_dev, patch_dev, s));
  return MCM_OK;
}

int mcm_encode_image_local(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, float* global_dev,
                           float* local_dev, void* stream) {
  return encode_image_local_impl(h, pixels_dev, pixel_format, B, global_dev, local_dev, stream);
}

int mcm_score_glmcm(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, const float* text_dev, int32_t K,
                    float T, float lambda, float* scores_dev, float* global_scores_dev, float* local_scores_dev,
                    float* patch_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!text_dev || !scores_dev) return fail(h, MCM_EINVAL, "null pointer");
  if (K < 1 || bad_temperature(T) || !std::isfinite(lambda)) return fail(h, MCM_EINVAL, "bad K / T / lambda");
  if ((uintptr_t)text_dev & 15) return fail(h, MCM_EINVAL, "text_dev must be 16-byte aligned");
  // the compacted local rows go where out_proj's rows were (h->x is dead again behind post_layernorm: B R P <= B ntok D
  // floats, check_local_call); the row values and the parts nobody asked for go to h->att, which is dead as well
  const int R = h->ntok - 1;
  float* local = h->x;
  int rc = encode_image_local_impl(h, pixels_dev, pixel_format, B, h->feat, local, stream);
  if (rc) return rc;
  float* work = (float*)h->att;  // [B R] row values, then [B] and [B]: B (R + 2) floats <= the B ntok D operand elements it holds
  float* gs = global_scores_dev ? global_scores_dev : work + (size_t)B * R;
  float* ls = local_scores_dev ? local_scores_dev : work + (size_t)B * R + B;
  if ((rc = mcm_score_features(h, h->feat, B, text_dev, K, T, MCM_SCORE_MCM, gs, stream))) return rc;
  if ((rc = mcm_local_score_features(h, local, B, R, text_dev, K, T, work, local_work_bytes(B, R), ls, patch_dev, stream))) return rc;
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B);
  HIP_TRY(h, launch_local_combine(gs, ls, lambda, scores_dev, B, s));
  return MCM_OK;
}

int mcm_encode_image_u8(mcm_handle* h, const uint8_t* pixels_dev, int32_t B, float* out_dev,
                        void* stream) {
  return encode_image_impl(h, pixels_dev, true, B, out_dev, stream);
}

int mcm_score_u8(mcm_handle* h, const uint8_t* pixels_dev, int32_t B, const float* text_feat_dev,
                 int32_t K, float T, int32_t kind, float* scores_dev, void* stream) {
  int rc = encode_image_impl(h, pixels_dev, true, B, h ? h->feat : nullptr, stream);
  if (rc) return rc;
  return mcm_score_features(h, h->feat, B, text_feat_dev, K, T, kind, scores_dev, stream);
}

namespace {
// torchvision's Resize(int) and CenterCrop arithmetic (see preprocess.hip): resized size and crop
// origin of an H x W image for a square target S
bool prep_geometry(int32_t H, int32_t W, int32_t S, PrepImage& g) {
  const int32_t shrt = W <= H ? W : H, lng = W <= H ? H : W;
  g.H = H;
  g.W = W;
  if (shrt == S) {
    g.nh = H;
    g.nw = W;
  } else {
    const int32_t nl = (int32_t)((double)S * (double)lng / (double)shrt);  // int(size * long / short)
    g.nw = W <= H ? S : nl;
    g.nh = W <= H ? nl : S;
  }
  if (g.nh < S || g.nw < S) return false;
  auto round_half_even = [](double v) {  // Python 3 round() on the x.0 / x.5 values that occur here
    const double f = floor(v), d = v - f;
    if (d < 0.5) return (int32_t)f;
    if (d > 0.5) return (int32_t)f + 1;
    return ((int64_t)f % 2 == 0) ? (int32_t)f : (int32_t)f + 1;
  };
  g.top = round_half_even((g.nh - S) / 2.0);
  g.left = round_half_even((g.nw - S) / 2.0);
  return true;
}
}  // namespace

int mcm_resize_crop_u8(mcm_handle* h, const uint8_t* const* src_dev_ptrs, const int32_t* heights,
                       const int32_t* widths, int32_t B, uint8_t* dst_dev, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!src_dev_ptrs || !heights || !widths || !dst_dev) return fail(h, MCM_EINVAL, "null pointer");
  if (B <= 0) return fail(h, MCM_EINVAL, "B must be positive");
  if (B > h->cfg.max_batch) return fail(h, MCM_ERANGE, "batch exceeds max_batch");
  const int32_t S = h->cfg.image_size;
  hipStream_t s = (hipStream_t)stream;
  const unsigned slot = h->prep_next++ % mcm_handle::PREP_RING;
  PrepImage* pin = h->prep_pin + (size_t)slot * h->cfg.max_batch;
  PrepImage* dev = h->prep_dev + (size_t)slot * h->cfg.max_batch;
  HIP_TRY(h, hipEventSynchronize(h->prep_ev[slot]));  // the copy out of this slot, PREP_RING calls ago (long done: no stall)
  for (int32_t b = 0; b < B; ++b) {
    PrepImage& g = pin[b];
    if (!src_dev_ptrs[b] || heights[b] <= 0 || widths[b] <= 0) return fail(h, MCM_EINVAL, "bad image");
    g.src = src_dev_ptrs[b];
    if (!prep_geometry(heights[b], widths[b], S, g)) return fail(h, MCM_EINVAL, "image smaller than the crop");
    const int taps_x = g.nw != g.W ? 2 * (int)ceil(fmax((double)g.W / g.nw, 1.0)) + 1 : 1;
    const int taps_y = g.nh != g.H ? 2 * (int)ceil(fmax((double)g.H / g.nh, 1.0)) + 1 : 1;
    if (taps_x > prep_max_taps() || taps_y > prep_max_taps())
      return fail(h, MCM_ERANGE, "downscale factor above 31 is not supported");
  }
  HIP_TRY(h, hipMemcpyAsync(dev, pin, (size_t)B * sizeof(PrepImage), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipEventRecord(h->prep_ev[slot], s));
  if (!h->prep_coef) {  // first call on this handle (one synchronous allocation; text-only / pre-cropped users never pay it)
    rc = dev_alloc(h, (void**)&h->prep_coef, (size_t)mcm_handle::PREP_RING * prep_coef_bytes(h->cfg.max_batch, S));
    if (rc) return rc;
  }
  int32_t* coef = (int32_t*)((char*)h->prep_coef + (size_t)slot * prep_coef_bytes(h->cfg.max_batch, S));
  HIP_TRY(h, launch_resize_crop(dev, coef, B, S, dst_dev, s, g_resize_fused_only != 0));
  return MCM_OK;
}

int mcm_jpeg_reconstruct(mcm_handle* h, const void* coef_dev, const mcm_jpeg_image* meta, const uint16_t* quant, int32_t n,
                         uint8_t* rgb_dev, const int64_t* rgb_offsets, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!coef_dev || !meta || !quant || !rgb_dev || !rgb_offsets) return fail(h, MCM_EINVAL, "null pointer");
  if (n <= 0) return fail(h, MCM_EINVAL, "n must be positive");
  if (n > h->cfg.max_batch) return fail(h, MCM_ERANGE, "batch exceeds max_batch");
  hipStream_t s = (hipStream_t)stream;
  // a slot of the staging ring: max_batch records, then (16-byte aligned: the kernel reads them as 16-byte rows) the tables
  const size_t qoff = ((size_t)h->cfg.max_batch * sizeof(JpegImageDev) + 15) / 16 * 16;
  const size_t slot_bytes = (qoff + (size_t)h->cfg.max_batch * 3 * 64 * sizeof(uint16_t) + 255) / 256 * 256;
  if ((uintptr_t)coef_dev & 15) return fail(h, MCM_EINVAL, "coef_dev must be 16-byte aligned");
  if (!h->jpg_ready) {  // first call on this handle; `jpg_ready` only once EVERY piece exists (a failed half is retried)
    if (!h->jpg_pin && hipHostMalloc((void**)&h->jpg_pin, mcm_handle::PREP_RING * slot_bytes) != hipSuccess) {
      h->jpg_pin = nullptr;
      return fail(h, MCM_ENOMEM, "hipHostMalloc jpeg");
    }
    if (!h->jpg_dev && (rc = dev_alloc(h, (void**)&h->jpg_dev, mcm_handle::PREP_RING * slot_bytes))) return rc;
    for (int k = 0; k < mcm_handle::PREP_RING; ++k)
      if (!h->jpg_ev[k] && hipEventCreateWithFlags(&h->jpg_ev[k], hipEventDisableTiming) != hipSuccess) {
        h->jpg_ev[k] = nullptr;
        return fail(h, MCM_EHIP, "hipEventCreate jpeg");
      }
    h->jpg_ready = true;
  }
  const unsigned slot = h->jpg_next++ % mcm_handle::PREP_RING;
  char* pin = h->jpg_pin + slot * slot_bytes;
  char* dev = h->jpg_dev + slot * slot_bytes;
  HIP_TRY(h, hipEventSynchronize(h->jpg_ev[slot]));
  JpegImageDev* md = (JpegImageDev*)pin;
  uint16_t* qd = (uint16_t*)(pin + qoff);
  size_t planes = 0;
  int m = 0, max_blocks = 0, max_pixels = 0;
  for (int32_t i = 0; i < n; ++i) {
    const mcm_jpeg_image& im = meta[i];
    if (im.status != 0) continue;  // not taken by the entropy decoder: the caller fills this image's pixels itself
    if (im.width <= 0 || im.height <= 0 || (im.ncomp != 1 && im.ncomp != 3) || rgb_offsets[i] < 0) return fail(h, MCM_EINVAL, "bad jpeg record");
    JpegImageDev& d = md[m];
    d.width = im.width; d.height = im.height; d.ncomp = im.ncomp;
    d.H = im.ncomp == 3 ? im.hs[0] : 1;
    d.V = im.ncomp == 3 ? im.vs[0] : 1;
    if (im.ncomp == 3 && !((d.H == 1 && d.V == 1) || (d.H == 2 && d.V == 1) || (d.H == 2 && d.V == 2))) return fail(h, MCM_EINVAL, "sampling not taken");
    int blocks = 0;
    for (int c = 0; c < 3; ++c) {
      d.wb[c] = c < im.ncomp ? im.wb[c] : 0;
      d.hb[c] = c < im.ncomp ? im.hb[c] : 0;
      d.coef_off[c] = c < im.ncomp ? im.coef_off[c] : 0;
      d.plane_off[c] = (int64_t)planes;
      if (c < im.ncomp) {
        if (im.wb[c] <= 0 || im.hb[c] <= 0 || im.coef_off[c] < 0 || (im.coef_off[c] & 15)) return fail(h, MCM_EINVAL, "bad jpeg plane");
        planes += (size_t)im.wb[c] * im.hb[c] * 64;
        blocks += im.wb[c] * im.hb[c];
      }
    }
    d.rgb_off = rgb_offsets[i];
    memcpy(qd + (size_t)m * 192, quant + (size_t)i * 192, 192 * sizeof(uint16_t));
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
    max_pixels = im.width * im.height > max_pixels ? im.width * im.height : max_pixels;
    ++m;
  }
  if (m == 0) return MCM_OK;
  if (planes > h->jpg_planes_bytes) {  // grow (synchronous, rare: the first batches of a run)
    HIP_TRY(h, hipStreamSynchronize(s));
    if (h->jpg_planes) (void)hipFree(h->jpg_planes);
    h->jpg_planes = nullptr;
    h->jpg_planes_bytes = 0;
    const size_t want = planes + planes / 4 + (1 << 20);
    if (hipMalloc((void**)&h->jpg_planes, want) != hipSuccess) return fail(h, MCM_ENOMEM, "hipMalloc jpeg planes");
    h->jpg_planes_bytes = want;
  }
  HIP_TRY(h, hipMemcpyAsync(dev, pin, (size_t)m * sizeof(JpegImageDev), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(dev + qoff, pin + qoff, (size_t)m * 192 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipEventRecord(h->jpg_ev[slot], s));
  HIP_TRY(h, launch_jpeg_reconstruct((const JpegImageDev*)dev, (const uint16_t*)(dev + qoff), coef_dev, h->jpg_planes, rgb_dev, m,
                                     max_blocks, max_pixels, s));
  return MCM_OK;
}

int mcm_reduce_bank(mcm_handle* h, const float* feats_dev, int32_t K, int32_t T, float* bank_dev,
                    void* stream) {
  if (!h) return MCM_EINVAL;
  if (!feats_dev || !bank_dev || K <= 0 || T <= 0) return fail(h, MCM_EINVAL, "bad argument");
  HIP_TRY(h, launch_bank_reduce(feats_dev, K, T, h->cfg.proj_dim, bank_dev, (hipStream_t)stream));
  return MCM_OK;
}

int mcm_measures(mcm_handle* h, const float* pos_dev, int64_t n_pos, const float* neg_dev,
                 int64_t n_neg, int32_t negate, double recall_level, double* out_host, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!pos_dev || !neg_dev || !out_host) return fail(h, MCM_EINVAL, "null pointer");
  if (n_pos <= 0 || n_neg <= 0 || n_pos + n_neg > 0x7fffffffLL)
    return fail(h, MCM_EINVAL, "both score vectors must be non-empty");
  if (!(recall_level >= 0.0 && recall_level <= 1.0)) return fail(h, MCM_EINVAL, "recall_level outside [0,1]");
  hipStream_t s = (hipStream_t)stream;
  // the three per-example count arrays (12 B per score) live in the MLP activation buffer, which is
  // idle between encode calls and ordered against them by the stream (the caller passes the stream its
  // encode / score calls ran on — include/mcm.h); score vectors that do not fit it get a one-off
  // stream-ordered allocation instead of a refusal
  const size_t need = measures_workspace_bytes((long)(n_pos + n_neg));
  void* ws = h->hbuf;
  bool own = false;
  if (need > h->hbuf_bytes) {
    HIP_TRY(h, hipMallocAsync(&ws, need, s));
    own = true;
  }
  double* out_dev = nullptr;
  hipError_t e = launch_measures(pos_dev, (long)n_pos, neg_dev, (long)n_neg, negate, recall_level, ws, &out_dev, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out_host, out_dev, 3 * sizeof(double), hipMemcpyDeviceToHost, s);
  if (own) (void)hipFreeAsync(ws, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(h, MCM_EHIP, std::string("mcm_measures: ") + hipGetErrorString(e));
  return MCM_OK;
}

int mcm_score_histogram(mcm_handle* h, const float* scores_dev, int64_t n, const float* edges_dev,
                        int32_t n_bins, int64_t* counts_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if ((!scores_dev && n) || !edges_dev || !counts_dev || n < 0 || n_bins <= 0)  // n == 0: all-zero counts, no vector needed
    return fail(h, MCM_EINVAL, "bad argument");
  if (n_bins > 8192) return fail(h, MCM_ERANGE, "at most 8192 bins");
  HIP_TRY(h, launch_histogram(scores_dev, (long)n, edges_dev, n_bins, (unsigned long long*)counts_dev,
                              (hipStream_t)stream));
  return MCM_OK;
}

int mcm_encode_text(mcm_handle* h, const int32_t* ids_host, int32_t K, int32_t S, float* out_dev,
                    void* stream) {
  return mcm_encode_text_ex(h, ids_host, K, S, 1, out_dev, stream);
}

namespace {
// The text tower over validated prompts, in passes of max_prompt_tokens / S prompts.  slot_host == NULL: mcm_encode_text_ex, the
// ids embedded by launch_text_embed as they always were.  Otherwise mcm_encode_text_ctx: the slot map travels in the id words
// the pass uploads anyway — a position with slot j >= 0 is staged as -(j + 1), which launch_text_embed_ctx reads as row j of the
// prompt's context set — so there is no buffer beyond mcm_encode_text_ex's.  Pooling reads ids_host either way, the placeholder
// ids under the slots included.
int encode_text_passes(mcm_handle* h, const int32_t* ids_host, const int32_t* slot_host, int32_t K, int32_t S,
                       const float* ctx_dev, int32_t n_ctx, int32_t n_sets, int32_t normalize, float* out_dev, hipStream_t s) {
  const mcm_config& c = h->cfg;
  int rc;
  const int D = c.t_width;
  const int chunk = c.max_prompt_tokens / S;  // prompts per pass
  for (int k0 = 0; k0 < K; k0 += chunk) {
    const int kc = (K - k0) < chunk ? (K - k0) : chunk;
    HIP_TRY(h, hipStreamSynchronize(s));  // pinned staging buffers are reused
    for (int k = 0; k < kc; ++k) {
      const int32_t* row = ids_host + (size_t)(k0 + k) * S;
      const int32_t* slot = slot_host ? slot_host + (size_t)(k0 + k) * S : nullptr;
      int best = 0;  // first EOS = argmax id (HF modeling_clip.py:561-581; CoOp: tokenized_prompts.argmax(-1))
      for (int j = 0; j < S; ++j) {
        h->ids_pin[(size_t)k * S + j] = (slot && slot[j] >= 0) ? -(slot[j] + 1) : row[j];
        if (row[j] > row[best]) best = j;
      }
      h->rowidx_pin[k] = k * S + best;
    }
    HIP_TRY(h, hipMemcpyAsync(h->ids_dev, h->ids_pin, (size_t)kc * S * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->rowidx_dev, h->rowidx_pin, (size_t)kc * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
    {
      Scope sc(h, s, MCM_KC_EMBED, 0.0);
      if (slot_host)
        HIP_TRY(h, launch_text_embed_ctx(h->ids_dev, W(h, "text_model.embeddings.token_embedding.weight"),
                                         W(h, "text_model.embeddings.position_embedding.weight"), ctx_dev, h->x,
                                         kc, S, D, n_ctx, n_sets, k0, s));
      else
        HIP_TRY(h, launch_text_embed(h->ids_dev, W(h, "text_model.embeddings.token_embedding.weight"),
                                     W(h, "text_model.embeddings.position_embedding.weight"), h->x,
                                     kc, S, D, s));
    }
    if ((rc = run_layers(h, s, h->txt, kc, S, true, false))) return rc;
    {
      Scope sc(h, s, MCM_KC_POOL_PROJECT, 2.0 * kc * D * c.proj_dim);
      HIP_TRY(h, launch_pool_project(h->x, h->rowidx_dev, 0, kc, D,
                                     W(h, "text_model.final_layer_norm.weight"),
                                     W(h, "text_model.final_layer_norm.bias"), c.ln_eps,
                                     W(h, "text_projection.weight"), c.proj_dim,
                                     out_dev + (size_t)k0 * c.proj_dim, s, normalize != 0));
    }
  }
  return MCM_OK;
}
}  // namespace

int mcm_encode_text_ex(mcm_handle* h, const int32_t* ids_host, int32_t K, int32_t S, int32_t normalize,
                       float* out_dev, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!ids_host || !out_dev) return fail(h, MCM_EINVAL, "null pointer");
  const mcm_config& c = h->cfg;
  if (K <= 0 || S <= 0) return fail(h, MCM_EINVAL, "K and S must be positive");
  if (S > c.max_positions)  // HF modeling_clip.py:241-245 raises ValueError
    return fail(h, MCM_ERANGE, "sequence length exceeds max_position_embeddings");
  for (int64_t i = 0; i < (int64_t)K * S; ++i)
    if (ids_host[i] < 0 || ids_host[i] >= c.vocab_size) return fail(h, MCM_EINVAL, "token id out of range");
  return encode_text_passes(h, ids_host, nullptr, K, S, nullptr, 0, 0, normalize, out_dev, (hipStream_t)stream);
}

int mcm_encode_text_ctx(mcm_handle* h, const int32_t* ids_host, const int32_t* slot_host, int32_t K, int32_t S,
                        const float* ctx_dev, int32_t n_ctx, int32_t n_sets, int32_t normalize, float* out_dev, void* stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!ids_host || !slot_host || !ctx_dev || !out_dev) return fail(h, MCM_EINVAL, "null pointer");
  const mcm_config& c = h->cfg;
  if (K <= 0 || S <= 0 || n_ctx <= 0) return fail(h, MCM_EINVAL, "K, S and n_ctx must be positive");
  if (n_sets != 1 && n_sets != K) return fail(h, MCM_EINVAL, "n_sets must be 1 (one context for every prompt) or K (one per prompt)");
  if ((uintptr_t)ctx_dev & 15) return fail(h, MCM_EINVAL, "ctx_dev must be 16-byte aligned");
  if (S > c.max_positions)  // as mcm_encode_text_ex
    return fail(h, MCM_ERANGE, "sequence length exceeds max_position_embeddings");
  for (int64_t i = 0; i < (int64_t)K * S; ++i) {
    if (ids_host[i] < 0 || ids_host[i] >= c.vocab_size) return fail(h, MCM_EINVAL, "token id out of range");
    if (slot_host[i] < -1 || slot_host[i] >= n_ctx) return fail(h, MCM_EINVAL, "context slot out of range (-1 .. n_ctx - 1)");
  }
  return encode_text_passes(h, ids_host, slot_host, K, S, ctx_dev, n_ctx, n_sets, normalize, out_dev, (hipStream_t)stream);
}

int mcm_score_features(mcm_handle* h, const float* img_feat_dev, int32_t B, const float* text_feat_dev,
                       int32_t K, float T, int32_t kind, float* scores_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!img_feat_dev || !text_feat_dev || !scores_dev) return fail(h, MCM_EINVAL, "null pointer");
  if (B <= 0 || K <= 0 || kind < 0 || kind > MCM_SCORE_VAR || !(T > 0.f))
    return fail(h, MCM_EINVAL, "bad B / K / kind / T");
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * (double)K * h->cfg.proj_dim);
  HIP_TRY(h, launch_score(img_feat_dev, B, text_feat_dev, K, h->cfg.proj_dim, T, kind, scores_dev, s));
  return MCM_OK;
}

int mcm_score(mcm_handle* h, const float* pixels_dev, int32_t B, const float* text_feat_dev, int32_t K,
              float T, int32_t kind, float* scores_dev, void* stream) {
  int rc = mcm_encode_image(h, pixels_dev, B, h ? h->feat : nullptr, stream);
  if (rc) return rc;
  return mcm_score_features(h, h->feat, B, text_feat_dev, K, T, kind, scores_dev, stream);
}

namespace {
// every refusal of the top-k tail, made before anything is launched (mcm_score_topk encodes first)
int check_topk_call(mcm_handle* h, const float* text_feat_dev, int32_t B, int32_t K, float T, int32_t kind,
                    int32_t topk, const float* scores_dev, const int32_t* idx_dev) {
  if (!text_feat_dev || !scores_dev || !idx_dev) return fail(h, MCM_EINVAL, "null pointer");
  if (B <= 0 || K <= 0 || kind < 0 || kind > MCM_SCORE_VAR || !(T > 0.f))
    return fail(h, MCM_EINVAL, "bad B / K / kind / T");
  if (topk < 1 || topk > MCM_TOPK_MAX) return fail(h, MCM_EINVAL, "topk must be 1..MCM_TOPK_MAX");
  if (!score_shape_ok(K, h->cfg.proj_dim))
    return fail(h, MCM_EINVAL, "proj_dim % 4 != 0, or the bank exceeds the scoring tail's LDS ((proj_dim + K) * 4 > 150 KiB)");
  return MCM_OK;
}
}  // namespace

int mcm_score_features_topk(mcm_handle* h, const float* img_feat_dev, int32_t B, const float* text_feat_dev,
                            int32_t K, float T, int32_t kind, int32_t topk, float* scores_dev, int32_t* idx_dev,
                            float* prob_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!img_feat_dev) return fail(h, MCM_EINVAL, "null pointer");
  int rc = check_topk_call(h, text_feat_dev, B, K, T, kind, topk, scores_dev, idx_dev);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  Scope sc(h, s, MCM_KC_SCORE, 2.0 * B * (double)K * h->cfg.proj_dim);
  HIP_TRY(h, launch_score_topk(img_feat_dev, B, text_feat_dev, K, h->cfg.proj_dim, T, kind, topk, scores_dev,
                               idx_dev, prob_dev, s));
  return MCM_OK;
}

int mcm_score_topk(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t x2, int32_t B,
                   const float* text_feat_dev, int32_t K, float T, int32_t kind, int32_t topk, float* scores_dev,
                   int32_t* idx_dev, float* prob_dev, void* stream) {
  if (!h) return MCM_EINVAL;
  if (int rc = check_pixel_format(h, pixel_format)) return rc;
  int rc = check_topk_call(h, text_feat_dev, B, K, T, kind, topk, scores_dev, idx_dev);
  if (rc) return rc;
  if ((rc = encode_image_impl(h, pixels_dev, pixel_format == MCM_PIXELS_U8_NHWC, B, h->feat, stream, true, x2 != 0)))
    return rc;
  return mcm_score_features_topk(h, h->feat, B, text_feat_dev, K, T, kind, topk, scores_dev, idx_dev, prob_dev, stream);
}

int mcm_saturation_check(mcm_handle* h, int32_t on) {
  if (!h) return MCM_EINVAL;
  h->sat_on = on != 0;
  return MCM_OK;
}

int mcm_saturation_count(mcm_handle* h, int32_t reset, uint64_t* count_host, void* stream) {
  if (!h || !count_host) return fail(h, MCM_EINVAL, "null argument");
  hipStream_t s = (hipStream_t)stream;
  unsigned int v = 0;
  HIP_TRY(h, hipMemcpyAsync(&v, h->sat_dev, sizeof(v), hipMemcpyDeviceToHost, s));
  if (reset) HIP_TRY(h, hipMemsetAsync(h->sat_dev, 0, sizeof(v), s));
  HIP_TRY(h, hipStreamSynchronize(s));
  *count_host = v;
  return MCM_OK;
}

int mcm_profile_enable(mcm_handle* h, int32_t on) {
  if (!h) return MCM_EINVAL;
  h->prof = on != 0;
  return MCM_OK;
}

int mcm_profile_read(mcm_handle* h, double* ms_out, int64_t* launches_out, double* flops_out) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, hipDeviceSynchronize());
  for (size_t i = 0; i < h->ev_used; ++i) {
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev_pool[i].a, h->ev_pool[i].b));
    h->ms_acc[h->ev_pool[i].kc] += ms;
    if (h->ev_pool[i].kc2 >= 0) h->ms_acc[h->ev_pool[i].kc2] += ms;
  }
  h->ev_used = 0;
  for (int k = 0; k < MCM_KC_COUNT; ++k) {
    if (ms_out) ms_out[k] = h->ms_acc[k];
    if (launches_out) launches_out[k] = h->launches[k];
    if (flops_out) flops_out[k] = h->flops[k];
    h->ms_acc[k] = 0;
    h->launches[k] = 0;
    h->flops[k] = 0;
  }
  return MCM_OK;
}

// ---- operator-level entry points ------------------------------------------------------

int mcm_op_linear(mcm_handle* h, int32_t prec, const void* x_dev, const void* w_dev, const float* bias_dev,
                  void* y_dev, float* resid_dev, int32_t M, int32_t N, int32_t K, int32_t epi,
                  void* stream) {
  return mcm_op_linear_ex(h, prec, x_dev, w_dev, bias_dev, y_dev, resid_dev, M, N, K, epi, 0, stream);
}

int mcm_op_linear_ex(mcm_handle* h, int32_t prec, const void* x_dev, const void* w_dev, const float* bias_dev,
                     void* y_dev, float* resid_dev, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t flags,
                     void* stream) {
  if (!h) return MCM_EINVAL;
  if (epi < EPI_STORE || epi > EPI_RESID) return fail(h, MCM_EINVAL, "bad epilogue");
  const bool split = (flags & MCM_LINEAR_SPLIT_W) != 0, xs = (flags & MCM_LINEAR_SPLIT_X) != 0, os = (flags & MCM_LINEAR_SPLIT_OUT) != 0;
  const bool erf = (flags & MCM_LINEAR_ACT_GELU) != 0;
  if ((flags & ~(MCM_LINEAR_SPLIT_W | MCM_LINEAR_SPLIT_X | MCM_LINEAR_SPLIT_OUT | MCM_LINEAR_ACT_GELU)) ||
      (split && (prec == MCM_PREC_F32 || K % 64)))
    return fail(h, MCM_EINVAL, "bad flags (split weights: 16-bit modes, K % 64 == 0)");
  if (erf && epi != EPI_GELU) return fail(h, MCM_EINVAL, "bad flags (MCM_LINEAR_ACT_GELU: epilogue 1 only)");
  if ((xs || os) && (prec != MCM_PREC_F16 || K % 64 || (os && (epi == EPI_RESID || N % 64))))
    return fail(h, MCM_EINVAL, "bad flags (split activations / outputs: fp16 mode, K % 64 == 0; outputs: epilogues 0 / 1, N % 64 == 0)");
  GemmArgs a{};
  a.x = x_dev; a.w = w_dev; a.bias = bias_dev; a.out = y_dev; a.resid = resid_dev;
  a.M = M; a.N = N; a.K = split ? 2 * K : K; a.ldx = xs ? 2 * K : K; a.ldo = os ? 2 * N : N; a.ksplit = split ? 1 : 0;
  a.xsplit = xs ? 1 : 0;
  if (os) epi = epi == EPI_STORE ? EPI_STORE_X2 : erf ? EPI_GELU_ERF_X2 : EPI_GELU_X2;
  else if (erf) epi = EPI_GELU_ERF;
  a.sat = h->sat_on ? h->sat_dev : nullptr;
  HIP_TRY(h, launch_gemm(prec, epi, a, (hipStream_t)stream));
  return MCM_OK;
}

int mcm_op_split_weight(mcm_handle* h, int32_t prec, const float* w_dev, int32_t N, int32_t K, void* out_dev,
                        void* stream) {
  if (!h) return MCM_EINVAL;
  if (!w_dev || !out_dev || N <= 0 || K <= 0 || K % 64 || prec == MCM_PREC_F32)
    return fail(h, MCM_EINVAL, "split weights: 16-bit modes, K % 64 == 0");
  HIP_TRY(h, launch_cvt_weight_split(prec, w_dev, out_dev, N, K, K, (hipStream_t)stream));
  return MCM_OK;
}

int mcm_op_layernorm(mcm_handle* h, int32_t prec, const float* x_dev, const float* gamma_dev,
                     const float* beta_dev, void* y_dev, int32_t M, int32_t D, float eps, int32_t out_f32,
                     void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_layernorm(prec, x_dev, gamma_dev, beta_dev, y_dev, M, D, eps, out_f32 != 0,
                              (hipStream_t)stream, 0, 0, false, h->sat_on ? h->sat_dev : nullptr));
  return MCM_OK;
}

int mcm_op_layernorm_split(mcm_handle* h, const float* x_dev, const float* gamma_dev, const float* beta_dev,
                           void* y_dev, int32_t M, int32_t D, float eps, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_layernorm(MCM_PREC_F16, x_dev, gamma_dev, beta_dev, y_dev, M, D, eps, false, (hipStream_t)stream, 0, 0,
                              false, h->sat_on ? h->sat_dev : nullptr, true));
  return MCM_OK;
}

int mcm_op_attention_split(mcm_handle* h, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                           int32_t heads, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_attention(MCM_PREC_F16, qkv_dev, out_dev, nseq, seq_len, heads, 64, false, 0, (hipStream_t)stream, false, 0, true));
  return MCM_OK;
}

int mcm_op_attention(mcm_handle* h, int32_t prec, const void* qkv_dev, void* out_dev, int32_t nseq,
                     int32_t seq_len, int32_t heads, int32_t causal, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_attention(prec, qkv_dev, out_dev, nseq, seq_len, heads, 64, causal != 0, 0,
                              (hipStream_t)stream, false, 0, false, h->fault_dev));
  return MCM_OK;
}

#ifdef MCM_HARNESS  // libmcm_hip_harness.so only: process-wide A/B switches for tests and tools
// The MLP activations as the GEMM epilogues compute them (common.hpp), element-wise on a device array: the test that sweeps
// every fp32 bit pattern through gelu_erf.  act: 0 quick_gelu, 1 quick_gelu_fast, 2 gelu_erf.
__global__ void act_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, int act) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = act == 2 ? gelu_erf(x[i]) : act == 1 ? quick_gelu_fast(x[i]) : quick_gelu(x[i]);
}
int mcm_debug_op_act(mcm_handle* h, int32_t act, const float* x_dev, float* y_dev, int64_t n, void* stream) {
  if (!h) return MCM_EINVAL;
  if (act < 0 || act > 2 || !x_dev || !y_dev || n <= 0) return fail(h, MCM_EINVAL, "act 0 ... 2, n > 0, device pointers");
  const size_t blocks = ((size_t)n + 255) / 256;
  hipLaunchKernelGGL(act_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev,
                     (size_t)n, (int)act);
  HIP_TRY(h, hipGetLastError());
  return MCM_OK;
}

int mcm_debug_attention_variant(int32_t variant) {
  if (variant != 0 && variant != 1 && variant != 10 && variant != 11 && variant != 21 && variant != 36) return MCM_EINVAL;
  attention_set_variant(variant);
  return MCM_OK;
}

// polls a wait of the persistent attention kernel may take before it gives up (attention.hip PS_SPIN_BUDGET = 1 << 22 is what
// the shipped library always passes); 0 = every wait that has to wait gives up at once: the test of the fault path
int mcm_debug_attn_spin_budget(int64_t polls) {
  if (polls < 0 || polls > 0xffffffffLL) return MCM_EINVAL;
  attention_set_spin_budget((unsigned int)polls);
  return MCM_OK;
}

// clears the handle's sticky kernel-fault word (tests of the fault path only: a real fault leaves results invalid)
int mcm_debug_clear_faults(mcm_handle* h) {
  if (!h || !h->fault_pin) return MCM_EINVAL;
  (void)hipDeviceSynchronize();
  *(volatile unsigned int*)h->fault_pin = 0u;
  return MCM_OK;
}

// mcm_op_attention with the two launch parameters only the model sets: the number of query rows (the CLS-only last layer) and
// the walk direction
int mcm_debug_op_attention(mcm_handle* h, int32_t prec, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                           int32_t heads, int32_t causal, int32_t qrows, int32_t reverse, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_attention(prec, qkv_dev, out_dev, nseq, seq_len, heads, 64, causal != 0, qrows, (hipStream_t)stream, reverse != 0, 0, false,
                              h->fault_dev));
  return MCM_OK;
}

// the same with the head width as an argument: 64 takes mcm_debug_op_attention's routes, 80 the streaming family of ViT-H/14's
// vision tower (attn_hd80_kernel: bidirectional only, seq_len <= 1025); qkv [nseq seq_len, 3 heads head_dim], head h at column
// h head_dim of q, k and v.  A refused argument launches nothing.
int mcm_debug_op_attention_hd(mcm_handle* h, int32_t prec, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                              int32_t heads, int32_t head_dim, int32_t causal, int32_t qrows, int32_t reverse, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_attention(prec, qkv_dev, out_dev, nseq, seq_len, heads, head_dim, causal != 0, qrows, (hipStream_t)stream,
                              reverse != 0, 0, false, h->fault_dev));
  return MCM_OK;
}

// mcm_op_attention_split with the same two launch parameters (the split arm of the model passes qrows = 1 in the CLS-only last
// layer and alternates the walk direction)
int mcm_debug_op_attention_split(mcm_handle* h, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                                 int32_t heads, int32_t qrows, int32_t reverse, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_attention(MCM_PREC_F16, qkv_dev, out_dev, nseq, seq_len, heads, 64, false, qrows, (hipStream_t)stream,
                              reverse != 0, 0, true));
  return MCM_OK;
}

// ... and with the head width: split images "per 64 columns hi[64] then lo[64]" over the whole heads x head_dim row, so at
// head_dim 80 a head straddles blocks (column c of a row at (c / 64) 128 + c % 64, lo 64 further)
int mcm_debug_op_attention_split_hd(mcm_handle* h, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                                    int32_t heads, int32_t head_dim, int32_t qrows, int32_t reverse, void* stream) {
  if (!h) return MCM_EINVAL;
  HIP_TRY(h, launch_attention(MCM_PREC_F16, qkv_dev, out_dev, nseq, seq_len, heads, head_dim, false, qrows, (hipStream_t)stream,
                              reverse != 0, 0, true));
  return MCM_OK;
}

// The front of encode_image_impl (vision_front: the same calls on the handle's own weights and workspace), stopped at `stage`
// (0: behind the patch GEMM, 1: behind launch_layernorm_pre), with the fp32 residual rows [B ntok, D] copied to resid_out_dev
// and, at stage 1, the operand rows h->ln (16-bit / fp32 [B ntok, D], or the split image [B ntok, 2 D]) to ln_out_dev.
// poison: the patch matrix and the residual rows of this batch are filled with 0xFF bytes first (NaN as bf16, fp16 and fp32):
// a pad column that is not written as zero, or a CLS row read instead of synthesised, shows as a NaN.
int mcm_debug_vision_front(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t x2, int32_t B, int32_t stage,
                           int32_t poison, float* resid_out_dev, void* ln_out_dev, void* stream) {
  if (int rc = check_pixel_format(h, pixel_format)) return rc;
  int rc = check_image_call(h, pixels_dev, resid_out_dev, B, x2 != 0);
  if (rc) return rc;
  if (stage < 0 || stage > 1 || (stage == 1 && !ln_out_dev)) return fail(h, MCM_EINVAL, "stage 0 or 1; stage 1 needs ln_out_dev");
  hipStream_t s = (hipStream_t)stream;
  const size_t es = (size_t)prec_esize(h->cfg.precision) * (x2 ? 2 : 1), rows = (size_t)B * h->ntok, D = (size_t)h->cfg.v_width;
  if (poison) {
    HIP_TRY(h, hipMemsetAsync(h->patches, 0xFF, (size_t)B * h->np * h->kpad * es, s));
    HIP_TRY(h, hipMemsetAsync(h->x, 0xFF, rows * D * sizeof(float), s));
  }
  if ((rc = vision_front(h, s, pixels_dev, pixel_format == MCM_PIXELS_U8_NHWC, B, x2 != 0, stage))) return rc;
  HIP_TRY(h, hipMemcpyAsync(resid_out_dev, h->x, rows * D * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (stage == 1) HIP_TRY(h, hipMemcpyAsync(ln_out_dev, h->ln, rows * D * es, hipMemcpyDeviceToDevice, s));
  return MCM_OK;
}

// launch_pool_project as the towers call it: the pooled rows of x [x_rows, D] by index (row_idx_host, n entries) or by stride
// (row_idx_host NULL).  The indices come from the host and are checked against x_rows here (the towers compute theirs on the
// host as well); the call synchronises the stream.
int mcm_debug_op_pool_project(mcm_handle* h, const float* x_dev, int64_t x_rows, const int32_t* row_idx_host, int32_t row_stride,
                              int32_t n, int32_t D, const float* gamma_dev, const float* beta_dev, float eps,
                              const float* proj_dev, int32_t P, float* out_dev, int32_t normalize, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!x_dev || !gamma_dev || !beta_dev || !proj_dev || !out_dev || n <= 0 || D <= 0 || P <= 0 || x_rows <= 0 || row_stride < 0)
    return fail(h, MCM_EINVAL, "bad argument");
  if (row_idx_host) {
    for (int32_t i = 0; i < n; ++i)
      if (row_idx_host[i] < 0 || row_idx_host[i] >= x_rows) return fail(h, MCM_EINVAL, "row index outside x");
  } else if ((int64_t)(n - 1) * row_stride >= x_rows) {
    return fail(h, MCM_EINVAL, "strided rows outside x");
  }
  hipStream_t s = (hipStream_t)stream;
  int32_t* idx_dev = nullptr;
  if (row_idx_host) {
    HIP_TRY(h, hipMalloc((void**)&idx_dev, (size_t)n * sizeof(int32_t)));
    hipError_t e = hipMemcpy(idx_dev, row_idx_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(idx_dev);
      HIP_TRY(h, e);
    }
  }
  hipError_t e = launch_pool_project(x_dev, idx_dev, row_stride, n, D, gamma_dev, beta_dev, eps, proj_dev, P, out_dev, s,
                                     normalize != 0);
  const bool refused = e == hipErrorInvalidValue;  // the launcher's own shape guard: nothing was launched
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (idx_dev) (void)hipFree(idx_dev);
  if (refused) return fail(h, MCM_EINVAL, "launch_pool_project refused the shape (D <= 1280, D % 4 == 0 — D % 64 == 0 past 1024 —, P <= 1024)");
  HIP_TRY(h, e);
  return MCM_OK;
}

// launch_text_embed: x[k S + s] = tok[ids[k S + s]] + pos[s]; tok [vocab, D], pos [>= S rows, D].  The ids come from the host
// and are checked against vocab here, as mcm_encode_text_ex checks its own; the call synchronises the stream.
int mcm_debug_op_text_embed(mcm_handle* h, const int32_t* ids_host, int32_t vocab, const float* tok_dev, const float* pos_dev,
                            float* x_dev, int32_t K, int32_t S, int32_t D, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!ids_host || !tok_dev || !pos_dev || !x_dev || K <= 0 || S <= 0 || D <= 0 || vocab <= 0) return fail(h, MCM_EINVAL, "bad argument");
  const size_t nid = (size_t)K * S;
  for (size_t i = 0; i < nid; ++i)
    if (ids_host[i] < 0 || ids_host[i] >= vocab) return fail(h, MCM_EINVAL, "token id out of range");
  hipStream_t s = (hipStream_t)stream;
  int32_t* ids_dev = nullptr;
  HIP_TRY(h, hipMalloc((void**)&ids_dev, nid * sizeof(int32_t)));
  hipError_t e = hipMemcpy(ids_dev, ids_host, nid * sizeof(int32_t), hipMemcpyHostToDevice);
  bool refused = false;
  if (e == hipSuccess) {
    e = launch_text_embed(ids_dev, tok_dev, pos_dev, x_dev, K, S, D, s);
    refused = e == hipErrorInvalidValue;  // the launcher's own shape guard: nothing was launched
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(ids_dev);
  if (refused) return fail(h, MCM_EINVAL, "launch_text_embed refused the shape (D % 4 == 0)");
  HIP_TRY(h, e);
  return MCM_OK;
}

// launch_text_embed_ctx: mcm_debug_op_text_embed with a slot per position — slot -1: tok[ids], slot j >= 0: row j of the prompt's
// set in ctx [n_sets, n_ctx, D] (n_sets 1 or K).  Ids and slots come from the host and are checked here, as mcm_encode_text_ctx
// checks its own, and folded into one word per position the same way; the call synchronises the stream.
int mcm_debug_op_text_embed_ctx(mcm_handle* h, const int32_t* ids_host, const int32_t* slot_host, int32_t vocab,
                                const float* tok_dev, const float* pos_dev, const float* ctx_dev, int32_t n_ctx, int32_t n_sets,
                                float* x_dev, int32_t K, int32_t S, int32_t D, void* stream) {
  if (!h) return MCM_EINVAL;
  if (!ids_host || !slot_host || !tok_dev || !pos_dev || !ctx_dev || !x_dev || K <= 0 || S <= 0 || D <= 0 || vocab <= 0 || n_ctx <= 0)
    return fail(h, MCM_EINVAL, "bad argument");
  if (n_sets != 1 && n_sets != K) return fail(h, MCM_EINVAL, "n_sets must be 1 or K");
  const size_t nid = (size_t)K * S;
  std::vector<int32_t> words(nid);
  for (size_t i = 0; i < nid; ++i) {
    if (ids_host[i] < 0 || ids_host[i] >= vocab) return fail(h, MCM_EINVAL, "token id out of range");
    if (slot_host[i] < -1 || slot_host[i] >= n_ctx) return fail(h, MCM_EINVAL, "context slot out of range (-1 .. n_ctx - 1)");
    words[i] = slot_host[i] >= 0 ? -(slot_host[i] + 1) : ids_host[i];
  }
  hipStream_t s = (hipStream_t)stream;
  int32_t* words_dev = nullptr;
  HIP_TRY(h, hipMalloc((void**)&words_dev, nid * sizeof(int32_t)));
  hipError_t e = hipMemcpy(words_dev, words.data(), nid * sizeof(int32_t), hipMemcpyHostToDevice);
  bool refused = false;
  if (e == hipSuccess) {
    e = launch_text_embed_ctx(words_dev, tok_dev, pos_dev, ctx_dev, x_dev, K, S, D, n_ctx, n_sets, 0, s);
    refused = e == hipErrorInvalidValue;  // the launcher's own shape guard: nothing was launched
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(words_dev);
  if (refused) return fail(h, MCM_EINVAL, "launch_text_embed_ctx refused the call (D % 4 == 0, ctx 16-byte aligned)");
  HIP_TRY(h, e);
  return MCM_OK;
}

// The activation workspace and the feature scratch filled with one byte value over their full allocated sizes, pad rows
// included (include/mcm_debug_workspace.h): data only, no ring, counter, weight, index buffer or fault word
int mcm_debug_workspace_fill(mcm_handle* h, int32_t byte, void* stream) {
  if (!h) return MCM_EINVAL;
  if (byte < 0 || byte > 255) return fail(h, MCM_EINVAL, "byte 0 ... 255");
  hipStream_t s = (hipStream_t)stream;
  const size_t feat_bytes = (size_t)h->cfg.max_batch * h->cfg.proj_dim * sizeof(float);
  const std::pair<void*, size_t> bufs[] = {{h->x, h->x_bytes},     {h->ln, h->ln_bytes},           {h->qkv, h->qkv_bytes},
                                           {h->att, h->att_bytes}, {h->hbuf, h->hbuf_bytes},       {h->patches, h->patches_bytes},
                                           {h->feat, feat_bytes}};
  for (const auto& b : bufs)
    if (b.first && b.second) HIP_TRY(h, hipMemsetAsync(b.first, byte, b.second, s));
  return MCM_OK;
}

// The walk direction the next launch of the handle's towers takes (next_dir): read into *parity_out (may be NULL), then set to
// `set` where that is 0 or 1 (-1: left as it is).  Host state only.
int mcm_debug_walk_parity(mcm_handle* h, int32_t set, int32_t* parity_out) {
  if (!h || set < -1 || set > 1) return MCM_EINVAL;
  if (parity_out) *parity_out = h->flip ? 1 : 0;
  if (set >= 0) h->flip = set != 0;
  return MCM_OK;
}

int mcm_debug_gemm_dbg(int32_t bits) {  // ablation / A-B bits of gemm.hip (GemmArgs::dbg)
  gemm_set_dbg(bits);
  return MCM_OK;
}

int mcm_debug_ln_fold(int32_t on) {  // 0 (shipped behaviour): every LayerNorm as its own launch; 1: folded where the GEMMs qualify
  g_ln_fold = on ? 1 : 0;
  return MCM_OK;
}

int mcm_debug_ln_tail(int32_t on) {  // 1: LayerNorm in the tail of the residual GEMMs; 0 (shipped behaviour): LayerNorm launches
  g_ln_tail = on ? 1 : 0;
  return MCM_OK;
}
int mcm_debug_ln_cluster(int32_t on) {  // 1: LayerNorm by the row panel's cluster of workgroups (gemm_arms.hpp LNC); 0 (shipped behaviour): LayerNorm launches
  g_ln_cluster = on ? 1 : 0;
  return MCM_OK;
}
int mcm_debug_ln_row(int32_t on) {  // 1: out-proj / fc2 + LayerNorm as 64-row full-row tiles (gemm_arms.hpp ROW64); 0 (shipped behaviour): launches
  g_ln_row = (on >= 1 && on <= 4) ? on : 0;   // 2 / 4: three W stages per wave (N = 768); 3 / 4: W in the blocked layout
  return MCM_OK;
}
int mcm_debug_ln_cluster_spin(int32_t polls) {  // < 0: the first LNC form (waits); n >= 0: the defer form with n polls (and the clean-up launch)
  g_lnc_spin = polls < 0 ? -1 : polls;
  return MCM_OK;
}
int mcm_debug_ln_cluster_deferred(mcm_handle* h, uint64_t* count_host) {  // segments the clean-up kernel normalised since mcm_create
  if (!h || !count_host) return MCM_EINVAL;
  *count_host = 0;
  if (!h->ln_state) return MCM_OK;
  HIP_TRY(h, hipDeviceSynchronize());
  for (int x = 0; x < 8; ++x) {
    unsigned int v = 0;
    HIP_TRY(h, hipMemcpy(&v, h->ln_state + (size_t)x * h->ln_rs + 2 * h->ln_cap8 + 3, sizeof(v), hipMemcpyDeviceToHost));
    *count_host += v;
  }
  return MCM_OK;
}
int mcm_debug_ln_tail_timeouts(mcm_handle* h, uint64_t* count_host) {  // tickets that gave up waiting (0 in a correct run)
  if (!h || !count_host) return MCM_EINVAL;
  *count_host = 0;
  if (!h->ln_state) return MCM_OK;
  HIP_TRY(h, hipDeviceSynchronize());
  for (int x = 0; x < 8; ++x) {
    unsigned int v = 0;
    HIP_TRY(h, hipMemcpy(&v, h->ln_state + (size_t)x * h->ln_rs + h->ln_cap8 + 2, sizeof(v), hipMemcpyDeviceToHost));
    *count_host += v;
  }
  return MCM_OK;
}
int mcm_debug_qkv_head_major(int32_t on) {
  g_qkv_head_major = on ? 1 : 0;
  return MCM_OK;
}
int mcm_debug_patch_fold(int32_t on) {  // 1 (shipped): the patch GEMM gathers pixels itself; 0: patchify + plain GEMM
  g_patch_fold = on ? 1 : 0;
  return MCM_OK;
}
int mcm_debug_persistent_grid(int32_t n) {  // 0 (shipped): one workgroup per CU; n: the persistent GEMMs take n CUs (a multiple of 8)
  if (n < 0 || n % 8 != 0) return MCM_EINVAL;
  gemm_set_persistent_grid(n);
  return MCM_OK;
}
int mcm_debug_resize_fused_only(int32_t on) {  // 0 (shipped): LDS form where the window fits; 1: the fused form everywhere
  g_resize_fused_only = on ? 1 : 0;
  return MCM_OK;
}
int mcm_debug_gemm_group_n(int32_t gn) {  // 0 (default): the plain n-fastest walk; g > 0: N tiles walked in groups of g (arms kernel, variant 9)
  if (gn < 0 || gn > 64) return MCM_EINVAL;
  gemm_set_group_n(gn);
  return MCM_OK;
}
int mcm_debug_nsplit(int32_t n) {  // 1 (shipped): one launch per GEMM; 2 / 3 / 4: QKV and fc1 as n column-block launches
  if (n < 1 || n > 4) return MCM_EINVAL;
  g_nsplit = n;
  return MCM_OK;
}
int mcm_debug_qkv_chunks(int32_t n) {
  if (n < 1 || n > 16) return MCM_EINVAL;
  g_qkv_chunks = n;
  return MCM_OK;
}

int mcm_debug_gemm_variant(int32_t variant) {
  if (variant != -1 && variant != 0 && variant != 3 && variant != 4 && variant != 5 && variant != 9 && variant != 11) return MCM_EINVAL;
  gemm_set_variant(variant);
  return MCM_OK;
}

#endif

}  // extern "C"
