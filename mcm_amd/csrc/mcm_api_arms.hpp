// mcm_api_arms.hpp — the host side of the A/B laboratory: what mcm_api.hip needs to drive the kernel arms of gemm_arms.hpp.
// mcm_api.hip includes it only in the A/B builds (-DMCM_HARNESS: libmcm_hip_harness.so; -DMCM_LN_FOLD / -DMCM_LN_TAIL:
// libmcm_hip_fold.so / libmcm_hip_tail.so), in front of its launch wrappers: libmcm_hip.so does not contain a line of this
// file.  There the handle carries no arm field, the switches the shipped code reads are constants and `Arms` is an empty type
// whose every answer is a compile-time "no" (mcm_api.hip, beside the include).
//
// Six closed experiments live in `Arms`, the per-call plan run_layers asks at three points — LayerNorm fold, LayerNorm in the
// GEMM tail, LayerNorm by cluster (LNC; wait and defer forms), ROW64 (with and without blocked W), head-major qkv, QKV +
// attention per batch chunk — and three more in the hooks of the wrappers: the n-split of gemm(), MCM_ABL_SKIP_LN of lnorm()
// and g_patch_fold of vision_front.  None of them knows exact GELU, the split-activation arm, head_dim 80 or split weights:
// the plan refuses those itself (arms_ok, can_fold), so run_layers never has to.
#pragma once

namespace {
// arm-only operands of one vision layer (the text tower runs fp32: no arm takes it)
struct ArmLayerW {
  // LayerNorm fold (vision tower, 16-bit modes): c = W gamma and b' = b + W beta of the two GEMMs that follow a LayerNorm
  float *cqkv = nullptr, *bqkvf = nullptr, *c1 = nullptr, *b1f = nullptr;
  // ROW64 arm, blocked W (harness; built on first use): wo / w2 as [K-step of 32][16-row block][1 KiB piece, chunks XOR-ed] — the
  // LDS image of a piece, contiguous in memory, so that every LDS-DMA piece is eight whole cache lines (gemm_arms.hpp ROW64)
  void *wo_blk = nullptr, *w2_blk = nullptr;
};
}  // namespace

struct mcm_handle : HandleCore {
  std::vector<ArmLayerW> lw;  // per vision layer (build_layer)
  float2 *fold_part = nullptr, *fold_rs = nullptr;  // LayerNorm fold: row moments [v_width / 64][rows], (rstd, mean rstd) [rows]
  // LayerNorm in the tail of the residual GEMMs (gemm.hip): per-XCD regions of counters, all zero between launches;
  // nullptr when the device did not pass the workgroup -> XCD check (xcd_round_robin) or the widths do not qualify
  unsigned int* ln_state = nullptr;
  int ln_rs = 0, ln_cap8 = 0;
};

namespace {

// the launch wrappers of mcm_api.hip, defined behind this header
hipError_t gemm(mcm_handle* h, hipStream_t s, int prec, int epi, const GemmArgs& a_in);
hipError_t attn(mcm_handle* h, hipStream_t s, int prec, int nseq, int L, int heads, int hd, bool causal, int qrows, int seq0, int hm,
                bool split);

// ---- the switches (harness: mcm_debug_*; the fold / tail builds: constants) ---------------------------------------------
#ifdef MCM_HARNESS
int g_patch_fold = 1;  // A/B (mcm_debug_patch_fold): 0 = patchify + plain patch GEMM (rounds 1 - 3), 1 = pixel-gathering patch GEMM
int g_resize_fused_only = 0;  // A/B (mcm_debug_resize_fused_only): 1 = the resize kernel's rounds-2/3 form everywhere
int g_nsplit = 1;  // A/B (mcm_debug_nsplit): the wide store GEMMs (QKV, fc1) as n launches over column blocks of N / n
// A/B arm (harness: mcm_debug_qkv_head_major): qkv of the 16-bit towers head-major ([3 heads][rows][64],
// GemmArgs::hm) between the QKV projection and attention.  Bit-identical; attention 1.63 -> 1.56 ms per step, the QKV
// projection's stores +0.04 ... 0.08 ms: no net gain, the shipped library keeps [rows][3 D].
int g_qkv_head_major = 0;
int g_qkv_chunks = 1;  // A/B: QKV projection + attention per chunk of the batch (qkv of a chunk stays in the Infinity Cache)
int g_ln_fold = 0;     // A/B: 1 = LayerNorm fold (mcm_debug_ln_fold); 0 = every LayerNorm as its own launch (shipped)
// LayerNorm in the tail of the residual GEMMs (gemm.hip "LayerNorm in the tail"): 1 = the LayerNorm that follows a
// whole-batch out-proj / fc2 of a 16-bit tower is computed by that GEMM's own waves; 0 = every LayerNorm is a launch
// An A/B arm: bit-identical, equal at ViT-B/16 batch 512, +0.5 % at ViT-L/14, -1 ... -7 % on smaller problems
int g_ln_tail = 0;  // mcm_debug_ln_tail
int g_ln_cluster = 0;  // mcm_debug_ln_cluster: LayerNorm by the row panel's cluster of workgroups (gemm_arms.hpp "LNC", round 6)
int g_ln_row = 0;      // mcm_debug_ln_row: out-proj / fc2 + the LayerNorm behind them as 64-row FULL-ROW tiles (gemm_arms.hpp ROW64, R6.7)
int g_lnc_spin = -1;   // mcm_debug_ln_cluster_spin: < 0 the first form (wait for the partners); n >= 0 the defer form: n polls, then
                       // the segment is left to launch_lnc_cleanup behind the GEMM
#else
constexpr int g_patch_fold = 1, g_resize_fused_only = 0, g_qkv_head_major = 0, g_qkv_chunks = 1;
constexpr int g_ln_cluster = 0, g_lnc_spin = -1, g_ln_row = 0;
#ifdef MCM_LN_FOLD  // A/B build of the shipped library with the fold on (make fold: libmcm_hip_fold.so, tools/bench_with_lib.py)
constexpr int g_ln_fold = 1, g_ln_tail = 0;
#else               // MCM_LN_TAIL: A/B build of the shipped library with the tail on
constexpr int g_ln_fold = 0, g_ln_tail = 1;
#endif
#endif

// The tail's coherence argument needs every workgroup with the same blockIdx & 7 on the same XCD (one L2).  That is
// how the dispatcher deals workgroups in the default (SPX) mode; it is checked on the device, once per handle, with
// the grid the persistent kernels use: XCC_ID of every workgroup.  Anything else (another partition mode, a masked
// lease) and the tail is simply not used.
__global__ void xcc_probe_kernel(unsigned int* out) {
  if (threadIdx.x == 0) {
    unsigned int id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    out[blockIdx.x] = id & 0xfu;
  }
}
bool xcd_round_robin(mcm_handle* h, int grid) {
  if (grid < 8 || grid % 8 || grid > 1024) return false;
  unsigned int* dev = nullptr;
  if (hipMalloc((void**)&dev, (size_t)grid * sizeof(unsigned int)) != hipSuccess) return false;
  std::vector<unsigned int> ids((size_t)grid, 0xffu);
  bool ok = true;
  for (int rep = 0; rep < 3 && ok; ++rep) {  // (the mapping must not depend on what ran before)
    hipLaunchKernelGGL(xcc_probe_kernel, dim3(grid), dim3(512), 0, 0, dev);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(ids.data(), dev, (size_t)grid * sizeof(unsigned int), hipMemcpyDeviceToHost) == hipSuccess;
    for (int b = 0; ok && b < grid; ++b) ok = ids[(size_t)b] == ids[(size_t)(b & 7)];
    for (int i = 0; ok && i < 8; ++i)
      for (int j = 0; ok && j < i; ++j) ok = ids[(size_t)i] != ids[(size_t)j];
  }
  (void)hipFree(dev);
  return ok;
}

hipError_t fold_stats(mcm_handle* h, hipStream_t s, int Mp, int D) {
  Scope sc(h, s, MCM_KC_LAYERNORM, 4.0 * Mp * (D / 64));
  return launch_fold_stats(h->fold_part, D / 64, Mp, D, h->cfg.ln_eps, h->fold_rs, s);
}

// The arms of one run_layers call: which of them this tower, batch and switch setting admit (decided once, in the
// constructor), and the launches each puts in the place of the layer's own.  A question answered `true` means "done here,
// rc says how it went"; `false` means the caller launches what the shipped library launches.
struct Arms {
  mcm_handle* h;
  hipStream_t s;
  const Tower& t;
  const int nseq, L, Mp, D, P;
  const bool pooled_row0, x2;
  ArmLayerW* const lw;  // the vision tower's arm operands; nullptr: the text tower
  int pkind;
  bool can_fold, tail_ok0, cluster_ok, row_ok, tail_ok;
  // LayerNorm fold (mcm_debug_ln_fold(1)), an A/B arm (measured 1 % slower end to end than the LayerNorm launches, DESIGN.md
  // 5.5; the shipped library never takes it).  The LayerNorm between a residual GEMM and the GEMM behind it is not launched:
  // the residual epilogue also writes z = gamma o x (into h->ln, where the LayerNorm output would have gone) and the row
  // moments, fold_stats turns those into (rstd, mean rstd) per row, and the consumer's epilogue normalises (gemm.hip,
  // "LayerNorm fold").  Not for the layer the caller pools row 0 of (its LayerNorms see other rows / strides) and not for
  // layer 0's layer_norm1 (fused with pre_layrnorm by the caller).
  bool folded = false;  // h->ln holds gamma o x and h->fold_rs the row statistics: the next consumer GEMM normalises

  Arms(mcm_handle* h_, hipStream_t s_, const Tower& t_, int nseq_, int L_, bool pooled_row0_, bool x2_)
      : h(h_), s(s_), t(t_), nseq(nseq_), L(L_), Mp((int)padded_rows(h_, nseq_ * L_)), D(t_.D), P(t_.prec),
        pooled_row0(pooled_row0_), x2(x2_), lw(&t_ == &h_->vis && !h_->lw.empty() ? h_->lw.data() : nullptr) {
    // the arms (LayerNorm fold / tail / cluster / ROW64, head-major qkv) know head_dim 64 and widths <= 1024 only
    const bool arms_ok = lw && D / t.heads == 64 && D <= 1024;
    // (the LayerNorm fold's consumer epilogue is QuickGELU only)
    const bool fold_ok = arms_ok && !x2 && t.act != MCM_ACT_GELU;
    // producer form: 1 = fused into the residual GEMM's epilogue (ping-pong kernel), 2 = plain residual GEMM + fold_rows
    // (tile kernel: small batches) - bit-identical; the consumers need a fold epilogue in whichever kernel they take
    pkind = gemm_fold_kind(EPI_RESID, Mp, D);
    can_fold = fold_ok && g_ln_fold && g_qkv_chunks == 1 && h->fold_part && P != MCM_PREC_F32 && !t.split &&
               lw[0].cqkv != nullptr && pkind != 0 && gemm_fold_kind(EPI_STORE, Mp, 3 * D) != 0 &&
               gemm_fold_kind(EPI_GELU, Mp, t.ff) != 0;
    // LayerNorm in the tail: the residual GEMMs of whole-batch layers also produce the LayerNorm that follows them
    tail_ok0 = arms_ok && g_ln_tail && !x2 && !can_fold && !t.split && h->ln_state && Mp % 256 == 0 && Mp / 256 <= h->ln_cap8 * 8 &&
               gemm_ln_tail_ok(P, Mp, D);
    // LayerNorm by the row panel's cluster (LNC, harness arm): the same hand-over of gamma / beta / output / counters, plus the
    // slot-moment buffer; the residual epilogue itself writes the LayerNorm output (no idle-wave tickets, no re-read of x)
    cluster_ok = arms_ok && g_ln_cluster && !g_ln_tail && !x2 && !can_fold && !t.split && h->ln_state && h->fold_part && Mp % 256 == 0 &&
                 2 * ((Mp / 256 + 7) / 8) <= h->ln_cap8 && gemm_ln_tail_ok(P, Mp, D);
    // ROW64 arm (harness): the residual GEMM as 64-row full-row tiles whose epilogue writes x and the LayerNorm output
    row_ok = arms_ok && g_ln_row && !g_ln_tail && !g_ln_cluster && !x2 && !can_fold && !t.split && P != MCM_PREC_F32 && Mp % 64 == 0 &&
             (D == 768 || D == 1024) && t.ff % 128 == 0;
    tail_ok = tail_ok0 || cluster_ok || row_ok;   // any of the arms: the residual GEMM also produces the LayerNorm behind it
  }

  bool took(hipError_t e, const char* what, int& rc) {
    rc = e == hipSuccess ? MCM_OK : fail(h, MCM_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return true;
  }

  hipError_t produce(GemmArgs& g, const float* gamma) {  // residual GEMM + z / moments / statistics
    if (pkind == 1) { g.fold_z = h->ln; g.fold_g = gamma; g.fold_part = h->fold_part; }
    hipError_t e = gemm(h, s, P, EPI_RESID, g);
    if (e == hipSuccess && pkind == 2) {
      Scope sc(h, s, MCM_KC_LAYERNORM, 6.0 * Mp * D);
      e = launch_fold_rows(P, h->x, gamma, h->ln, h->fold_part, Mp, D, s, h->sat_on ? h->sat_dev : nullptr);
    }
    return e == hipSuccess ? fold_stats(h, s, Mp, D) : e;
  }
  void with_tail(GemmArgs& g, const float* gamma, const float* beta) {
    g.ln_g = gamma; g.ln_b = beta; g.ln_y = h->ln; g.ln_eps = h->cfg.ln_eps;
    g.ln_state = h->ln_state; g.ln_rs = h->ln_rs; g.ln_cap8 = h->ln_cap8;
    if (cluster_ok) { g.lnc = 1; g.fold_part = h->fold_part; g.lnc_spin = g_lnc_spin; }
  }
#ifdef MCM_HARNESS
  // LNC defer form: the clean-up launch behind a residual GEMM that ran with GemmArgs::lnc (a few hundred workgroups that read one
  // mask word and exit, plus the segments the GEMM's waves did not wait for)
  hipError_t lnc_cleanup(const float* gamma, const float* beta) {
    if (!cluster_ok || g_lnc_spin < 0) return hipSuccess;
    Scope sc(h, s, MCM_KC_LAYERNORM, 8.0 * Mp * D);
    return launch_lnc_cleanup(P, h->x, gamma, beta, h->ln, h->fold_part, Mp, D, h->cfg.ln_eps, h->ln_state, h->ln_rs, h->ln_cap8, s,
                              h->sat_on ? h->sat_dev : nullptr);
  }
  hipError_t row_gemm(GemmArgs g, const float* gamma, const float* beta, void** blk) {
    g.ln_g = gamma; g.ln_b = beta; g.ln_y = h->ln; g.ln_eps = h->cfg.ln_eps;
    g.M = Mp; g.sat = h->sat_on ? h->sat_dev : nullptr;
    if (g_ln_row >= 3) {   // blocked W: built once per weight (not inside a graph capture: the first call allocates)
      if (!*blk) {
        if (dev_alloc(h, blk, (size_t)g.N * g.K * 2)) return hipErrorOutOfMemory;
        hipError_t e = launch_row64_block_w(g.w, *blk, g.N, g.K, s);
        if (e != hipSuccess) return e;
      }
      g.w = *blk;
      g.wblk = 1;
    }
    Scope sc(h, s, MCM_KC_GEMM, 2.0 * g.M * (double)g.N * g.K, g.N == g.K ? MCM_KC_GEMM_OUTPROJ : MCM_KC_GEMM_FC2);
    return launch_gemm_row64_ln(P, g, s, (g_ln_row == 2 || g_ln_row == 4) ? 3 : 2);
  }
#else  // (the fold / tail builds have neither switch: cluster_ok and row_ok are false)
  hipError_t lnc_cleanup(const float*, const float*) { return hipSuccess; }
  hipError_t row_gemm(GemmArgs, const float*, const float*, void**) { return hipErrorInvalidValue; }
#endif

  // "Decorate this consumer GEMM": the QKV projection (fc1 = false) or fc1 of layer l, about to be launched on h->ln
  void consumer(GemmArgs& a, int l, bool fc1) {
    if (!folded) return;
    folded = false;
    a.bias = fc1 ? lw[l].b1f : lw[l].bqkvf; a.fold_rs = h->fold_rs; a.fold_c = fc1 ? lw[l].c1 : lw[l].cqkv;
  }

  // "QKV projection + attention of a whole-batch layer": `a` is the projection of all nseq sequences.  Taken per chunk of
  // the batch (mcm_debug_qkv_chunks) or with q / k / v handed over head-major (mcm_debug_qkv_head_major): whole-batch
  // launches of a 16-bit tower then write the same bytes into h->qkv in another order (the row-0-only layer and the fp32
  // towers keep [rows][3 D])
  bool qkv_attention(const GemmArgs& a0, int epi, bool causal, int& rc) {
    const int nch = (!x2 && g_qkv_chunks > 1 && nseq % g_qkv_chunks == 0) ? g_qkv_chunks : 1;
    const int hm = (g_qkv_head_major && !x2 && nch == 1 && P != MCM_PREC_F32 && t.heads * 64 == D) ? Mp : 0;
    if (nch == 1 && !hm) return false;
    const int es = prec_esize(P);
    hipError_t e = hipSuccess;
    for (int c = 0; c < nch && e == hipSuccess; ++c) {
      const int sq = nseq / nch, r0 = c * sq * L;
      GemmArgs a = a0;
      a.x = (const char*)a0.x + (size_t)r0 * D * es;
      a.out = (char*)a0.out + (size_t)r0 * 3 * D * es;
      a.M = sq * L;
      a.hm = hm;
      e = gemm(h, s, P, epi, a);
      if (e == hipSuccess) e = attn(h, s, P, sq, L, t.heads, D / t.heads, causal, 0, c * sq, hm, x2);
    }
    return took(e, "QKV projection + attention (A/B arm)", rc);
  }

  // "Residual GEMM and the LayerNorm behind it; did you take it?": g is out-proj (the LayerNorm is layer l's layer_norm2) or
  // fc2 (layer l + 1's layer_norm1: all rows, also in front of a row-0-only layer — but the fold does not reach into that
  // one) of a whole-batch layer; true: x and the LayerNorm's output in h->ln (or what the fold puts there) are on the stream
  bool resid_ln(GemmArgs& g, int l, bool fc2, const float* gamma, const float* beta, int& rc) {
    if (can_fold) {
      if (fc2 && pooled_row0 && l + 1 == t.layers - 1 && L > 1) return false;
      folded = true;
      return took(produce(g, gamma), "residual GEMM + LayerNorm fold (A/B arm)", rc);
    }
    if (row_ok) return took(row_gemm(g, gamma, beta, fc2 ? &lw[l].w2_blk : &lw[l].wo_blk), "ROW64 residual GEMM (A/B arm)", rc);
    if (!tail_ok) return false;
    with_tail(g, gamma, beta);  // the LayerNorm by the residual kernel's idle waves / the panel's cluster
    hipError_t e = gemm(h, s, P, EPI_RESID, g);
    if (e == hipSuccess) e = lnc_cleanup(gamma, beta);
    return took(e, "residual GEMM + LayerNorm in its tail (A/B arm)", rc);
  }

  // ---- the hooks of the wrappers and of the handle's set-up ---------------------------------------------------------------

  // gemm(): the wide store GEMMs as n launches over column blocks (mcm_debug_nsplit)
  static bool column_blocks(mcm_handle* h, hipStream_t s, int prec, int epi, const GemmArgs& a_in, hipError_t& e) {
#ifdef MCM_HARNESS
    const GemmArgs& a = a_in;
    // (N = 3 x 768 / 3 x 1024 / 3072 / 4096 only: like the other arms it does not learn ViT-H/14's 3840 / 5120 columns)
    if (g_nsplit > 1 && (epi == EPI_STORE || epi == EPI_GELU) && a.K <= 1024 && a.N <= 4096 && a.N >= 2048 && a.N % (256 * g_nsplit) == 0 && !a.fold_rs && !a.hm && a.M > 4096) {
      // W re-fetch experiment: the XCD's L2 (4 MiB) cannot hold all of W (fc1: 4.7 MB) beside the X
      // panels in flight, so W streams through it once per tile round; with the columns cut in n blocks only N / n of W
      // is live per launch (X is then read n times).  Same bits (a column's K-sum does not depend on its neighbours).
      const int n = g_nsplit, nb = a.N / n;
      const size_t wrow = (size_t)a.K * prec_esize(prec) * (a.ksplit ? 2 : 1);
      e = hipSuccess;
      g_nsplit = 1;
      for (int i = 0; i < n && e == hipSuccess; ++i) {
        GemmArgs p = a_in;
        p.N = nb;
        p.w = (const char*)a_in.w + (size_t)i * nb * wrow;
        p.bias = a_in.bias ? a_in.bias + (size_t)i * nb : nullptr;
        p.out = (char*)a_in.out + (size_t)i * nb * prec_esize(prec);
        e = gemm(h, s, prec, epi, p);
      }
      g_nsplit = n;
      return true;
    }
#endif
    return false;
  }

  // lnorm(): timing experiment (results are garbage): what a tower without its big LayerNorm launches would cost.
  // MCM_ABL_SKIP_LN=1: nothing in their place; =2: a write of the 16-bit output's size (the extra epilogue store
  // of a LayerNorm folded into the neighbouring GEMMs)
  static bool skip_layernorm(mcm_handle* h, hipStream_t s, int prec, int M, int D, bool out_f32, hipError_t& e) {
#ifdef MCM_HARNESS
    static const char* skip = getenv("MCM_ABL_SKIP_LN");
    if (skip && M > 4096 && !out_f32) {
      e = skip[0] == '2' ? hipMemsetAsync(h->qkv, 0, (size_t)M * D * prec_esize(prec), s) : hipSuccess;  // dead at both LN sites
      return true;
    }
#endif
    return false;
  }

  // mcm_create: the arms' workspace; mv = the vision tower's token rows in whole 256-row tiles
  static int create(mcm_handle* h, int64_t mv) {
    const mcm_config& c = h->cfg;
    int rc = MCM_OK;
#if defined(MCM_HARNESS) || defined(MCM_LN_FOLD)  // LayerNorm fold (A/B arm): row moments and row statistics
    if (!rc && c.precision != MCM_PREC_F32 && c.v_width % 256 == 0 && c.v_mlp % 256 == 0 && c.v_width <= 1024 &&
        c.v_width == c.v_heads * 64) {   // (the arm knows head_dim 64 and widths <= 1024: arms_ok)
      rc = dev_alloc(h, (void**)&h->fold_part, (size_t)(c.v_width / 64) * mv * sizeof(float2));
      if (!rc) rc = dev_alloc(h, (void**)&h->fold_rs, (size_t)mv * sizeof(float2));
    }
#endif
#if defined(MCM_HARNESS) || defined(MCM_LN_TAIL)  // LayerNorm in the tail (A/B arm): its counters, if the device qualifies
    if (!rc && c.precision != MCM_PREC_F32 && (c.v_width == 768 || c.v_width == 1024) && xcd_round_robin(h, gemm_persistent_grid())) {
      h->ln_cap8 = 2 * (int)((mv / 256 + 7) / 8);  // (x 2: the cluster arm counts the upper and lower half of a row panel separately)
      h->ln_rs = (2 * h->ln_cap8 + 4 + 63) / 64 * 64;  // words per XCD region: whole 256-B blocks, no line shared between XCDs
                                                       // ([cap8] counters, 3 words, [cap8] segment masks + 1 word of the LNC defer form)
      const size_t bytes = (size_t)8 * h->ln_rs * sizeof(unsigned int);
      rc = dev_alloc(h, (void**)&h->ln_state, bytes);
      if (!rc && hipMemset(h->ln_state, 0, bytes) != hipSuccess) rc = fail(h, MCM_EHIP, "hipMemset LayerNorm-tail state");
    }
#endif
    return rc;
  }

  // build_tower: layer l's arm operands, behind its weight images (w.wqkv, w.w1, w.bqkv)
  static int build_layer(mcm_handle* h, const Tower& t, int l, const std::string& pre, hipStream_t s) {
    if (&t != &h->vis) return MCM_OK;
    h->lw.resize(t.layers);
    if (h->fold_part && !t.split) {  // LayerNorm fold: the column vectors of the two LayerNorm consumers
      const LayerW& w = t.L[l];
      ArmLayerW& a = h->lw[l];
      const int D = t.D, ff = t.ff;
      int rc;
      if ((rc = dev_alloc(h, (void**)&a.cqkv, (size_t)3 * D * sizeof(float)))) return rc;
      if ((rc = dev_alloc(h, (void**)&a.bqkvf, (size_t)3 * D * sizeof(float)))) return rc;
      if ((rc = dev_alloc(h, (void**)&a.c1, (size_t)ff * sizeof(float)))) return rc;
      if ((rc = dev_alloc(h, (void**)&a.b1f, (size_t)ff * sizeof(float)))) return rc;
      HIP_TRY(h, launch_fold_prep(t.prec, w.wqkv, W(h, pre + ".layer_norm1.weight"), W(h, pre + ".layer_norm1.bias"),
                                  w.bqkv, a.cqkv, a.bqkvf, 3 * D, D, s));
      HIP_TRY(h, launch_fold_prep(t.prec, w.w1, W(h, pre + ".layer_norm2.weight"), W(h, pre + ".layer_norm2.bias"),
                                  W(h, pre + ".mlp.fc1.bias"), a.c1, a.b1f, ff, D, s));
    }
    return MCM_OK;
  }
};

}  // namespace
