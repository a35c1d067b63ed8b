/*
 * mcm.h — C ABI of libmcm_hip.so, the MI355X (gfx950) Maximum-Concept-Matching scorer.
 *
 * The reference (deeplearning-wisc/MCM) has no FFI: its boundary is the duck-typed
 * Python contract of utils/detection_util.py:209-249 (`get_ood_scores_clip`) over a
 * `net` exposing `get_image_features` / `get_text_features` (HF transformers
 * modeling_clip.py:683-753).  This header is the C boundary a maintainer binds
 * *underneath* that contract (ctypes stub: INTEGRATION.md).  Each entry point names the
 * reference interface it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross the boundary;
 *   - every function returns 0 on success or a negative MCM_E* code and never throws;
 *     mcm_last_error(h) returns a human-readable message for the last failure;
 *   - `*_dev` pointers are device (HBM) addresses, `*_host` pointers are host addresses;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); what an entry promises about it is its class
 *     in the "Stream contract" below, which every entry with a `stream` names in the last sentence of its comment;
 *   - the activation workspace is allocated by mcm_create (sized from cfg.max_batch / cfg.max_prompt_tokens); the
 *     entries that allocate later are the host_staged ingest entries, on a first or a growing call;
 *   - one handle is used from one host thread at a time (the reference is
 *     single-threaded: utils/detection_util.py:219);
 *   - a result depends on the call's arguments only, never on earlier calls on the handle: same arguments, same bits; the
 *     workspace needs no initialisation between calls, and mcm_saturation_count counts the calls since its last reset only.
 *
 * Stream contract — every entry with a `stream` parameter is in one of three classes (the table, with the line of code that
 * decides each entry: tests/stream_contract.py; held by tests/test_gpu_stream_contract.py):
 *   replayable     asynchronous on `stream`; no allocation, no host synchronisation, and no host array read at call time.
 *                  The call may be captured into a hipGraph and replayed: a replay computes from what the buffers hold then
 *                  and writes the bits the eager call writes; scalars and pointers are baked into the graph.  Make one call
 *                  with the same arguments outside the capture first (the first launch of a kernel with dynamic LDS raises
 *                  its limit), and keep per-kernel timing (mcm_profile_enable) off while capturing.
 *                  Every entry with a `stream` that is not named under the two classes below.
 *   host_staged    correct on any stream and asynchronous or nearly so, but NOT capturable: the entry reads host arrays at
 *                  call time (they may be reused as soon as it returns), and it waits on an event of its staging ring, or
 *                  drains `stream` before it rewrites its pinned staging buffer, or allocates on a first or a growing call:
 *                  mcm_encode_text, mcm_encode_text_ex, mcm_encode_text_ctx, mcm_resize_crop_u8, mcm_jpeg_reconstruct.
 *   synchronising  returns host results and drains `stream` before it returns: mcm_measures, mcm_saturation_count.
 * ONE STREAM PER HANDLE AT A TIME: the activation workspace, the feature scratch and the pinned staging buffers are the
 * handle's, one of each.  Calls on one handle must be ordered — issued on one stream, or on several ordered by events —;
 * two calls on one handle on two unordered streams race on those buffers (the text path drains only the current call's
 * stream before it rewrites its staging buffer).  Two handles are independent.
 */
#ifndef MCM_H_
#define MCM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCM_ABI_VERSION 5 /* 2: mcm_set_weight takes the host element type; mcm_config.weight_operands; split-weight
                          * arm and mcm_weights_operand_exact; mcm_op_linear_ex / mcm_op_split_weight; the round-2
                          * mcm_debug_* exports live in libmcm_hip_harness.so only
                          * 3: MCM_KC_COUNT 7 -> 11 (per-shape GEMM classes: mcm_profile_read's arrays grew); the
                          * split-activation arm (mcm_score_x2 ...) and the MCM_LINEAR_SPLIT_X / _OUT flags
                          * 4: mcm_config.x2_max_batch (the split-activation workspace is sized by the caller);
                          * mcm_kernel_faults + the sticky fault word (every wait of a persistent kernel is bounded)
                          * 5: mcm_config.v_hidden_act / t_hidden_act (MCM_ACT_*: the MLP activation is a property of the
                          * model; 0 = QuickGELU as before, 1 = exact erf GELU for OpenCLIP-trained checkpoints) and the
                          * MCM_LINEAR_ACT_GELU flag of mcm_op_linear_ex
                          * (still 5) mcm_score_features_topk / mcm_score_topk: two added symbols, no struct, constant or
                          * existing entry changed — a caller built against the earlier ABI 5 header runs unchanged
                          * (still 5) mcm_maha_fit_accumulate: an added symbol, on the same terms
                          * (still 5) mcm_knn_workspace_bytes / mcm_knn_score_features: two added symbols, on the same terms
                          * (still 5) mcm_neglabel_workspace_bytes / mcm_neglabel_score_features: two added symbols, on the same terms
                          * (still 5) mcm_local_workspace_bytes / mcm_local_score_features / mcm_encode_image_local /
                          * mcm_score_glmcm: four added symbols, on the same terms
                          * (still 5) mcm_vim_workspace_bytes / mcm_vim_score_features: two added symbols, on the same terms
                          * (still 5) mcm_encode_text_ctx: an added symbol, on the same terms */

/* error codes */
#define MCM_OK 0
#define MCM_EINVAL (-1)   /* bad argument (shape, size, NULL)                         */
#define MCM_ENOMEM (-2)   /* hipMalloc failed                                         */
#define MCM_EHIP (-3)     /* a HIP runtime call failed                                */
#define MCM_ENOWEIGHT (-4)/* a required parameter was never set                       */
#define MCM_ENAME (-5)    /* unknown parameter name                                   */
#define MCM_ESHAPE (-6)   /* parameter shape does not match the config                */
#define MCM_ERANGE (-7)   /* batch / prompt count / sequence exceeds the config       */

/* arithmetic modes for the GEMM/attention operands of the VISION tower (accumulation is always fp32,
 * the residual stream, LayerNorm statistics, softmax and the whole scoring tail are always fp32).
 * The TEXT tower always runs in MCM_PREC_F32: the prompt bank is encoded once per dataset, off the hot
 * loop, and rounding it would perturb every image's cosines in the same direction. */
#define MCM_PREC_BF16 0   /* bf16 MFMA operands  (v_mfma_f32_16x16x32_bf16)            */
#define MCM_PREC_F32 1    /* exact fp32 MFMA     (v_mfma_f32_16x16x4_f32) — parity arm  */
#define MCM_PREC_F16 2    /* fp16 MFMA operands  (v_mfma_f32_16x16x32_f16): same rate as bf16,
                           * 10-bit mantissa; BASELINE config 4 (ViT-L/14 fp16)        */

/* element type of a host parameter buffer handed to mcm_set_weight */
#define MCM_DT_F32 0
#define MCM_DT_F16 1      /* IEEE binary16 (the dtype OpenAI's CLIP checkpoints carry their Linear / conv weights in) */
#define MCM_DT_BF16 2

/* How the 16-bit vision modes hold a GEMM weight (cfg.weight_operands).  A weight that IS an fp16 (bf16) number —
 * the reference's checkpoints: values trained and released in fp16, widened to fp32 by the HF conversion — is
 * lossless as one 16-bit MFMA operand.  A weight that is not (seeded fp32 parameters, a fine-tuned fp32 checkpoint)
 * would be ROUNDED, a fixed perturbation of the model that moves AUROC / FPR95 by more than the activation rounding
 * does.  The split form keeps such a weight as W_hi + W_lo (two 16-bit operands, 22 significand bits), two MFMAs per
 * fragment pair into the same fp32 accumulator: exact for the weight operand at twice the GEMM work. */
#define MCM_WEIGHTS_AUTO 0   /* split exactly when some GEMM weight of the vision tower does not round-trip through
                              * the operand dtype (counted on the device in mcm_finalize_weights)               */
#define MCM_WEIGHTS_SINGLE 1 /* one rounded operand whatever the values (rounds 1 - 3 behaviour)                 */
#define MCM_WEIGHTS_SPLIT 2  /* always the split form                                                            */

/* MLP activation of a tower (cfg.v_hidden_act / cfg.t_hidden_act) = the `hidden_act` of HF's CLIPVisionConfig /
 * CLIPTextConfig.  OpenAI's checkpoints were trained with QuickGELU; the OpenCLIP-trained ones (LAION-2B, DataComp) that load
 * into the same CLIPModel — same shapes, same state-dict names — with the exact GELU.  The shapes cannot tell them apart: a
 * checkpoint scored with the other activation gives plausible, wrong scores (the two differ by up to 0.020 per element). */
#define MCM_ACT_QUICK_GELU 0 /* x * sigmoid(1.702 x)   (activations.py QuickGELUActivation; "quick_gelu")         */
#define MCM_ACT_GELU 1       /* x * Phi(x), erf form   (activations.py GELUActivation = torch gelu; "gelu")        */

/* score kinds — the epilogues of utils/detection_util.py:233-248 */
#define MCM_SCORE_MCM 0       /* -max_k softmax(cos/T)             (:236,:248) */
#define MCM_SCORE_MAX_LOGIT 1 /* -max_k cos                        (:234,:248) */
#define MCM_SCORE_ENERGY 2    /* -T*logsumexp(cos/T)               (:239)      */
#define MCM_SCORE_ENTROPY 3   /* Shannon entropy of softmax(cos/T) (:243)      */
#define MCM_SCORE_VAR 4       /* -var_k softmax(cos/T), ddof=0     (:246)      */

typedef struct mcm_handle mcm_handle;

/* Model geometry = the fields of transformers CLIPVisionConfig / CLIPTextConfig that
 * the path reads (configuration_clip.py), plus workspace bounds. */
typedef struct mcm_config {
  int32_t abi_version;      /* must be MCM_ABI_VERSION                                */
  int32_t device;           /* HIP device ordinal                                     */
  int32_t precision;        /* MCM_PREC_*                                             */
  /* vision tower (modeling_clip.py:138-218, 594-656) */
  int32_t image_size;       /* 224                                                    */
  int32_t patch_size;       /* 16 (B/16), 32 (B/32), 14 (L/14)                        */
  int32_t v_width;          /* 768 / 1024 / 1280 (ViT-H/14)                           */
  int32_t v_heads;          /* 12 / 16  (head_dim = width / heads: 64, or 80 in the   */
                            /* vision tower only — ViT-H/14; the text tower: 64)      */
  int32_t v_layers;         /* 12 / 24                                                */
  int32_t v_mlp;            /* 3072 / 4096                                            */
  /* text tower (modeling_clip.py:221-256, 494-586) */
  int32_t vocab_size;       /* 49408                                                  */
  int32_t max_positions;    /* 77                                                     */
  int32_t t_width;          /* 512 / 768                                              */
  int32_t t_heads;          /* 8 / 12                                                 */
  int32_t t_layers;         /* 12                                                     */
  int32_t t_mlp;            /* 2048 / 3072                                            */
  int32_t proj_dim;         /* 512 / 768  (visual_projection / text_projection rows)  */
  float ln_eps;             /* 1e-5 (configuration_clip.py layer_norm_eps)            */
  /* workspace bounds */
  int32_t max_batch;        /* images per mcm_encode_image / mcm_score call           */
  int32_t max_prompt_tokens;/* K*S per mcm_encode_text call                           */
  int32_t weight_operands;  /* MCM_WEIGHTS_*; ignored in MCM_PREC_F32                 */
  int32_t x2_max_batch;     /* MCM_PREC_F16 handles: images per mcm_score_x2 / mcm_encode_image_x2 call.  0 = max_batch (the
                             * activation buffers at twice the bytes: +1.5 GB at ViT-B/16 batch 512), n > 0 = at most n (the
                             * buffers hold max(max_batch rows, 2 x the rows of n images): nothing extra for n <= max_batch / 2),
                             * < 0 = no split-activation workspace (those calls return MCM_EINVAL)  */
  int32_t v_hidden_act;     /* MCM_ACT_* of the vision tower's MLPs (ABI 5; 0 = QuickGELU: a zeroed struct is an OpenAI model) */
  int32_t t_hidden_act;     /* MCM_ACT_* of the text tower's MLPs; anything but the two values: MCM_EINVAL from mcm_create */
} mcm_config;

int mcm_abi_version(void);

/* Replaces CLIPModel.__init__ + .cuda() (utils/train_eval_util.py:23-24): allocates the
 * parameter store and the activation workspace on cfg->device.
 *
 * The geometries it accepts — every one of these is a model the kernels compute, held to the CPU oracle and to fp64 operator
 * budgets at points away from the shipped checkpoints (tests/geometry_envelope.py, tests/test_gpu_geometry_envelope.py);
 * anything else is MCM_EINVAL with the rule in mcm_last_error(NULL), before any device memory is touched:
 *   v_width        64 * v_heads with v_heads = 1 ... 20, or 80 * v_heads with 80 * v_heads a multiple of 64 (4, 8, 12, 16
 *                  heads); 320 is both 5 heads of 64 and 4 heads of 80, and v_heads says which
 *   t_width        64 * t_heads, at most 1024 (the text tower has no 80-wide heads)
 *   v_mlp, t_mlp   any multiple of 64
 *   proj_dim       any multiple of 4 up to 1024
 *   patch_size     any divisor of image_size that leaves at most 1025 vision tokens ((image_size / patch_size)^2 + 1);
 *                  image_size == patch_size is the 2-token tower
 *   v_layers, t_layers   at least 1 (a one-layer tower is its first and its last layer at once; there is no zero-layer tower)
 *   max_positions  1 ... 306: the text tower's causal fp32 attention keeps K, V and the logits of a head in LDS, and 306 tokens
 *                  are the longest prompt that fits (Long-CLIP's 248 does); at most max_prompt_tokens
 *   vocab_size     any; v_hidden_act, t_hidden_act: MCM_ACT_QUICK_GELU or MCM_ACT_GELU
 * A prompt longer than max_positions is MCM_ERANGE from mcm_encode_text*, as HF raises. */
int mcm_create(const mcm_config* cfg, mcm_handle** out);
void mcm_destroy(mcm_handle* h);
const char* mcm_last_error(const mcm_handle* h); /* h may be NULL: last create error */

/* Replaces load_state_dict / from_pretrained (utils/train_eval_util.py:23): copies one
 * parameter, keyed by its HF state_dict name, host → device.  `dtype` = MCM_DT_*: the element
 * type of host_ptr (an fp16 / bf16 checkpoint is handed over as it is; the fp32 master the library keeps is the exact
 * widening).  The caller keeps ownership of host_ptr.  `shape`/`ndim` are checked against cfg. */
int mcm_set_weight(mcm_handle* h, const char* hf_name, const void* host_ptr, int32_t dtype,
                   const int64_t* shape, int32_t ndim);
/* Verifies every parameter was set, counts the vision-tower GEMM weights that are not exactly representable in the
 * operand dtype, chooses the weight form (cfg.weight_operands) and builds the packed operand copies the kernels
 * read (concatenated QKV, 16-bit or split copies).  Must be called once before any encode. */
int mcm_finalize_weights(mcm_handle* h);
/* After mcm_finalize_weights: *inexact_host = number of GEMM-weight elements of the vision tower (q/k/v/out_proj, fc1,
 * fc2 of every layer and the patch embedding) whose fp32 value is not an fp16 (bf16 in MCM_PREC_BF16) number — 0 for the
 * reference's checkpoints in fp16, ~99.9 % of the elements for fp32-valued parameters; always 0 in MCM_PREC_F32.
 * *split_host = 1 when the handle runs the split-weight GEMMs (MCM_WEIGHTS_*), else 0.  Either pointer may be NULL. */
int mcm_weights_operand_exact(mcm_handle* h, uint64_t* inexact_host, int32_t* split_host);

/* Replaces `net.get_text_features(input_ids, attention_mask).float()` followed by
 * `/= norm` (utils/detection_util.py:229-231; modeling_clip.py:683-715).
 * ids_host: int32 [K,S] row-major, each row BOS … EOS pad…; the pooled row is the
 * first EOS (= argmax id, modeling_clip.py:561-581).  attention_mask is not needed:
 * the mask is causal and pooling reads the first EOS.
 * out_dev: fp32 [K, proj_dim], L2-normalised rows.
 * The prompts run in passes of max_prompt_tokens / S; before each pass, the first included, the call drains `stream` and
 * stages the pass's ids through the handle's pinned buffer.  Stream contract: host_staged. */
int mcm_encode_text(mcm_handle* h, const int32_t* ids_host, int32_t K, int32_t S,
                    float* out_dev, void* stream);

/* Replaces `net.get_image_features(pixel_values=images).float()` followed by `/= norm`
 * (utils/detection_util.py:225-226; modeling_clip.py:719-753).
 * pixels_dev: fp32 NCHW [B,3,image_size,image_size] contiguous, already normalised by
 * the preprocess of utils/train_eval_util.py:27-33.
 * out_dev: fp32 [B, proj_dim], L2-normalised rows.  Stream contract: replayable. */
int mcm_encode_image(mcm_handle* h, const float* pixels_dev, int32_t B, float* out_dev,
                     void* stream);

/* The two calls above with the reference's `/= norm` step optional: normalize == 0 returns exactly what
 * HF `get_image_features` / `get_text_features` return (modeling_clip.py:751,713 — the projection
 * output), which is what unmodified reference code expects from `net` (utils/detection_util.py:158,
 * 187,225,229) before it normalises the rows itself.  pixel_format selects the ingest layout.
 * mcm_encode_image_ex — Stream contract: replayable. */
#define MCM_PIXELS_F32_NCHW 0 /* fp32 [B,3,S,S], already normalised (mcm_encode_image)            */
#define MCM_PIXELS_U8_NHWC 1  /* uint8 [B,S,S,3]; ToTensor + Normalize fused (mcm_encode_image_u8) */
int mcm_encode_image_ex(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B,
                        int32_t normalize, float* out_dev, void* stream);
/* mcm_encode_text with `normalize` (above); staged as mcm_encode_text is.  Stream contract: host_staged. */
int mcm_encode_text_ex(mcm_handle* h, const int32_t* ids_host, int32_t K, int32_t S, int32_t normalize,
                       float* out_dev, void* stream);

/* Learned prompt contexts.  Replaces CoOp's `PromptLearner.forward` + `TextEncoder.forward` (Zhou et al., "Learning to Prompt
 * for Vision-Language Models"; LoCoOp trains the same module): token-embed the tokenised prompt "X X ... X classname.",
 * overwrite the n_ctx placeholder positions with the learned vectors, add the position embedding, run the unchanged
 * transformer, ln_final, pool at `tokenized_prompts.argmax(-1)`, project.  It is mcm_encode_text_ex with the embedding step
 * replaced — the same passes of max_prompt_tokens / S prompts, the same layers, the same pooling kernel:
 *   x[k, s] = (slot[k, s] < 0 ? token_embedding[ids[k, s]] : ctx[set(k), slot[k, s]]) + position_embedding[s]
 * ids_host / slot_host: int32 [K,S] row-major, host memory.  slot -1 = an ordinary token; slot j in [0, n_ctx) = row j of the
 * prompt's context set.  The id under a context slot is a placeholder (CoOp's "X"): it is not looked up, but it takes part in
 * pooling like any id — the pooled row is the first position of the largest id of ids_host — and must be a valid id.
 * ctx_dev: fp32 [n_sets, n_ctx, t_width], device memory, 16-byte aligned; set(k) = 0 when n_sets == 1 (CoOp's unified
 * context), k when n_sets == K (class-specific contexts, "CSC").  It is read on `stream`: the caller keeps it alive until the
 * stream has passed the call.  Nothing is allocated: the slot map travels in the id words a pass uploads anyway.
 * out_dev: fp32 [K, proj_dim]; normalize as mcm_encode_text_ex.
 * MCM_EINVAL, with nothing launched: a NULL ids_host / slot_host / ctx_dev / out_dev; K, S or n_ctx < 1; n_sets other than 1 or K;
 * a slot outside -1 ... n_ctx - 1; an id outside the vocabulary; ctx_dev not 16-byte aligned.  MCM_ERANGE: S > max_positions.
 * Staged as mcm_encode_text is (ids and slots are read on the host, `stream` is drained before every pass).
 * Stream contract: host_staged. */
int mcm_encode_text_ctx(mcm_handle* h, const int32_t* ids_host /* [K,S] */, const int32_t* slot_host /* [K,S] */,
                        int32_t K, int32_t S, const float* ctx_dev /* [n_sets, n_ctx, t_width] fp32 */,
                        int32_t n_ctx, int32_t n_sets, int32_t normalize, float* out_dev, void* stream);

/* Replaces the scoring tail utils/detection_util.py:232-248 on already-normalised
 * features: sim = img @ text.T, softmax(sim/T), reduction `kind` → scores_dev fp32 [B].
 * Never materialises [B,K].  Stream contract: replayable. */
int mcm_score_features(mcm_handle* h, const float* img_feat_dev, int32_t B,
                       const float* text_feat_dev, int32_t K, float T, int32_t kind,
                       float* scores_dev, void* stream);

/* One batch of the whole hot loop body utils/detection_util.py:223-248:
 * mcm_encode_image + mcm_score_features, text bank pre-encoded (hoisted out of the
 * loop; the reference re-encodes it every batch with identical results).  Stream contract: replayable. */
int mcm_score(mcm_handle* h, const float* pixels_dev, int32_t B, const float* text_feat_dev,
              int32_t K, float T, int32_t kind, float* scores_dev, void* stream);

/* ---- top-k matched concepts next to every score (added under ABI 5: symbols only) ---------------------------------
 * Replaces what a consumer of the reference does with the [B,K] softmax it pulls to the host
 * (utils/detection_util.py:232-236: `output = image_features @ text_features.T`, `smax = softmax(output / T)`)
 * to learn WHICH concept an image matched — np.argmax / argsort of smax per row, the zero-shot prediction the MCM
 * paper reports top-1 / top-5 accuracy of.  The same single launch as mcm_score_features; [B,K] still never
 * reaches HBM, and scores_dev receives the bits mcm_score_features writes for the same arguments.
 *   idx_dev  int32 [B, topk]: the bank rows of the topk largest similarities, 1 <= topk <= MCM_TOPK_MAX, ordered by
 *            value descending, then by row index ascending — numpy.argsort(-sim, kind="stable")[:topk].
 *            Ties: equal similarities (+0.0 and -0.0 are equal) go to the lower index first.
 *            NaN: a NaN similarity is never selected.  A slot with no candidate left (topk > K, or fewer than topk
 *            non-NaN similarities) holds -1.
 *   prob_dev fp32 [B, topk] or NULL: softmax(sim / T)[idx] from the exp terms and the fp64 normaliser of the score
 *            itself, for EVERY kind (MCM_SCORE_MAX_LOGIT then runs the softmax it otherwise skips).  For
 *            MCM_SCORE_MCM on a NaN-free row prob[b,0] == -scores[b] bit for bit.  NaN where idx is -1.
 * Refusals (nothing is launched): MCM_EINVAL for topk outside 1..MCM_TOPK_MAX, a NULL scores_dev / idx_dev, T <= 0,
 * a bad B / K / kind, and the sizes mcm_score_features refuses (proj_dim % 4, (proj_dim + K) * 4 > 150 KiB).
 *
 * mcm_score_topk is one batch of the hot loop body with it (mcm_score / mcm_score_u8 / mcm_score_x2 in one entry):
 * pixel_format is MCM_PIXELS_*; x2 != 0 runs the split-activation arm under the rules of mcm_score_x2 (fp16 handle with
 * the workspace, B <= the arm's largest batch — otherwise MCM_EINVAL / MCM_ERANGE), x2 == 0 the handle's own arm through
 * the encode calls of mcm_score / mcm_score_u8.  Both entries — Stream contract: replayable. */
#define MCM_TOPK_MAX 8
#define MCM_SCORE_LDS_MAX_BYTES 153600 /* 150 KiB: the LDS of the tail that keeps (proj_dim + K) floats per image */
int mcm_score_features_topk(mcm_handle* h, const float* img_feat_dev, int32_t B, const float* text_feat_dev,
                            int32_t K, float T, int32_t kind, int32_t topk, float* scores_dev,
                            int32_t* idx_dev /* [B,topk] */, float* prob_dev /* [B,topk] or NULL */, void* stream);
int mcm_score_topk(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t x2, int32_t B,
                   const float* text_feat_dev, int32_t K, float T, int32_t kind, int32_t topk, float* scores_dev,
                   int32_t* idx_dev, float* prob_dev, void* stream);

/* uint8 ingest: pixels_dev is uint8 NHWC [B,image_size,image_size,3] (what a
 * JPEG decoder + resize/crop produces); ToTensor (/255) and Normalize with the CLIP mean/std of
 * utils/train_eval_util.py:27-33 are fused into the patch gather.  Same results as
 * mcm_encode_image / mcm_score on the equivalent fp32 NCHW tensor.  Both entries — Stream contract: replayable. */
int mcm_encode_image_u8(mcm_handle* h, const uint8_t* pixels_dev, int32_t B, float* out_dev,
                        void* stream);
int mcm_score_u8(mcm_handle* h, const uint8_t* pixels_dev, int32_t B, const float* text_feat_dev,
                 int32_t K, float T, int32_t kind, float* scores_dev, void* stream);

/* ---- split-activation arm (ABI 3): the re-scorer of threshold refinement ------------------------------------------
 * The same image tower on the same weights and the same workspace, fp16 handles only, with every activation that feeds
 * an MFMA carried as a split pair x = hi + lo of fp16 numbers (~22 significand bits; hi = round(x), lo = round(x - hi))
 * and every GEMM run as X_hi W^T + X_lo W^T in one fp32 accumulator chain — the mirror image of the split-WEIGHT form
 * (MCM_WEIGHTS_SPLIT; with split weights as well: four passes per K-step); attention as three MFMA passes per product.
 * Scores agree with the exact-fp32 arm (MCM_PREC_F32) to fp32 round-off at about half the fp16 arm's throughput, where
 * the fp32 arm runs at a tenth of it: what mcm_amd/refine.py re-scores the images near the FPR95 threshold with
 * (reference utils/detection_util.py:66-106: FPR95 is a count at one threshold).  No second handle, no extra weights:
 * the split rows (twice the width) live in the same activation buffers, which mcm_create sizes for cfg.x2_max_batch images
 * of them: B <= mcm_x2_max_batch(h) (0 = this handle is not fp16, or was created without the workspace).  pixel_format: MCM_PIXELS_*.
 * mcm_encode_image_x2 and mcm_score_x2 — Stream contract: replayable. */
int mcm_x2_max_batch(const mcm_handle* h);
int mcm_encode_image_x2(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, int32_t normalize,
                        float* out_dev, void* stream);
int mcm_score_x2(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, const float* text_feat_dev,
                 int32_t K, float T, int32_t kind, float* scores_dev, void* stream);

/* Resize(S) + CenterCrop(S), S = cfg.image_size, on the device: the first two
 * steps of the reference's loader transform, utils/train_eval_util.py:27-33 (transforms.Resize(224),
 * transforms.CenterCrop(224) on the PIL image; torchvision's size / crop rules around Pillow's
 * antialiased BILINEAR Image.resize).  Bit-exact against Pillow (tests/golden/preprocess.npz).
 * src_dev_ptrs / heights / widths are HOST arrays of length B: device pointers to [H_i, W_i, 3]
 * uint8 RGB images and their sizes.  dst_dev [B, S, S, 3] uint8 is the layout mcm_score_u8 and
 * mcm_encode_image_u8 take.  MCM_ERANGE: B > max_batch, or a scale factor above 31 (more filter
 * taps than the kernel holds).  Asynchronous on `stream`: the geometry is staged through a ring of four pinned buffers, and
 * a call waits only for the copy out of its slot, four calls ago (it never drains the stream), so a batch can be resized
 * while the previous one is being scored.  The host arrays are read at call time; the first call on a handle allocates the
 * kernel's coefficient tables (one synchronous device allocation).  Stream contract: host_staged. */
int mcm_resize_crop_u8(mcm_handle* h, const uint8_t* const* src_dev_ptrs, const int32_t* heights,
                       const int32_t* widths, int32_t B, uint8_t* dst_dev, void* stream);

/* Host side of the raw-image ingest: copies n images (host pointers srcs[i], sizes[i] bytes) to dst + offsets[i] — the ONE
 * pinned buffer a batch is uploaded from with a single asynchronous copy (replaces the loader's per-batch `.cuda()` of
 * reference utils/detection_util.py:222-223) — with `threads` native threads, the work cut by bytes.  Pure host code;
 * MCM_ERANGE when an image does not fit dst_bytes. */
int mcm_pack_u8(const uint8_t* const* srcs, const int64_t* sizes, const int64_t* offsets, int32_t n, uint8_t* dst,
                int64_t dst_bytes, int32_t threads);

/* JPEG ingest, host half (csrc/jpeg_entropy.cpp): file -> markers -> Huffman decode -> quantised DCT coefficients, written by
 * `threads` native threads into dst (the pinned buffer a batch is uploaded from) — the part of the reference loader's
 * `Image.open(path).convert("RGB")` (torchvision ImageFolder, utils/train_eval_util.py:96-146) that is bit-serial; the
 * device half (mcm_jpeg_reconstruct) turns the coefficients into the RGB pixels libjpeg would have produced.
 * Baseline / extended-sequential and progressive Huffman JPEGs are taken.
 * meta[i].status: 0 taken; 1 a JPEG this path does not take (arithmetic, 12-bit, CMYK / RGB-coded, sequential multi-scan,
 * sampling other than 4:4:4 / 4:2:2 / 4:2:0): decode it with the fallback decoder; 2 unreadable, corrupt, or merely
 * suspicious — a scan is taken only if every RSTn and the EOI sit exactly where a clean scan has them and every dequantised
 * coefficient is plausible for 8-bit samples; libjpeg's warn-and-recover output for anything else is the fallback's to give.
 * Component c of image i: int16 [hb][wb][64] coefficients in natural order at dst + coef_off[c]; its quantisation table at
 * quant[(i * 3 + c) * 64].  *bytes_used = bytes of dst the batch needs; MCM_ERANGE (nothing decoded) when dst_bytes is less. */
typedef struct mcm_jpeg_image {
  int32_t status;
  int32_t width, height, ncomp;
  int32_t hs[3], vs[3];   /* sampling factors */
  int32_t wb[3], hb[3];   /* blocks per row / per column of the coefficient planes (whole MCUs) */
  int64_t coef_off[3];
} mcm_jpeg_image;
int mcm_jpeg_entropy_decode(const char* const* paths, int32_t n, void* dst, int64_t dst_bytes, mcm_jpeg_image* meta,
                            uint16_t* quant, int32_t threads, int64_t* bytes_used);

/* JPEG ingest, device half (csrc/jpeg.hip): the coefficients of a batch (uploaded as they were written by
 * mcm_jpeg_entropy_decode; coef_dev = device copy of its dst) -> dequantisation, libjpeg's default inverse DCT
 * (jpeg_idct_islow), fancy chroma upsampling and YCbCr -> RGB: uint8 [height_i, width_i, 3] at rgb_dev + rgb_offsets[i] —
 * byte for byte what Pillow's Image.open(path).convert("RGB") returns (the reference's loader decodes with it).  meta / quant /
 * rgb_offsets are HOST arrays of length n; images whose status is not 0 are skipped (the caller decodes those with its
 * fallback and writes their pixels itself).  Asynchronous on `stream` in the steady state; the output is what
 * mcm_resize_crop_u8 takes.  The host arrays are read at call time into a ring of four pinned buffers (a call waits for the
 * copy out of its slot, four calls ago); the first call on a handle allocates the ring, and a batch whose sample planes
 * exceed the handle's buffer grows it: `stream` is drained, the buffer freed and allocated again.
 * Stream contract: host_staged. */
int mcm_jpeg_reconstruct(mcm_handle* h, const void* coef_dev, const mcm_jpeg_image* meta, const uint16_t* quant, int32_t n,
                         uint8_t* rgb_dev, const int64_t* rgb_offsets, void* stream);

/* Prompt-ensemble bank (BASELINE config 5): feats_dev = unit-norm text
 * features [K*T, proj_dim], class-major (row k*T + t = template t of class k), as written by
 * mcm_encode_text; bank_dev [K, proj_dim] = normalise(mean over the T templates).  The reference
 * ships the 80 templates (utils/imagenet_templates.py) but never calls them; this is the
 * standard CLIP zero-shot recipe.  Stream contract: replayable. */
int mcm_reduce_bank(mcm_handle* h, const float* feats_dev, int32_t K, int32_t T, float* bank_dev,
                    void* stream);

/* Detection metrics on the device: replaces get_measures /
 * fpr_and_fdr_at_recall, reference utils/detection_util.py:66-119, incl. the sklearn
 * roc_auc_score / average_precision_score calls at :115-116.  pos_dev [n_pos] = scores of the
 * ID set (the positive class, :112-113), neg_dev [n_neg] = scores of one OOD set, both device
 * fp32; negate != 0 evaluates on -score, which is how the reference calls it
 * (get_and_print_results, :255: the stored scores are negated confidences).
 * out_host[0..2] = AUROC, AUPR, FPR at the operating point whose recall is closest to
 * recall_level (0.95 in the reference), same tie rules as the reference.  Synchronises `stream`.
 * NON-FINITE SCORES: -inf and +inf are ordinary ordered scores (below / above every finite one, equal to
 * themselves); -0.0 ties +0.0; subnormal scores are distinct numbers.  A NaN has no place in the order: one
 * NaN anywhere in either vector makes all three outputs NaN (the call still returns MCM_OK), never a
 * finite number.  (The host route, sklearn, raises on any non-finite score instead.)
 * Scratch (12 bytes per score) is borrowed from the activation workspace mcm_create sized (the B/16
 * batch-512 workspace holds 25 million scores); larger inputs get a one-off stream-ordered allocation
 * (hipMallocAsync / hipFreeAsync on `stream`).
 * STREAM REQUIREMENT, an instance of "one stream per handle at a time" (Stream contract, above): because the scratch
 * is the workspace of the encode / score calls, `stream` must be the stream those calls were issued on (or be ordered
 * after them by an event): stream order is the only thing that keeps mcm_measures from overwriting a tower's
 * activations in flight.  Stream contract: synchronising. */
int mcm_measures(mcm_handle* h, const float* pos_dev, int64_t n_pos, const float* neg_dev,
                 int64_t n_neg, int32_t negate, double recall_level, double* out_host, void* stream);

/* Fixed-edge histogram of a device score vector: the constant-size per-rank payload `north_star` names
 * ("RCCL all-gather of per-shard score histograms"), summed over ranks by the caller's all-reduce.
 * edges_dev: fp32 [n_bins + 1] ascending; counts_dev: int64 [n_bins], overwritten.  numpy.histogram
 * semantics (bin i = [e_i, e_{i+1}), last bin closed, out-of-range scores dropped); n_bins <= 8192.
 * As numpy does with explicit bins, -inf, +inf and NaN scores are counted nowhere; repeated edges make
 * zero-width bins that stay empty (a score equal to a repeated LAST edge lands in the last bin).  n == 0 is
 * allowed (scores_dev may then be NULL): all counts are zero.  Stream contract: replayable. */
int mcm_score_histogram(mcm_handle* h, const float* scores_dev, int64_t n, const float* edges_dev,
                        int32_t n_bins, int64_t* counts_dev, void* stream);

/* ---- Mahalanobis baseline (--score maha) ---------------------------------------
 * mcm_encode_image_raw: HF get_image_features WITHOUT the reference's `/= norm` — what
 * get_mean_prec / get_Mahalanobis_score consume when args.normalize is False (their default),
 * reference utils/detection_util.py:158-161,187-190.
 * mcm_maha_prepare + mcm_maha_score_features replace the per-class loop of get_Mahalanobis_score
 * (:191-198): means_dev [C, proj_dim] fp32 and prec_dev [proj_dim, proj_dim] fp32 are
 * get_mean_prec's classwise_mean and precision; w_dev [C, proj_dim] and k_dev [C] (fp64) are
 * scratch the caller provides, filled by prepare and read by score; scores_dev [B] receives
 * min_c 0.5 (f - mu_c) P (f - mu_c)^T, the value the reference returns per sample.
 * All three entries — Stream contract: replayable. */
int mcm_encode_image_raw(mcm_handle* h, const float* pixels_dev, int32_t B, float* out_dev, void* stream);
int mcm_maha_prepare(mcm_handle* h, const float* means_dev, const float* prec_dev, int32_t C,
                     double* w_dev, double* k_dev, void* stream);
int mcm_maha_score_features(mcm_handle* h, const float* feats_dev, int32_t B, const float* prec_dev,
                            const double* w_dev, const double* k_dev, int32_t C, float* scores_dev,
                            void* stream);
/* The fit's running statistics (added under ABI 5: a symbol only), what get_mean_prec's covariance needs from a stream
 * of feature batches.  With x_b = (double)feats_dev[b] - (double)shift_dev (shift_dev [proj_dim] fp32, NULL = 0):
 *   gram_dev [proj_dim, proj_dim] += sum_b x_b x_b^T        sum_dev [proj_dim] += sum_b x_b        (fp64, b < B)
 * gram_dev and sum_dev are the caller's, zeroed by the caller before the first batch (like w_dev / k_dev above, the
 * library never allocates them); after n rows  cov = (gram - sum sum^T / n) / (n - 1)  whatever the shift, which is
 * there for the error alone: a shift near the column means (the first batch's) keeps the subtraction from cancelling.
 * Every product is rounded once (fma), an element is accumulated row after row in one thread starting from the value
 * already there: no atomics, the same bits on every run and for every split of the rows into calls.  Only the upper
 * triangle of gram_dev is read; the lower one is written as its mirror image, so gram[i][j] == gram[j][i] bit for bit.
 * Timed under MCM_KC_SCORE.  A replay adds to what gram_dev and sum_dev hold then, as a call does.
 * Refusals (nothing is launched): MCM_EINVAL for a NULL feats_dev / gram_dev / sum_dev or B < 1; MCM_EHIP for a
 * proj_dim beyond 4096, as mcm_maha_score_features.  Stream contract: replayable. */
int mcm_maha_fit_accumulate(mcm_handle* h, const float* feats_dev /* [B, proj_dim] */, int32_t B,
                            const float* shift_dev /* [proj_dim] or NULL */, double* gram_dev, double* sum_dev,
                            void* stream);

/* ---- deep k-nearest-neighbour baseline (--score knn; Sun et al. 2022) --------------------------------
 * The other training-set baseline: the distance from a feature row to its k-th nearest neighbour among the rows of a
 * bank of training features (added under ABI 5: two symbols only).  P = the handle's proj_dim, everything row-major:
 *   s[b, n]     = the fp32 dot product of feats_dev[b] and bank_dev[n]: every product rounded once into one fp32
 *                 accumulator chain over the P columns (the exact-fp32 MFMA), operands never narrowed;
 *   topv[b, :]  = the k largest s[b, .] as a multiset, sorted descending.  A NaN similarity is never selected, -0 and
 *                 +0 compare equal (and are both written as +0), slots with no candidate left (k > N, NaNs) hold -inf;
 *   scores[b]   = (float) sqrt(max(0, 2 - 2 (double) topv[b, k - 1])): for unit-norm rows the Euclidean distance to
 *                 the k-th nearest neighbour; larger = more OOD, the sign every stored score here has; -inf gives +inf.
 * The [B, N] similarities exist in registers and LDS only.  The bank is cut into `splits` contiguous ranges of
 * ceil(N / splits) rows (the last ones may be short or empty); each keeps a k-entry list per query in work_dev
 * (splits * B * k floats), a second launch merges them.  splits = 0: the library chooses from B, N and the device's CU
 * count; n > 0: exactly n, at most MCM_KNN_MAX_SPLITS.  A tuning argument only: the outputs are a pure function of
 * feats_dev, bank_dev and k — the same bits for every `splits`, for every cut of the queries into calls and on every
 * run (no atomics, nothing summed across workgroups, no workgroup waits for another).
 * mcm_knn_workspace_bytes: *bytes_out = the work_dev size mcm_knn_score_features needs for the same (B, N, k, splits);
 * with splits = 0 it resolves the split count on the CURRENT device, as the score call does.
 * Timed under MCM_KC_SCORE (2 B N P flop).
 * Refusals (nothing is launched): MCM_EINVAL for a NULL h / feats_dev / bank_dev / work_dev / scores_dev / bytes_out,
 * B < 1, N < 1, k outside 1 .. MCM_KNN_MAX_K, splits < 0 or > MCM_KNN_MAX_SPLITS, work_bytes below
 * mcm_knn_workspace_bytes, proj_dim % 4 != 0, or feats_dev / bank_dev not 16-byte aligned (rows are read 16 bytes at a
 * time).  topv_dev may be NULL.  Stream contract: replayable. */
#define MCM_KNN_MAX_K 1024
#define MCM_KNN_MAX_SPLITS 32
int mcm_knn_workspace_bytes(const mcm_handle* h, int32_t B, int64_t N, int32_t k, int32_t splits, int64_t* bytes_out);
int mcm_knn_score_features(mcm_handle* h, const float* feats_dev /* [B, proj_dim] */, int32_t B,
                           const float* bank_dev /* [N, proj_dim] */, int64_t N, int32_t k, int32_t splits,
                           void* work_dev, int64_t work_bytes, float* scores_dev /* [B] */,
                           float* topv_dev /* [B, k] or NULL */, void* stream);

/* ---- negative-label score (--score neglabel; Jiang et al., ICLR 2024) --------------------------------
 * The share of a feature row's softmax mass that falls on the in-distribution (ID) prompts of a bank that also holds
 * mined negative prompts (added under ABI 5: two symbols only).  P = the handle's proj_dim, everything row-major:
 *   bank_dev [N, P]  rows [0, K) are the ID prompts, rows [K + g gs, K + (g + 1) gs) are negative group g of G;
 *                    N = K + G gs, which must fit int32;
 *   s[b, n]          = the fp32 dot product of feats_dev[b] and bank_dev[n] as mcm_knn_score_features defines it (the
 *                    exact-fp32 MFMA: one rounding per product, operands never narrowed);
 *   LI[b]            = logsumexp_n s[b, n] / T over the ID rows, LN[b, g] = the same over group g;
 *   S[b, g]          = 1 / (1 + exp(LN[b, g] - LI[b])): the ID mass against group g alone (finite for finite inputs);
 *   scores[b]        = -(1 / G) sum_g S[b, g], summed in fp64 over the fp32 values group_dev gets; larger = more OOD, the
 *                    sign every stored score here has;
 *   group_dev[b, g]  = S[b, g] (optional).
 * A NaN similarity anywhere in a row makes that row's score NaN (as a softmax would); other rows are unaffected.
 * The [B, N] similarities exist in registers and LDS only.  The bank is cut into `splits` contiguous ranges of
 * ceil(N / splits) rows (the last ones may be short or empty); each keeps one online-softmax pair (max, sum of
 * exp((s - max) / T); the sum carried in fp64, stored as fp32) per query and per row range (the ID rows, or one group)
 * it holds rows of in work_dev ([splits, B, G + 1] pairs of 8 bytes); a second launch combines them in split order in
 * fp64.  Only the slots the first launch wrote are read (which those are follows from K, gs and the split length), so
 * work_dev needs no initialisation.  splits = 0: the library chooses from B, N and the device's CU count; n > 0:
 * exactly n, at most MCM_KNN_MAX_SPLITS.  For fixed arguments (splits included) the outputs are the same bits on every
 * run, for every cut of the queries into calls and every row position (no atomics, no workgroup waits for another);
 * across `splits` the sums are associated differently and the results agree to rounding, not bit for bit.
 * mcm_neglabel_workspace_bytes: *bytes_out = the work_dev size the score call needs for the same (B, K, G, gs, splits);
 * with splits = 0 it resolves the split count on the CURRENT device, as the score call does.
 * Timed under MCM_KC_SCORE (2 B N P flop).
 * Refusals (nothing is launched): MCM_EINVAL for a NULL h / feats_dev / bank_dev / work_dev / scores_dev / bytes_out,
 * B, K, G or gs < 1, G > MCM_NEG_MAX_GROUPS, T <= 0 or not finite, splits < 0 or > MCM_KNN_MAX_SPLITS, work_bytes below
 * mcm_neglabel_workspace_bytes, proj_dim % 4 != 0, feats_dev / bank_dev not 16-byte aligned, or K + G gs above
 * INT32_MAX.  group_dev may be NULL.  Stream contract: replayable. */
#define MCM_NEG_MAX_GROUPS 1024
int mcm_neglabel_workspace_bytes(const mcm_handle* h, int32_t B, int32_t K, int32_t G, int32_t gs, int32_t splits,
                                 int64_t* bytes_out);
int mcm_neglabel_score_features(mcm_handle* h, const float* feats_dev /* [B, proj_dim] */, int32_t B,
                                const float* bank_dev /* [K + G gs, proj_dim] */, int32_t K, int32_t G, int32_t gs,
                                float T, int32_t splits, void* work_dev, int64_t work_bytes,
                                float* scores_dev /* [B] */, float* group_dev /* [B, G] or NULL */, void* stream);

/* ---- virtual-logit matching (--score vim; Wang et al., CVPR 2022) --------------------------------------
 * The third training-set score: the norm of a feature row's component outside the training features' principal
 * subspace, scaled to logit units, minus the energy of its zero-shot logits (added under ABI 5: two symbols only).
 * P = the handle's proj_dim, everything row-major:
 *   bank_dev [N, P]  rows [0, K) are the prompts, rows [K, K + R) the rows of the null-space basis NS (orthonormal, the
 *                    eigenvectors of the R smallest eigenvalues of the training features' uncentred second moment);
 *                    N = K + R, which must fit int32;
 *   s[b, n]          = the fp32 dot product of feats_dev[b] and bank_dev[n] as mcm_knn_score_features defines it (the
 *                    exact-fp32 MFMA: one rounding per product, operands never narrowed);
 *   resid[b]         = sqrt(sum_{j < R} ((double) s[b, K + j] - off_dev[j])^2); off_dev [R] fp64 is the projection of the
 *                    head's origin on NS (o . NS_j; NULL = 0, the zero-shot head: it has no bias);
 *   lse[b]           = logsumexp_{k < K} s[b, k] / T,   maxlogit[b] = max_{k < K} s[b, k] / T (NaN entries skipped);
 *   scores[b]        = (float) ((double) alpha resid[b] - lse[b]); larger = more OOD, the sign every stored score here has;
 *   parts_dev[b, :]  = resid[b], lse[b], maxlogit[b] rounded to fp32 (optional: what a fit needs to form alpha).
 * A NaN similarity anywhere in a row makes that row's score NaN; other rows are unaffected.
 * The [B, N] similarities exist in registers and LDS only.  The bank is cut into `splits` contiguous ranges of
 * ceil(N / splits) rows (the last ones may be short or empty); each keeps per query one 16-byte slot in work_dev
 * ([splits, B] slots): the online-softmax pair (max, sum of exp((s - max) / T); the sum carried in fp64, stored as fp32)
 * of its prompt rows and the fp64 sum of squares of its basis rows; a second launch combines them in split order in
 * fp64.  Only the slots the first launch wrote are read (which those are follows from K, R and the split length), so
 * work_dev needs no initialisation.  splits = 0: the library chooses from B, N and the device's CU count; n > 0:
 * exactly n, at most MCM_KNN_MAX_SPLITS.  For fixed arguments (splits included) the outputs are the same bits on every
 * run, for every cut of the queries into calls and every row position (no atomics, no workgroup waits for another);
 * across `splits` the sums are associated differently and the results agree to rounding, not bit for bit.
 * mcm_vim_workspace_bytes: *bytes_out = the work_dev size the score call needs for the same (B, K, R, splits); with
 * splits = 0 it resolves the split count on the CURRENT device, as the score call does.
 * Timed under MCM_KC_SCORE (2 B N P flop).
 * Refusals (nothing is launched): MCM_EINVAL for a NULL h / feats_dev / bank_dev / work_dev / scores_dev / bytes_out,
 * B, K or R < 1, K + R above INT32_MAX, T <= 0 or not finite, alpha not finite, splits < 0 or > MCM_KNN_MAX_SPLITS,
 * work_bytes below mcm_vim_workspace_bytes, proj_dim % 4 != 0, feats_dev / bank_dev not 16-byte aligned, or off_dev /
 * work_dev not 8-byte aligned.  off_dev and parts_dev may be NULL.  Stream contract: replayable. */
int mcm_vim_workspace_bytes(const mcm_handle* h, int32_t B, int32_t K, int32_t R, int32_t splits, int64_t* bytes_out);
int mcm_vim_score_features(mcm_handle* h, const float* feats_dev /* [B, proj_dim] */, int32_t B,
                           const float* bank_dev /* [K + R, proj_dim]: prompts, then basis rows */, int32_t K, int32_t R,
                           const double* off_dev /* [R] or NULL */, float T, float alpha, int32_t splits,
                           void* work_dev, int64_t work_bytes, float* scores_dev /* [B] */,
                           float* parts_dev /* [B, 3] = resid, lse, maxlogit as fp32, or NULL */, void* stream);

/* ---- GL-MCM: a patch-level local score next to MCM (--score GL-MCM; Miyai et al.) ---------------------
 * score = -(S_G + lambda S_L): S_G the MCM term of the global (CLS) feature, S_L the best concept match of any single
 * image patch (added under ABI 5: four symbols only).  The definition is taken from the paper (MaskCLIP's value path);
 * DESIGN.md 4.14.  P = the handle's proj_dim, R = patch tokens per image, everything row-major.
 *
 * The local score on features:
 *   s[b, i, k]      = the fp32 dot product of local_dev[b, i] and text_dev[k] as mcm_knn_score_features defines it (the
 *                     exact-fp32 MFMA: one rounding per product, operands never narrowed);
 *   patch[b, i]     = max_k softmax_k(s[b, i, :] / T) = 1 / sum_k exp((s[b, i, k] - max_k s[b, i, k]) / T), the sum carried
 *                     in fp64 across the bank's 256-row tiles as an online-softmax pair, the result rounded to fp32;
 *   local_scores[b] = -max_i patch[b, i]; larger = more OOD, the sign every stored score here has.
 * A NaN anywhere in an image's R x K similarities makes that image's score NaN, and patch NaN for the rows that hold it;
 * other images are unaffected.  The [B R, K] similarities exist in registers and LDS only.  Two launches: one over the
 * B R rows in tiles of 64 that writes the row values to work_dev (B R floats; and to patch_dev when given), one workgroup
 * per image for the maximum.  work_dev needs no initialisation.  The outputs are a pure function of (local_dev, text_dev, T):
 * the same bits on every run, for every cut of the images into calls and for every image position (no atomics, no
 * workgroup waits for another).  Timed under MCM_KC_SCORE (2 B R K P flop).
 * Refusals (nothing is launched): MCM_EINVAL for a NULL h / local_dev / text_dev / work_dev / local_scores_dev / bytes_out,
 * B, R or K < 1, B R above INT32_MAX, T <= 0 or not finite, proj_dim % 4 != 0, local_dev / text_dev not 16-byte aligned
 * (an output not 4-byte aligned), or work_bytes below mcm_local_workspace_bytes.  patch_dev may be NULL.
 * mcm_local_score_features — Stream contract: replayable. */
int mcm_local_workspace_bytes(const mcm_handle* h, int32_t B, int32_t R, int32_t K, int64_t* bytes_out);
int mcm_local_score_features(mcm_handle* h, const float* local_dev /* [B, R, proj_dim] */, int32_t B, int32_t R,
                             const float* text_dev /* [K, proj_dim] */, int32_t K, float T, void* work_dev,
                             int64_t work_bytes, float* local_scores_dev /* [B] = -S_L */,
                             float* patch_dev /* [B, R] or NULL */, void* stream);
/* The local features from the vision tower.  h_i = the fp32 residual-stream row of token i entering the LAST encoder layer:
 *   v_i = W_v layer_norm1(h_i) + b_v     the V block the unchanged forward leaves in its workspace
 *   o_i = W_o v_i + b_o                  the layer's out_proj: no attention mixing, no residual, no MLP
 *   y_i = W_proj post_layernorm(o_i)     l_i = y_i / |y_i|
 * for the R = (image_size / patch_size)^2 patch tokens i = 1 .. R of every image (token 0, CLS, is not a local row).  A
 * variant that re-attaches the residual and the MLP is not implemented.
 * mcm_encode_image_local runs the forward of mcm_encode_image_ex(normalize = 1) — the same launches, global_dev the same
 * bits — and behind it the local pass: out_proj and the projection as GEMMs over all B (R + 1) rows in the handle's operand
 * mode (single or split weights; visual_projection.weight in that form is built by mcm_finalize_weights), post_layernorm,
 * and one launch that L2-normalises and compacts the rows into local_dev.  Every intermediate lives in workspace the
 * forward is done with.  No entry other than the two below launches any of it.
 * mcm_score_glmcm: the same, the local rows kept in the handle's workspace; global_scores[b] = -S_G are the bits of
 * mcm_score (MCM_SCORE_MCM) for the same pixels, local_scores / patch the bits of mcm_local_score_features on
 * mcm_encode_image_local's rows, scores[b] = (float)((double) global_scores[b] + (double) lambda (double) local_scores[b]).
 * There is no split-activation (x2) form of either.
 * Refusals (nothing is launched): those of mcm_encode_image_ex; MCM_EINVAL for a NULL local_dev / text_dev / scores_dev, a
 * local_dev or text_dev not 16-byte aligned, K < 1, T <= 0 or not finite, lambda not finite, proj_dim % 16 != 0 or
 * proj_dim > v_width (the workspace the local pass borrows), a tower without patch tokens.
 * Both entries — Stream contract: replayable. */
int mcm_encode_image_local(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B,
                           float* global_dev /* [B, proj_dim], unit-norm */,
                           float* local_dev /* [B, R, proj_dim], unit-norm */, void* stream);
int mcm_score_glmcm(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t B, const float* text_dev /* [K, proj_dim] */,
                    int32_t K, float T, float lambda, float* scores_dev /* [B] */,
                    float* global_scores_dev /* [B] or NULL: -S_G */, float* local_scores_dev /* [B] or NULL: -S_L */,
                    float* patch_dev /* [B, R] or NULL */, void* stream);

/* ---- CLIP byte-level BPE tokenizer, host side --------------------------------
 * Replaces CLIPTokenizer.from_pretrained(args.ckpt) + tokenizer(list[str], padding=True,
 * return_tensors="pt") of reference utils/detection_util.py:216,228.  vocab.json / merges.txt are the
 * checkpoint's tokenizer files.  Pure host code: usable without a GPU. */
typedef struct mcm_tokenizer mcm_tokenizer;
int mcm_tokenizer_create(const char* vocab_json_path, const char* merges_txt_path, mcm_tokenizer** out);
void mcm_tokenizer_destroy(mcm_tokenizer* t);
const char* mcm_tokenizer_last_error(const mcm_tokenizer* t); /* t == NULL: the last create error */
int32_t mcm_tokenizer_vocab_size(const mcm_tokenizer* t);
/* n prompts (UTF-8, NUL-terminated) -> ids_out / mask_out [n, *seq_len_out] int32, row-major,
 * *seq_len_out = longest prompt incl. BOS/EOS; shorter rows are padded with the pad token
 * (<|endoftext|>) and mask 0.  capacity = row capacity of the output buffers (e.g. 77);
 * MCM_ERANGE (with *seq_len_out set) when the longest prompt needs more. mask_out may be NULL. */
int mcm_tokenizer_encode(mcm_tokenizer* t, const char* const* texts, int32_t n, int32_t capacity,
                         int32_t* ids_out, int32_t* mask_out, int32_t* seq_len_out);

/* ---- per-kernel timing (HIP events on the caller's stream) -------------------------
 * When enabled, every kernel launch of the encode path is bracketed by a pair of
 * pre-created hipEvents.  mcm_profile_read synchronises the stream, accumulates the
 * elapsed times per kernel class and returns them; it resets the accumulators.
 * Classes: see MCM_KC_*. */
#define MCM_KC_PATCHIFY 0
#define MCM_KC_GEMM 1
#define MCM_KC_LAYERNORM 2
#define MCM_KC_ATTENTION 3
#define MCM_KC_POOL_PROJECT 4
#define MCM_KC_SCORE 5
#define MCM_KC_EMBED 6
/* sub-classes of MCM_KC_GEMM (ABI 3): the whole-batch GEMM shapes of an encoder layer, counted in MCM_KC_GEMM as well */
#define MCM_KC_GEMM_QKV 7
#define MCM_KC_GEMM_OUTPROJ 8
#define MCM_KC_GEMM_FC1 9
#define MCM_KC_GEMM_FC2 10
#define MCM_KC_COUNT 11
int mcm_profile_enable(mcm_handle* h, int32_t on);
/* ms_out[MCM_KC_COUNT], launches_out[MCM_KC_COUNT], flops_out[MCM_KC_COUNT] (algorithmic
 * FLOP issued by that class since the last read; GEMM counts 2*M*N*K of the *logical*
 * problem, not the padded tile grid). */
int mcm_profile_read(mcm_handle* h, double* ms_out, int64_t* launches_out, double* flops_out);

/* ---- operator-level entry points (same kernels the towers launch; used by the parity
 * tests to pin each kernel against the oracle, and usable as building blocks) --------
 * All tensors row-major.  `prec` = MCM_PREC_*: in BF16 mode activations/weights that
 * feed MFMA are bf16 (uint16 storage), in F32 mode they are fp32. */

/* y[M,N] = x[M,K] · w[N,K]^T + bias[N]  with epilogue `epi`:
 *   0: store (+bias)                out dtype = operand dtype
 *   1: QuickGELU(acc+bias)          out dtype = operand dtype   (activations.py:117-123)
 *   2: resid[M,N] (fp32) += acc+bias   in place; `y` ignored
 * M ≥ 1 arbitrary (ragged tiles are clamped/masked); K % 64 == 0 (bf16) or K % 32 == 0
 * (fp32): one K-step is 128 bytes per row; N % 16 == 0.  Stream contract: replayable. */
int mcm_op_linear(mcm_handle* h, int32_t prec, const void* x_dev, const void* w_dev,
                  const float* bias_dev, void* y_dev, float* resid_dev, int32_t M, int32_t N,
                  int32_t K, int32_t epi, void* stream);
/* mcm_op_linear with flags: bit 0 = w_dev is the split image [N, 2K] written by mcm_op_split_weight (16-bit modes;
 * K % 64 == 0): y = x (W_hi + W_lo)^T, both products in one fp32 accumulator chain. */
#define MCM_LINEAR_SPLIT_W 1
/* bit 1 (fp16 mode, K % 64 == 0): x_dev is the SPLIT image [M, 2K] of a logical [M, K] activation — per 64 columns
 * hi[64] = round(x) then lo[64] = round(x - hi), the layout mcm_op_split_weight writes for M rows — y = (X_hi + X_lo) W^T;
 * bit 2 (fp16 mode, epilogues 0 / 1, N % 64 == 0): y_dev is written as a split image [M, 2N] (QuickGELU in its exact form).
 * Together they are the GEMMs of the split-activation arm (mcm_score_x2). */
#define MCM_LINEAR_SPLIT_X 2
#define MCM_LINEAR_SPLIT_OUT 4
/* bit 3 (ABI 5; epilogue 1 only, every mode): the activation is the exact erf GELU (MCM_ACT_GELU) instead of QuickGELU — the
 * fc1 epilogue of a tower whose hidden_act is "gelu".  Combines with the three bits above exactly as epilogue 1 does.
 * mcm_op_linear_ex — Stream contract: replayable. */
#define MCM_LINEAR_ACT_GELU 8
int mcm_op_linear_ex(mcm_handle* h, int32_t prec, const void* x_dev, const void* w_dev,
                     const float* bias_dev, void* y_dev, float* resid_dev, int32_t M, int32_t N,
                     int32_t K, int32_t epi, int32_t flags, void* stream);
/* fp32 w [N,K] (device) → split operand image [N, 2K] in the 16-bit dtype of `prec` (K % 64 == 0).
 * Stream contract: replayable. */
int mcm_op_split_weight(mcm_handle* h, int32_t prec, const float* w_dev, int32_t N, int32_t K,
                        void* out_dev, void* stream);
/* LayerNorm over the last dim (modeling_clip.py:370,379,605,608): x fp32 [M,D] →
 * y (operand dtype of `prec`, or fp32 when out_f32 != 0) [M,D].  Stream contract: replayable. */
int mcm_op_layernorm(mcm_handle* h, int32_t prec, const float* x_dev, const float* gamma_dev,
                     const float* beta_dev, void* y_dev, int32_t M, int32_t D, float eps,
                     int32_t out_f32, void* stream);
/* The split-activation arm's LayerNorm and attention (fp16): y [M, 2D] / out [rows, 2 heads 64] are split images (per 64
 * columns hi[64] then lo[64]); mcm_op_attention_split reads qkv as a split image [rows, 6 heads 64].  head_dim 64; the
 * model's vision tower also runs head_dim 80 (ViT-H/14), which the operator level reaches through the harness library's
 * mcm_debug_op_attention_split_hd.  Both entries — Stream contract: replayable. */
int mcm_op_layernorm_split(mcm_handle* h, const float* x_dev, const float* gamma_dev, const float* beta_dev,
                           void* y_dev, int32_t M, int32_t D, float eps, void* stream);
int mcm_op_attention_split(mcm_handle* h, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                           int32_t heads, void* stream);
/* Multi-head SDPA (modeling_clip.py:259-277,313-331): qkv [nseq*seq_len, 3*heads*64]
 * packed as [q | k | v], head_dim 64, scale 0.125; causal != 0 for the text tower.  (This entry point means head_dim 64;
 * the model's vision tower also runs head_dim 80, scale 80^-0.5 — ViT-H/14, a streaming family of its own at every length —
 * which the operator level reaches through the harness library's mcm_debug_op_attention_hd.)
 * out [nseq*seq_len, heads*64].  Two routes, chosen by length:
 *   seq_len ≤ 288 (18 key tiles of 16): K and V of a head held whole in LDS (the B/32, B/16 and L/14 towers, causal text);
 *   seq_len 289 ... 1025, bidirectional only: K and V streamed through LDS in 64-key tiles with an online softmax (every mode,
 *   mcm_op_attention_split too; ViT-L/14@336px: 577 tokens).
 * A bidirectional seq_len above 1025 (the vision-token ceiling of mcm_create) is refused; causal attention (the text tower's
 * 77 tokens) has the first route only.  Stream contract: replayable. */
int mcm_op_attention(mcm_handle* h, int32_t prec, const void* qkv_dev, void* out_dev,
                     int32_t nseq, int32_t seq_len, int32_t heads, int32_t causal,
                     void* stream);

/* fp16 saturation watch.  In MCM_PREC_F16 every 16-bit activation write saturates at +-65504 instead of
 * overflowing to inf (MODE.FP16_OVFL) — which keeps a row finite but costs that element's precision.  So that
 * this never happens unnoticed (a real checkpoint has outlier channels the seeded weights do not), the GEMM
 * epilogues and the LayerNorm that write fp16 activations track the largest magnitude they packed and bump a
 * sticky per-handle device counter once per wave that packed a saturating value (|v| >= 65520).
 * mcm_saturation_count: *count_host = events since the last reset (0 = no activation of any call left the fp16
 * range); synchronises `stream`; reset != 0 clears the counter.  mcm_saturation_check(h, 0) stops the kernels
 * from reporting (the tracking itself is a handful of VALU instructions per tile and is always compiled in).
 * Always 0 in MCM_PREC_BF16 / MCM_PREC_F32 (fp32 exponent range).
 * mcm_saturation_count — Stream contract: synchronising. */
int mcm_saturation_check(mcm_handle* h, int32_t on);
int mcm_saturation_count(mcm_handle* h, int32_t reset, uint64_t* count_host, void* stream);

/* Kernel faults (ABI 4).  The persistent attention kernel (one workgroup per CU: loader waves and compute waves that wait for each
 * other through LDS counters) bounds every wait: a wave that has polled 2^22 times (three orders of magnitude above the kernel's
 * whole run time) stops its workgroup and stores 1 to a sticky per-handle word in host-mapped memory, so that a protocol slip ends
 * the launch with wrong rows instead of holding the GPU until a watchdog fires.  From then on every compute call on the handle
 * returns MCM_EHIP (mcm_last_error says why): the handle must be destroyed.  mcm_kernel_faults reads the word without
 * synchronising (non-zero = faulted; for a definitive answer synchronise the stream first); 0 in every correct run. */
int mcm_kernel_faults(const mcm_handle* h);

#ifdef MCM_HARNESS
/* libmcm_hip_harness.so only (built with -DMCM_HARNESS next to the shipped library; loaded by the A/B tests
 * and tools, never by the product path).  Process-wide switches.
 * GEMM variant: -1 the shipped size policy (64x128 / 128x128 tile kernels, persistent 256x256, ping-pong),
 * 0 = the 128x128 tile kernel always, 11 = the 64x128 tile kernel always, 3/4 = persistent 256x256 2-stage (4: counted
 * epilogue stores), 5 = persistent 256x256 ping-pong (problems whose M and N are multiples of 256; others run as 3),
 * 9 = the flagged ping-pong text of gemm_arms.hpp with every flag off (honours mcm_debug_gemm_group_n; whole tiles, others as 5).
 * Removed in round 6 after measuring negative (EXPERIMENTS.md "Removed arms"): 1/2 persistent 256x128 3-stage, 6 the ping-pong
 * loop on 32x32x16 MFMAs, 7 balanced DMA, 8 staggered epilogues.  Returns MCM_OK, or MCM_EINVAL for an unknown variant. */
int mcm_debug_gemm_variant(int32_t variant);
/* The MLP activations exactly as the GEMM epilogues compute them, element-wise: y[i] = act(x[i]) for n fp32 values on the device.
 * act: 0 = QuickGELU with the IEEE division (fp32 arm, split outputs), 1 = its v_exp / v_rcp form (16-bit outputs), 2 = the erf
 * GELU (every mode).  Asynchronous on `stream`. */
int mcm_debug_op_act(mcm_handle* h, int32_t act, const float* x_dev, float* y_dev, int64_t n, void* stream);
/* 16-bit attention kernel: 1 = the shipped policy (the transpose-read kernel; its persistent form at the B/16 shape from 16 jobs
 * per CU on), 0 = the round-1 kernel, 10 = XCD-aware deal of the (sequence, head) workgroups, 11 = the q-blocks dealt to the waves
 * rotated per workgroup (SIMD balance; bit-identical, no gain), 21 = the persistent form at every size and query count of the
 * 13-tile shape, 36 = the 8-wave kernel at every size.  Anything else: MCM_EINVAL (the arms 2 - 9, 12 - 20, 22 - 35 of rounds
 * 2 - 5 were removed in round 6: EXPERIMENTS.md "Removed arms"). */
int mcm_debug_attention_variant(int32_t variant);
/* Polls a wait of the persistent attention kernel may take before it gives up (the shipped library always passes 2^22);
 * 0 = every wait that has to wait gives up at once.  mcm_debug_clear_faults resets the handle's sticky fault word.  Both exist
 * for the test of the fault path only. */
int mcm_debug_attn_spin_budget(int64_t polls);
int mcm_debug_clear_faults(mcm_handle* h);
/* mcm_op_attention with the two launch parameters only the model sets: query rows (0 = all; the CLS-only last layer passes 1)
 * and the walk direction (reverse != 0: jobs in descending order). */
int mcm_debug_op_attention(mcm_handle* h, int32_t prec, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                           int32_t heads, int32_t causal, int32_t qrows, int32_t reverse, void* stream);
/* mcm_op_attention_split with the same two launch parameters: query rows (0 = all; 1 = the CLS-only last layer) and the walk
 * direction. */
int mcm_debug_op_attention_split(mcm_handle* h, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                                 int32_t heads, int32_t qrows, int32_t reverse, void* stream);
/* The two above with the head width as an argument.  head_dim 64: their routes.  head_dim 80: the streaming family of
 * ViT-H/14's vision tower — qkv [rows, 3 heads 80], head h at column 80 h of q, k and v, scale 80^-0.5, bidirectional only
 * (causal != 0 is refused), seq_len <= 1025; the split form's images are "per 64 columns hi[64] then lo[64]" over the whole
 * heads x 80 row (column c at (c / 64) 128 + c % 64, lo 64 further): a head straddles blocks.  Any other head_dim is refused.
 * A refused call launches nothing. */
int mcm_debug_op_attention_hd(mcm_handle* h, int32_t prec, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                              int32_t heads, int32_t head_dim, int32_t causal, int32_t qrows, int32_t reverse, void* stream);
int mcm_debug_op_attention_split_hd(mcm_handle* h, const void* qkv_dev, void* out_dev, int32_t nseq, int32_t seq_len,
                                    int32_t heads, int32_t head_dim, int32_t qrows, int32_t reverse, void* stream);
/* The front of the vision tower as mcm_encode_image* run it (the same function, the handle's own weights and workspace), stopped
 * at `stage`: 0 = behind the patch-embedding GEMM, 1 = behind the fused CLS row + pre_layrnorm + layer 0 layer_norm1 pass.  The
 * fp32 residual rows [B * tokens, v_width] are copied to resid_out_dev (at stage 0 the CLS rows are whatever the workspace held);
 * at stage 1 the first QKV operand rows are copied to ln_out_dev: [B * tokens, v_width] in the operand dtype, or the split image
 * [B * tokens, 2 v_width] fp16 with x2.  pixel_format: MCM_PIXELS_*; x2: the split-activation arm.  poison != 0: the patch
 * matrix and the residual rows are filled with 0xFF bytes first (NaN in every operand format).  The route (pixel-gathering GEMM
 * or patchify + GEMM) is the product's own choice, mcm_debug_patch_fold included. */
int mcm_debug_vision_front(mcm_handle* h, const void* pixels_dev, int32_t pixel_format, int32_t x2, int32_t B, int32_t stage,
                           int32_t poison, float* resid_out_dev, void* ln_out_dev, void* stream);
/* The pooling kernel of both towers on the caller's buffers: row i of out [n, P] = normalise?(LayerNorm(x[row]) proj^T) with
 * row = row_idx_host[i], or i * row_stride when row_idx_host is NULL; x [x_rows, D] fp32, proj [P, D] fp32.  The indices are
 * host memory and are checked against x_rows.  MCM_EINVAL for D > 1280, D % 4 != 0 (past 1024: D % 64 != 0), P > 1024 or a row outside x.
 * Synchronises the stream. */
int mcm_debug_op_pool_project(mcm_handle* h, const float* x_dev, int64_t x_rows, const int32_t* row_idx_host, int32_t row_stride,
                              int32_t n, int32_t D, const float* gamma_dev, const float* beta_dev, float eps,
                              const float* proj_dev, int32_t P, float* out_dev, int32_t normalize, void* stream);
/* The text embedding kernel on the caller's buffers: x [K * S, D] = tok[ids[k * S + s]] + pos[s]; tok [vocab, D], pos with at
 * least S rows.  The ids are host memory and are checked against vocab.  MCM_EINVAL for D % 4 != 0 or an id outside the table.
 * Synchronises the stream. */
int mcm_debug_op_text_embed(mcm_handle* h, const int32_t* ids_host, int32_t vocab, const float* tok_dev, const float* pos_dev,
                            float* x_dev, int32_t K, int32_t S, int32_t D, void* stream);
/* The context form of the text embedding kernel on the caller's buffers: x [K * S, D] = (slot < 0 ? tok[ids[k * S + s]] :
 * ctx[set, slot]) + pos[s]; ctx [n_sets, n_ctx, D] fp32 on the device, n_sets 1 (set 0 for every k) or K (set k).  Ids and slots are
 * host memory and are checked.  MCM_EINVAL for D % 4 != 0, an id outside the table, a slot outside -1 ... n_ctx - 1, n_sets other
 * than 1 or K, or a ctx_dev that is not 16-byte aligned.  Synchronises the stream. */
int mcm_debug_op_text_embed_ctx(mcm_handle* h, const int32_t* ids_host, const int32_t* slot_host, int32_t vocab,
                                const float* tok_dev, const float* pos_dev, const float* ctx_dev, int32_t n_ctx, int32_t n_sets,
                                float* x_dev, int32_t K, int32_t S, int32_t D, void* stream);
/* A/B and ablation bits of the GEMM kernels (gemm.hip, GemmArgs::dbg; 0 = shipped behaviour). */
int mcm_debug_gemm_dbg(int32_t bits);
/* A/B: run the QKV projection + attention of every layer per chunk of the batch (n chunks; 1 = shipped). */
int mcm_debug_qkv_chunks(int32_t n);
/* A/B: the wide store GEMMs (QKV projection, fc1) as n launches over column blocks of N / n (1 = shipped: one launch).
 * The W re-fetch experiment of DESIGN.md / EXPERIMENTS.md: only N / n of W is live in an XCD's L2 per launch. */
int mcm_debug_nsplit(int32_t n);
/* A/B: the persistent kernels walk their N tiles in groups of gn (0 = plain n-fastest walk, the shipped behaviour): only gn
 * N-tiles of W are live in an XCD's L2 at a time.  Honoured by gemm_p256_kernel and by the arms text of the ping-pong kernel
 * (variant 9); the shipped ping-pong kernel walks plainly. */
int mcm_debug_gemm_group_n(int32_t gn);
/* A/B: 1 (default, shipped) = the patch-embedding GEMM gathers its A operand from the fp32 NCHW pixels itself; 0 = the
 * rounds 1 - 3 route (patchify writes a patch matrix, the GEMM reads it back).  Bit-identical. */
int mcm_debug_patch_fold(int32_t on);
/* 0 (shipped): mcm_resize_crop_u8 stages the source window in LDS where it fits; 1: the per-pixel fused form of
   rounds 2 - 3 for every workgroup (A/B). */
int mcm_debug_resize_fused_only(int32_t on);
/* 0 (shipped): the persistent GEMM kernels launch one workgroup per CU; n (a multiple of 8): n workgroups, so that two
   handles on two streams can share the chip (tools/dual_stream_probe.py, removed in round 6: git history). */
int mcm_debug_persistent_grid(int32_t n);
/* A/B: 1 = the LayerNorms of the vision tower between a residual GEMM and its consumer folded into the two GEMM
 * epilogues (16-bit modes, widths that are multiples of 256; bit-identical for every batch size); 0 (default, the
 * shipped behaviour) = every LayerNorm as its own launch.  Measured 1 % slower end to end, DESIGN.md 5.5. */
int mcm_debug_ln_fold(int32_t on);
/* A/B: 1 = the 16-bit towers hand q / k / v from the QKV projection to attention head-major ([3 heads][rows][64]: an
 * attention workgroup's rows are consecutive bytes); 0 (default, shipped) = [rows][3 D].  Bit-identical; no net gain. */
int mcm_debug_qkv_head_major(int32_t on);
/* A/B: 1 = the LayerNorm behind a whole-batch out-proj / fc2 of a 16-bit vision tower is computed in the tail of that
 * GEMM's kernel by the waves that have run out of tiles (same bits as the LayerNorm launch); 0 (default, shipped) =
 * every LayerNorm is its own launch.  Measured equal at ViT-B/16 batch 512, slower on smaller problems, DESIGN.md 5.5. */
int mcm_debug_ln_tail(int32_t on);
/* A/B (round 6): 1 = the LayerNorm behind a whole-batch out-proj / fc2 of a 16-bit vision tower is written by that GEMM's own
 * EPILOGUE from the accumulator registers: the N / 256 workgroups that hold the tiles of one 256-row panel act as one
 * full-row tile — row moments exchanged through an XCD's L2, no re-read of the residual stream, no LayerNorm launch
 * (gemm_arms.hpp "LNC"; the full-row epilogue of VERDICT r5 item 2).  Scores agree with the shipped path to fp32 round-off
 * (Chan-combined slot moments instead of whole-row two-pass statistics), not bit for bit.  0 (default) = shipped behaviour.
 * Waits that gave up are counted by mcm_debug_ln_tail_timeouts. */
int mcm_debug_ln_cluster(int32_t on);
/* LNC, second form (R6.4): polls < 0 (default) = a wave WAITS for its row panel's partner workgroups (the first form); polls >= 0 =
 * the DEFER form: after that many polls of the partners' counter a wave leaves its 128 x 64 segment's LayerNorm to a clean-up
 * launch behind the GEMM (one mask word per panel half says which segments are owed; same arithmetic, same bits) and goes on
 * to its next tile.  mcm_debug_ln_cluster_deferred: segments normalised by the clean-up launches since mcm_create. */
int mcm_debug_ln_cluster_spin(int32_t polls);
/* A/B (round 6, R6.7): 1 = out-proj / fc2 of a whole-batch 16-bit vision layer run as 64-row FULL-ROW tiles (one workgroup holds
 * 64 x 768 / 1024 outputs) whose epilogue writes x once and the LayerNorm output from the accumulator registers — the literal
 * design of VERDICT r5 item 2, no cross-workgroup traffic (gemm_arms.hpp ROW64).  Round-off-equal to the shipped path.
 * 2 = three W stages per wave (N = 768); 3 / 4 = as 1 / 2 on a piece-contiguous copy of the weight, built on first use. */
int mcm_debug_ln_row(int32_t on);
int mcm_debug_ln_cluster_deferred(mcm_handle* h, uint64_t* count_host);
/* Tickets of the LayerNorm tail that gave up waiting for their rows (a bounded spin: wrong rows rather than a hung
 * device); 0 in a correct run.  Synchronises the device. */
int mcm_debug_ln_tail_timeouts(mcm_handle* h, uint64_t* count_host);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MCM_H_ */
