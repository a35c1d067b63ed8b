/* mcm_score_stream.h — an extension of the C ABI of include/mcm.h: the streamed tail of the MCM family.  Two symbols of
 * libmcm_hip.so (and of the harness library) on the terms every symbol added under MCM_ABI_VERSION 5 has: no struct,
 * constant or existing entry changes, a caller built against mcm.h alone runs unchanged.  They are declared here, not in
 * mcm.h, because the symbol set of mcm.h is what tests/golden/abi_prototypes.json froze when the Python binding became
 * derived from it; mcm_amd/abi.py reads this header with the same rules and keeps its entries in a table of their own. */
#ifndef MCM_SCORE_STREAM_H
#define MCM_SCORE_STREAM_H

#include "mcm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the MCM family against a prompt bank of any size ------------------------------------------------
 * mcm_score_features keeps one image's K similarities in LDS and so refuses (proj_dim + K) * 4 > 150 KiB; this entry walks
 * the bank as the bank-streamed scores do and has no such limit.  P = the handle's proj_dim, everything row-major:
 *   s[b, k]        = the fp32 dot product of img_feat_dev[b] and text_feat_dev[k] as mcm_knn_score_features defines it (the
 *                    exact-fp32 MFMA: one rounding per product, operands never narrowed);
 *   Td             = (double) T;  m[b] = max_k s[b, k] (NaN entries skipped);  x[b, k] = (s[b, k] - m[b]) / Td;
 *   Z = sum_k exp(x),   W = sum_k x exp(x),   Q = sum_k exp(2 x)      (fp64);
 *   MCM_SCORE_MCM        -1 / Z                                     (the largest softmax probability, negated)
 *   MCM_SCORE_MAX_LOGIT  -m                                         (the bits of the largest similarity, negated)
 *   MCM_SCORE_ENERGY     -Td (m / Td + log Z)
 *   MCM_SCORE_ENTROPY    log Z - W / Z
 *   MCM_SCORE_VAR        -(Q / Z^2 - 1 / K) / K                     (the softmax's mean is exactly 1 / K)
 *   scores_dev[b]  = the requested `kind`, rounded once to fp32; larger = more OOD, the sign every stored score here has;
 *   parts_dev[b, 0..4] (optional) = all five kinds in MCM_SCORE_* order; scores_dev[b] is the bits of parts_dev[b, kind];
 *   idx_dev [B, topk], prob_dev [B, topk] (topk > 0; prob_dev optional) = the bank rows of the topk largest similarities in
 *                    mcm_score_features_topk's order (value descending, then row ascending; +0 == -0; a NaN is never a
 *                    candidate) and (float) (exp((s - m) / Td) / Z); slots without a candidate hold -1 / NaN.  For MCM on
 *                    a NaN-free row prob_dev[b, 0] == -scores_dev[b] bit for bit.
 * A NaN similarity anywhere in a row makes that row's five scores and its probabilities NaN; other rows are unaffected.
 * The [B, K] similarities exist in registers and LDS only.  The bank is cut into `splits` contiguous ranges of
 * ceil(K / splits) rows (the last ones may be short or empty); each keeps per query one 32-byte slot {Z, W, Q as fp64, m as
 * fp32, 4 bytes unused} over its rows at its own maximum, and topk 8-byte list entries {fp32 similarity, int32 row}, in
 * work_dev: [splits, B] slots, then [splits, B, topk] entries.  A second launch combines them in split order in fp64: with
 * d = (m_s - m) / Td and a = exp(d) a split enters as a Z_s, a (W_s + d Z_s), a^2 Q_s.  Only the slots and lists the first
 * launch wrote are read (which those are follows from K and the split length), so work_dev needs no initialisation.
 * splits = 0: the library chooses from B, K and the device's CU count; n > 0: exactly n, at most MCM_KNN_MAX_SPLITS.  For
 * fixed arguments (splits included) the outputs are the same bits on every run, for every cut of the queries into calls and
 * every row position (no atomics, no workgroup waits for another); across `splits` the sums are associated differently
 * and the results agree to rounding, not bit for bit (max-logit and idx_dev do not depend on it).
 * mcm_score_stream_workspace_bytes: *bytes_out = the work_dev size the score call needs for the same (B, K, topk, splits);
 * with splits = 0 it resolves the split count on the CURRENT device, as the score call does.
 * Timed under MCM_KC_SCORE (2 B K P flop).
 * Refusals (nothing is launched): MCM_EINVAL for a NULL h / img_feat_dev / text_feat_dev / work_dev / scores_dev / bytes_out,
 * B or K < 1, K above INT32_MAX (rows are numbered in int32), T <= 0 or not finite, kind outside MCM_SCORE_MCM ..
 * MCM_SCORE_VAR, topk outside 0 .. MCM_TOPK_MAX, a NULL idx_dev with topk > 0, splits < 0 or > MCM_KNN_MAX_SPLITS, work_bytes
 * below mcm_score_stream_workspace_bytes, proj_dim % 4 != 0, img_feat_dev / text_feat_dev not 16-byte aligned, or work_dev
 * not 8-byte aligned.  parts_dev and prob_dev may be NULL; idx_dev and prob_dev are not touched with topk = 0.
 * From pixels: mcm_encode_image_ex(normalize = 1) (or mcm_encode_image_x2) into a buffer of the caller's, then this call.
 * mcm_score_features_stream — Stream contract: replayable (the classes: include/mcm.h, "Stream contract"). */
int mcm_score_stream_workspace_bytes(const mcm_handle* h, int32_t B, int64_t K, int32_t topk, int32_t splits,
                                     int64_t* bytes_out);
int mcm_score_features_stream(mcm_handle* h, const float* img_feat_dev /* [B, proj_dim] */, int32_t B,
                              const float* text_feat_dev /* [K, proj_dim] */, int64_t K, float T, int32_t kind,
                              int32_t topk, int32_t splits, void* work_dev, int64_t work_bytes,
                              float* scores_dev /* [B] */, float* parts_dev /* [B, 5] or NULL */,
                              int32_t* idx_dev /* [B, topk] */, float* prob_dev /* [B, topk] or NULL */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCM_SCORE_STREAM_H */
