"""The stream contract of the C ABI, one row per exported entry that takes a `stream` (include/mcm.h outside #ifdef MCM_HARNESS,
include/mcm_score_stream.h).  A plain module: no GPU, no library, standard library and mcm_amd.abi only.

The three classes (the "Stream contract" block of include/mcm.h says the same in the header's words):

    replayable     asynchronous on `stream`, no allocation, no host synchronisation, and no host array read at call time that a
                   replay would need refreshed.  May sit inside a captured hipGraph after one warm-up call with the same arguments
                   outside the capture (the first launch of a kernel with dynamic LDS raises its limit: common.hpp launch_lds).
                   Scalars and pointers are baked into the graph.
    host_staged    correct on any stream, not capturable: it reads host arrays at call time, or waits on a ring event, or drains
                   `stream` before it rewrites a pinned staging buffer, or may allocate on a first or growing call.
    synchronising  returns host results and drains `stream`.

Every class was read off the code, row by row; the line cited is the one that decides it (mcm_amd/csrc/mcm_api.hip unless another file
is named).  tests/test_stream_contract_cpu.py holds the keys to the headers; tests/test_gpu_stream_contract.py holds every
`replayable` row to "a replay gives the eager call's bits", and the `host_staged` rows to eager stream order.

What makes a row `replayable` is the same few facts each time, named once here:
    [s]     every launch of the entry goes to the caller's stream: each launcher passes its `hipStream_t s` to hipLaunchKernelGGL /
            launch_lds (common.hpp:30), and no launcher calls a hipMemset*, hipMemcpy*, hipMalloc*, hipFree* or a synchronise
    [zero]  what has to be zero is zeroed by launch_zero_spans (a kernel on `s`, embed.hip), not by hipMemsetAsync
    [ws]    every intermediate lives in the workspace mcm_create allocated, or in work_dev / scratch of the caller's
"""
import os
import re

from mcm_amd import abi

REPLAYABLE, HOST_STAGED, SYNCHRONISING = "replayable", "host_staged", "synchronising"
CLASSES = (REPLAYABLE, HOST_STAGED, SYNCHRONISING)
HEADERS = ("mcm.h", "mcm_score_stream.h")

_IMAGE = ("encode_image_impl :795 — vision_front :719 (patchify / patch GEMM, pad rows by launch_zero_spans :766 [zero], "
          "launch_layernorm_pre), run_layers :311, launch_pool_project :806: [s] [ws]")
_TEXT = ("encode_text_passes :1350 — hipStreamSynchronize(s) before every pass, the first included (:1358), then the host ids are "
         "staged through the handle's one pinned buffer (ids_pin / rowidx_pin :1364-1372)")
_BANK = "one partial launch over (query tiles, splits) and one combine launch, both on s; partials in the caller's work_dev: [s] [ws]"

CONTRACT = {
    # ---- the text tower: host ids, staged per pass
    "mcm_encode_text": (HOST_STAGED, "forwards to mcm_encode_text_ex :1341; " + _TEXT),
    "mcm_encode_text_ex": (HOST_STAGED, "validates ids_host on the host :1407, then " + _TEXT),
    "mcm_encode_text_ctx": (HOST_STAGED, "validates ids_host / slot_host on the host :1423, then " + _TEXT
                            + "; ctx_dev itself is read on s by launch_text_embed_ctx :1376"),
    # ---- the vision tower, every format and arm
    "mcm_encode_image": (REPLAYABLE, _IMAGE),
    "mcm_encode_image_raw": (REPLAYABLE, "normalize = false :822; " + _IMAGE),
    "mcm_encode_image_ex": (REPLAYABLE, "pixel_format checked on the host :827; " + _IMAGE),
    "mcm_encode_image_u8": (REPLAYABLE, "u8 = true :1142 (launch_patchify_u8 on s); " + _IMAGE),
    "mcm_encode_image_x2": (REPLAYABLE, "x2 = true :839 (the split rows live in the same workspace); " + _IMAGE),
    "mcm_encode_image_local": (REPLAYABLE, "encode_image_local_impl :1074 — the forward above, then local_pass :1047: two "
                               "launch_zero_spans (:1052, :1062 [zero]), two GEMMs, a LayerNorm and launch_local_compact on s [ws]; " + _IMAGE),
    # ---- scores on features
    "mcm_score_features": (REPLAYABLE, "one launch_score on s :1438 (score.hip:376, launch_lds): [s]"),
    "mcm_score_features_topk": (REPLAYABLE, "one launch_score_topk on s :1472 (score.hip:388, launch_lds): [s]"),
    "mcm_score_features_stream": (REPLAYABLE, "launch_score_stream :1016 (score_stream.hip:278) — " + _BANK),
    "mcm_knn_score_features": (REPLAYABLE, "launch_knn :923 (knn.hip:178) — " + _BANK),
    "mcm_neglabel_score_features": (REPLAYABLE, "launch_neglabel :949 (neglabel.hip:147, :160) — " + _BANK),
    "mcm_vim_score_features": (REPLAYABLE, "launch_vim :981 (vim.hip:158, :171) — " + _BANK),
    "mcm_local_score_features": (REPLAYABLE, "launch_local_score :1107 (glmcm.hip:152 rows, :154 per image), row values in the "
                                 "caller's work_dev: [s] [ws]"),
    # ---- one batch of the hot loop
    "mcm_score": (REPLAYABLE, "mcm_encode_image into h->feat, then mcm_score_features :1444-1446; " + _IMAGE),
    "mcm_score_u8": (REPLAYABLE, "the u8 encode into h->feat, then mcm_score_features :1147-1149; " + _IMAGE),
    "mcm_score_x2": (REPLAYABLE, "mcm_encode_image_x2 into h->feat, then mcm_score_features :844-846; " + _IMAGE),
    "mcm_score_topk": (REPLAYABLE, "every refusal first (check_topk_call :1482), the encode into h->feat :1484, then "
                       "mcm_score_features_topk :1486; " + _IMAGE),
    "mcm_score_glmcm": (REPLAYABLE, "encode_image_local_impl with the local rows in h->x :1127, mcm_score_features :1132, "
                        "mcm_local_score_features with h->att as its work :1133, launch_local_combine :1136 (glmcm.hip:132): [s] [ws]"),
    # ---- ingest: host arrays, staging rings
    "mcm_resize_crop_u8": (HOST_STAGED, "src_dev_ptrs / heights / widths are host arrays read at call time :1193-1202; waits on the ring "
                           "slot's event (hipEventSynchronize :1192); the first call on a handle allocates prep_coef (dev_alloc :1206)"),
    "mcm_jpeg_reconstruct": (HOST_STAGED, "meta / quant / rgb_offsets are host arrays read at call time :1247-1273; the first call "
                             "allocates the ring :1226-1238; waits on the slot's event :1242; a larger batch grows the planes buffer with "
                             "hipStreamSynchronize + hipFree + hipMalloc :1275-1283"),
    # ---- banks, metrics, Mahalanobis
    "mcm_reduce_bank": (REPLAYABLE, "one launch_bank_reduce on s :1296 (embed.hip:385): [s]"),
    "mcm_measures": (SYNCHRONISING, "out_host is written by a hipMemcpyAsync :1321 and the call ends in hipStreamSynchronize(s) :1323; "
                     "scores beyond the workspace get hipMallocAsync / hipFreeAsync on s :1316, :1322"),
    "mcm_score_histogram": (REPLAYABLE, "launch_histogram :1334 (metrics.hip:173) — counts zeroed by launch_zero_spans [zero], then "
                            "hist_kernel on s; integer atomics, so the sums do not depend on order: [s]"),
    "mcm_maha_prepare": (REPLAYABLE, "one launch_maha_prepare on s :853 (score.hip:359): [s]"),
    "mcm_maha_score_features": (REPLAYABLE, "one launch_maha_score on s :863 (score.hip:366): [s]"),
    "mcm_maha_fit_accumulate": (REPLAYABLE, "one launch_maha_fit on s :875 (score.hip:352); it adds into the caller's gram_dev / "
                                "sum_dev, so a replay continues from what they hold: [s]"),
    # ---- operators
    "mcm_op_linear": (REPLAYABLE, "forwards to mcm_op_linear_ex :1538"),
    "mcm_op_linear_ex": (REPLAYABLE, "launch_gemm on s :1561 (gemm.hip:1510: one launch, or two when gemm_route cuts a sliver round): [s]"),
    "mcm_op_split_weight": (REPLAYABLE, "one launch_cvt_weight_split on s :1570 (embed.hip:419): [s]"),
    "mcm_op_layernorm": (REPLAYABLE, "one launch_layernorm on s :1578 (layernorm.hip:205): [s]"),
    "mcm_op_layernorm_split": (REPLAYABLE, "one launch_layernorm (split) on s :1586: [s]"),
    "mcm_op_attention": (REPLAYABLE, "one launch_attention on s :1601 (attention.hip, every route through launch_lds or "
                         "hipLaunchKernelGGL on s): [s]"),
    "mcm_op_attention_split": (REPLAYABLE, "one launch_attention (split) on s :1594: [s]"),
    # ---- the saturation watch
    "mcm_saturation_count": (SYNCHRONISING, "hipMemcpyAsync of the counter to a host word :1499, hipMemsetAsync on reset :1500, "
                             "hipStreamSynchronize(s) :1501"),
}


def classes(cls):
    """The names of one class, sorted."""
    return sorted(n for n, (c, _) in CONTRACT.items() if c == cls)


def stream_entries(include_dir=None):
    """The exported prototypes with a parameter named `stream`, read from the headers as mcm_amd/abi.py reads them: comments and the
    #ifdef MCM_HARNESS block dropped, one declaration per `;`, every parameter a type and a name."""
    include_dir = include_dir or os.path.dirname(abi.HEADER_PATH)
    found = set()
    for name in HEADERS:
        with open(os.path.join(include_dir, name)) as f:
            text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
        text = re.sub(r"#ifdef MCM_HARNESS\b.*?#endif", "", text, flags=re.S)
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
        for decl in (" ".join(d.split()) for d in text.split(";")):
            m = re.fullmatch(r".*?\b(mcm_\w+) ?\(([^(){}]*)\)", decl)
            if not m or m[2].strip() == "void":
                continue
            params = [re.fullmatch(r".*?(\w+)", p.strip()) for p in m[2].split(",")]
            if any(p and p[1] == "stream" for p in params):
                found.add(m[1])
    return found
