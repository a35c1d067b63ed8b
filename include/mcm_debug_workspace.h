/* mcm_debug_workspace.h — an extension of the harness part of include/mcm.h: two entries of libmcm_hip_harness.so only
 * (-DMCM_HARNESS; libmcm_hip.so does not export them) for the tests that hold a handle's results independent of what the handle
 * ran before (tests/test_gpu_handle_history.py).  They are declared here, not in mcm.h, for the reason mcm_score_stream.h gives:
 * the symbol set of mcm.h is what tests/golden/abi_prototypes.json froze; mcm_amd/abi.py reads this header with the same rules
 * and keeps its entries in a table of their own (EXTENSION_HARNESS_PROTOTYPES). */
#ifndef MCM_DEBUG_WORKSPACE_H
#define MCM_DEBUG_WORKSPACE_H

#include "mcm.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifdef MCM_HARNESS
/* hipMemsetAsync of `byte` (0 ... 255) over the full allocated size, pad rows included, of the activation buffers the towers
 * share (the residual stream, the LayerNorm output, q / k / v, the attention output, the MLP hidden), of the patch matrix and
 * of the feature scratch of the fused scores.  Nothing else is touched: no staging ring, no index buffer, no counter, no weight,
 * no fault word.  Data only: no shipped kernel branches or waits on what these buffers hold.  Asynchronous on `stream`.
 * MCM_EINVAL for a NULL h or a byte outside 0 ... 255. */
int mcm_debug_workspace_fill(mcm_handle* h, int32_t byte, void* stream);
/* The walk direction the next tower launch of the handle takes (it alternates per GEMM, LayerNorm and attention launch of
 * the towers; the operator-level entries mcm_op_* neither read nor move it): *parity_out (may be NULL) = 0 or 1 as it stands,
 * then it becomes `set` where that is 0 or 1; -1 leaves it.  Host state only, nothing is launched.  MCM_EINVAL for a NULL h or
 * another `set`. */
int mcm_debug_walk_parity(mcm_handle* h, int32_t set, int32_t* parity_out);
#endif

#ifdef __cplusplus
}
#endif

#endif /* MCM_DEBUG_WORKSPACE_H */
