"""Error model of the exact-GELU epilogues (EPI_GELU_ERF / EPI_GELU_ERF_X2, common.hpp gelu_erf), in the style of
tests/error_budget.py: an fp64 reference and a per-element budget on |got - ref| (pure numpy / torch-CPU, no GPU).

Reference: ref = 0.5 lin erfc(-lin / sqrt 2) in float64, the cancellation-free form (0.5 lin (1 + erf(lin / sqrt 2)) loses
every digit below lin ~ -5.5).  lin and s come from error_budget.gemm_reference on the exact operands.

Budget of one output:
    pre = GELU_ERF_DERIV * acc + C_GELU_ERF * u32 * |lin|,     acc = C_ACC u32 s + u32 |lin|   (gemm_budget's own)
then the store rule of the mode exactly as gemm_budget / gemm_split_budget apply it.

GELU_ERF_DERIV = 1.129 = max |Phi(x) + x phi(x)|, attained at x = sqrt 2 (1.12890; test_gelu_budget.py checks it).

C_GELU_ERF = 8, and the term is relative to |lin|, NOT to |ref|.  Both come from the reference's own arithmetic, not from
the kernel: torch's fp32 gelu (what HF's GELUActivation calls) is off from the fp64 reference by at most 6.38 u32 |x| over a
4e7-point grid on [-12, 12] and 1e7 normal draws on the CPU; 8 is a bound that arithmetic itself meets with 25 % to spare
(test_gelu_budget.py re-measures it on a smaller grid).  In the negative tail torch returns 0 for a non-zero true value
(x = -12): an error of 100 % of |ref| and of nothing of |x|, which is why no bound relative to |ref| can hold there, and why
it does not matter: fc2 multiplies the value by an O(1) weight beside O(1) neighbours.

There is ONE device form, gelu_erf, in every precision mode and kernel (common.hpp): no fast form, so no second constant.
"""
from __future__ import annotations

import numpy as np

from tests import error_budget as eb

GELU_ERF_DERIV = 1.129
C_GELU_ERF = 8.0


def gelu_erf64(z) -> np.ndarray:
    """0.5 z erfc(-z / sqrt 2) in float64."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64))
    return (0.5 * t * torch.special.erfc(-t / np.sqrt(2.0))).numpy()


def act_budget(x, ref=None) -> np.ndarray:
    """The activation term alone (the element-wise device function on an fp32 input x): C_GELU_ERF u32 |x| plus one fp32
    ulp of the reference."""
    x = np.asarray(x, np.float64)
    ref = gelu_erf64(x) if ref is None else ref
    return C_GELU_ERF * eb.U32 * np.abs(x) + eb.ulp(ref, "fp32")


def gemm_gelu_budget(lin, s, out: str, out_split: bool = False, din=0.0):
    """(ref, budget) of one output of a GEMM with the exact-GELU epilogue (mcm_op_linear_ex, epilogue 1 with
    MCM_LINEAR_ACT_GELU).  out: "bf16" / "fp16" / "fp32", the stored format; out_split: the output is a split fp16 image
    (MCM_LINEAR_SPLIT_OUT), `got` then being hi + lo.  din: an error of the operands themselves carried into lin
    (error_budget.gemm_unsplit_budget's term)."""
    lin = np.asarray(lin, np.float64)
    acc = eb.C_ACC * eb.U32 * s + eb.U32 * np.abs(lin) + din
    ref = gelu_erf64(lin)
    pre = GELU_ERF_DERIV * acc + C_GELU_ERF * eb.U32 * np.abs(lin)
    if out_split:
        bud = eb.ulp(ref, "fp32") + pre
        return ref, bud + eb.split_repr(np.abs(ref) + bud)
    if out == "fp32":
        return ref, eb.ulp(ref, "fp32") + pre
    bud = 0.5 * eb.ulp(np.abs(ref) + pre, out) + pre
    if out == "fp16":
        bud = np.where(np.abs(ref) + pre < eb.FP16_MAX, bud, np.inf)
    return ref, bud
