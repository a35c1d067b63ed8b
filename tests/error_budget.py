"""Error model of the hot-path kernels: fp64 references and per-element error budgets (pure numpy, no GPU).

Every budget is a bound on |got - ref| for one output element, where ref is computed in float64 on the exact operands the
kernel multiplies (for the 16-bit modes: the already-rounded x, w, qkv).  Each term names the kernel step it covers; a
GPU test passes when max |got - ref| / budget <= 1.  tests/test_error_budget.py proves on the CPU that correct emulations
of each kernel stay inside these budgets and that a list of plausible kernel mistakes does not.

u32 = 2^-24 is the unit roundoff of fp32.  The one free constant is C_ACC, the multiple of u32 * sum_k |x_k w_k| that an
fp32 dot product may be off by.  It was chosen on the CPU (tests/test_error_budget.py::test_c_acc_covers_cpu_dot_products):
a sequential fp32 dot product (the order of a chain of v_mfma_f32_* accumulating one K-step after another) and torch's
CPU fp32 matmul stay below C_ACC / 2 at every K from 64 to 4096 on the tests' operand distributions.
"""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24
# unit roundoff of the 16-bit formats (RNE: half the relative spacing)
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
# (significand bits incl. the implicit one, smallest normal exponent)
_FMT = {"fp32": (24, -126), "bf16": (8, -126), "fp16": (11, -14)}
FP16_MAX = 65504.0

C_ACC = 16.0        # fp32 accumulation of a dot product: |err| <= C_ACC * u32 * sum |x_k w_k|
GELU_DERIV = 1.13   # max |d/dx x sigmoid(1.702 x)| (attained near x = 1.5)
C_GELU = 4.0        # quick_gelu_fast (common.hpp): v_exp_f32 + v_rcp_f32, ~1 ulp each, and the final product
C_EXP = 4.0         # v_exp_f32 (attention.hip) / expf (score.hip): a few ulps relative


def ulp(x, dtype: str) -> np.ndarray:
    """Spacing of the format `dtype` ("fp32", "bf16", "fp16") at |x|, subnormal spacing included
    (fp16: 2^-24 below 2^-14; bf16 / fp32: 2^-133 / 2^-149)."""
    p, emin = _FMT[dtype]
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, emin), emin)
    return np.ldexp(1.0, (e - (p - 1)).astype(np.int64))


def round_to(a, dtype: str) -> np.ndarray:
    """Round-to-nearest-even into a 16-bit format (returned as float32 values)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to({"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]).float().numpy()


def sample_rows(M: int, extra=()) -> np.ndarray:
    """Rows to check of a large problem: the first and last 256 and both sides of every 64-row boundary (so of every 128 /
    256 tile boundary too), plus `extra` (e.g. both sides of a launch split)."""
    r = set(range(min(M, 256))) | set(range(max(0, M - 256), M))
    for b in range(64, M, 64):
        r.update((b - 1, b))
    r.update(int(i) for i in extra if 0 <= i < M)
    return np.array(sorted(r), dtype=np.int64)


def quick_gelu64(z):
    return z / (1.0 + np.exp(-1.702 * z))


# ---- GEMM ---------------------------------------------------------------------------------------------------------------
def gemm_reference(x, w, bias):
    """fp64 lin = x w^T + bias and s = |x| |w|^T on the operands as given (rows of x already sampled)."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    lin = x64 @ w64.T + np.asarray(bias, np.float64)[None, :]
    s = np.abs(x64) @ np.abs(w64).T
    return lin, s


def gemm_budget(lin, s, out: str, epi: int, resid0=None):
    """(ref, budget) of one GEMM output.  out: the output format of the mode ("bf16" / "fp16" / "fp32"); epi 0: bias,
    1: bias + QuickGELU, 2: resid0 + lin into the fp32 residual (every mode).  fp16 elements beyond the fp16 range get an
    infinite budget (they saturate by design: test_gpu_kernels.py::test_fp16_outputs_saturate_instead_of_overflowing)."""
    lin = np.asarray(lin, np.float64)
    # fp32 accumulation of the K products (MFMA chain over the K-steps), then the fp32 bias add (wave_epilogue: acc + bv)
    acc = C_ACC * U32 * s + U32 * np.abs(lin)
    if epi == 2:
        ref = np.asarray(resid0, np.float64) + lin
        return ref, ulp(ref, "fp32") + acc          # the fp32 residual add: <= 1/2 ulp, and the accumulation
    if epi == 1:
        ref = quick_gelu64(lin)
        # |gelu'| <= 1.13 carries the accumulation error through; quick_gelu_fast's own error: a few fp32 ulps of the
        # result plus the rounding of its exponent argument -1.702 log2(e) x (relative u32 * 1.702 |x| in exp)
        pre = GELU_DERIV * acc + U32 * np.abs(ref) * (C_GELU + 1.702 * np.abs(lin))
    else:
        ref = lin
        pre = acc
    if out == "fp32":
        bud = ulp(ref, "fp32") + pre
    else:
        bud = 0.5 * ulp(np.abs(ref) + pre, out) + pre   # RNE of the fp32 value (which may sit in the next binade)
        if out == "fp16":
            bud = np.where(np.abs(ref) + pre < FP16_MAX, bud, np.inf)
    return ref, bud


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------
def layernorm_reference(x, g, b, eps=1e-5):
    """Two-pass fp64 LayerNorm of the fp32 rows x."""
    x64 = np.asarray(x, np.float64)
    mu = x64.mean(axis=1, keepdims=True)
    c = x64 - mu
    var = (c * c).mean(axis=1, keepdims=True)
    return c / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def layernorm_budget(x, g, b, out: str, eps=1e-5):
    """(ref, budget) of the LayerNorm kernel (ln_row.hpp: fp32 two-pass statistics, one wave per row)."""
    x64 = np.asarray(x, np.float64)
    D = x64.shape[1]
    ref = layernorm_reference(x, g, b, eps)
    mu = x64.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x64 - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    g64, b64 = np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(b, np.float64))
    depth = math.ceil(math.log2(D)) + 4
    # the fp32 row sum (ln_part_sum: <= 16 values per lane, then the 6-step wave_sum: a tree of depth <= log2(D) + 4) and
    # the division by D: the mean is off by this much, and every centred value with it (x - mean is exact-ish)
    dmean = depth * U32 * np.abs(x64).mean(axis=1, keepdims=True) + U32 * np.abs(mu)
    # the centred sum of squares (same tree, relative), var / D + eps, sqrtf and 1 / . (ln_rstd), x * rstd and the fma
    # with gamma, beta (ln_scale): relative to the normalised value, plus the fma's rounding against beta
    norm = np.abs(ref - np.asarray(b, np.float64))
    bud_f32 = dmean * rstd * g64 + (0.5 * depth + 6) * U32 * norm + U32 * b64
    if out == "fp32":
        return ref, bud_f32 + 0.5 * ulp(ref, "fp32")
    bud = 0.5 * ulp(np.abs(ref) + bud_f32, out) + bud_f32
    if out == "fp16":
        bud = np.where(np.abs(ref) + bud_f32 < FP16_MAX, bud, np.inf)
    return ref, bud


# ---- attention ---------------------------------------------------------------------------------------------------------
def attention_budget(q, k, v, causal: bool, out: str, scale=0.125):
    """(ref, budget) of one (sequence, head): q, k, v [L, 64] (the rounded operands), fp64 softmax reference.
    out: the mode's format; P (the unnormalised softmax, max 1) is rounded to it before P.V in the 16-bit modes
    (attention.hip: pack2 of exp2 in attn_bf16_kernel / attn_tr_kernel), kept in fp32 in the fp32 kernels."""
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    L = q64.shape[0]
    s = scale * (q64 @ k64.T)
    sa = scale * (np.abs(q64) @ np.abs(k64).T)
    if causal:
        mask = np.tril(np.ones((L, L), bool))
        s = np.where(mask, s, -np.inf)
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    p = e / e.sum(axis=1, keepdims=True)
    ref = p @ v64
    pv = p @ np.abs(v64)                                       # sum_j p_j |v_j|
    dev = np.einsum("qj,qjd->qd", p, np.abs(v64[None, :, :] - ref[:, None, :]))   # sum_j p_j |v_j - ref|
    # logit perturbation per key, relative in e_j: S = QK^T on the MFMA (fp32 accumulate), the fma s*SC - m*SC rounded in
    # fp32 (exponent argument), and v_exp_f32 / expf
    sfin = np.where(np.isfinite(s), np.abs(s), 0.0)
    ds = C_ACC * U32 * sa + U32 * (sfin + np.abs(m)) * 2.0 + C_EXP * U32
    if causal:
        ds = np.where(mask, ds, 0.0)
    dsmax = ds.max(axis=1, keepdims=True)
    uP = U16.get(out, U32)
    bud = (2.0 * uP * pv                       # P rounded to the operand format; the row sum over fp32 or rounded P
           + dsmax * dev                       # logit / exp error, carried through the softmax
           + C_ACC * U32 * pv                  # fp32 accumulation of P.V
           # the fp32 row sum: one add per 16-key tile in each lane plus the two cross-lane adds (attn_bf16_kernel), or
           # the all-ones MFMA accumulating per 32-key step (attn_tr_kernel); a sum of positive terms, relative error
           + (math.ceil(L / 16) + 4) * U32 * np.abs(ref)
           + 2.0 * U32 * np.abs(ref))          # 1 / rowsum and the final product
    if out == "fp16":
        bud = bud + L * 2.0 ** -25 * np.abs(v64).max()   # P below 2^-14 lands on fp16's subnormal grid (spacing 2^-24)
    if out == "fp32":
        bud = bud + 0.5 * ulp(ref, "fp32")
    else:
        bud = 0.5 * ulp(np.abs(ref) + bud, out) + bud
    return ref, bud


def attention_qkv_budget(qkv, nseq, L, heads, causal, out, pairs=None):
    """attention_budget over the (sequence, head) pairs of a [nseq * L, 3 * heads * 64] qkv (all pairs by default).
    Returns {(n, h): (ref [L, 64], budget [L, 64])}."""
    D = heads * 64
    res = {}
    for n, h in (pairs if pairs is not None else [(n, h) for n in range(nseq) for h in range(heads)]):
        rows = qkv[n * L:(n + 1) * L]
        q = rows[:, h * 64:(h + 1) * 64]
        k = rows[:, D + h * 64:D + (h + 1) * 64]
        v = rows[:, 2 * D + h * 64:2 * D + (h + 1) * 64]
        res[(n, h)] = attention_budget(q, k, v, causal, out)
    return res


# ---- scores ------------------------------------------------------------------------------------------------------------
def score_reference(img, txt, T: float, kind: int):
    """fp64 scores of all five kinds (reference utils/detection_util.py:232-248); kind as mcm_amd.config.SCORE_KINDS:
    0 MCM, 1 max-logit, 2 energy, 3 entropy, 4 var.  Returns (score [B], sim [B, K])."""
    sim = np.asarray(img, np.float64) @ np.asarray(txt, np.float64).T
    if kind == 1:
        return -sim.max(axis=1), sim
    u = sim / T - (sim.max(axis=1, keepdims=True) / T)
    e = np.exp(u)
    z = e.sum(axis=1)
    p = e / z[:, None]
    if kind == 0:
        return -1.0 / z, sim
    if kind == 2:
        return -T * (sim.max(axis=1) / T + np.log(z)), sim
    if kind == 3:
        return np.log(z) - (p * u).sum(axis=1), sim
    return -p.var(axis=1), sim


def score_budget(img, txt, T: float, kind: int):
    """(ref, budget) of score.hip: fp32 fmaf dot products (one wave per prompt), fp32 u = s / T - m / T and expf, fp64 sums
    of the K terms, then each kind's closing arithmetic."""
    ref, sim = score_reference(img, txt, T, kind)
    sa = np.abs(np.asarray(img, np.float64)) @ np.abs(np.asarray(txt, np.float64)).T
    dsim = C_ACC * U32 * sa                                   # the similarities' fp32 dot products
    if kind == 1:
        return ref, dsim.max(axis=1) + 0.5 * ulp(ref, "fp32")
    mt = sim.max(axis=1, keepdims=True) / T
    u = sim / T - mt
    # per-term perturbation of u (absolute) = relative perturbation of e: the dot product, s / T, m / T and the subtraction
    du = dsim / T + U32 * (np.abs(sim / T) + 2 * np.abs(mt) + np.abs(u))
    dumax = du.max(axis=1)
    eps_e = C_EXP * U32                                       # expf
    e = np.exp(u)
    z = e.sum(axis=1)
    p = e / z[:, None]
    if kind == 0:     # -1 / z in fp64, rounded to fp32
        bud = np.abs(ref) * (dumax + eps_e) * 1.01
    elif kind == 2:   # -(T * (mt + (float)log z)): log z in fp64, the add and the product in fp32
        bud = T * (dumax + eps_e) * 1.01 + U32 * (np.abs(mt[:, 0]) + np.abs(np.log(z))) * T + U32 * np.abs(ref)
    elif kind == 3:   # H = log z - sum(e u) / z in fp64: d H / d u_k = -p_k (u_k - ubar), the e_k error weights p_k |1 - u_k + ubar|
        ubar = (p * u).sum(axis=1, keepdims=True)
        spread = (p * np.abs(u - ubar)).sum(axis=1)
        bud = dumax * spread + eps_e * (1.0 + spread) + U32 * (np.abs(u) * p).sum(axis=1)
    else:             # -var(p) with p_k = e_k * (float)(1 / z) in fp32: relative error r per p_k, d var = 2/K sum (p - 1/K) dp
        K = p.shape[1]
        r = 2 * (dumax + eps_e) + 3 * U32
        bud = (2.0 / K) * r * (np.abs(p - 1.0 / K) * p).sum(axis=1)
    return ref, bud + 0.5 * ulp(ref, "fp32")


def worst(got, ref, bud):
    """max |got - ref| / budget over the elements, and the flat index of the worst one (NaN in got counts as infinite)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    ratio = np.where(np.isinf(bud), 0.0, err / bud)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i
