"""Error model of the hot-path kernels: fp64 references and per-element error budgets (pure numpy, no GPU).

Every budget is a bound on |got - ref| for one output element, where ref is computed in float64 on the exact operands the
kernel multiplies (for the 16-bit modes: the already-rounded x, w, qkv).  Each term names the kernel step it covers; a
GPU test passes when max |got - ref| / budget <= 1.  tests/test_error_budget.py proves on the CPU that correct emulations
of each kernel stay inside these budgets and that a list of plausible kernel mistakes does not.

u32 = 2^-24 is the unit roundoff of fp32.  The one free constant is C_ACC, the multiple of u32 * sum_k |x_k w_k| that an
fp32 dot product may be off by.  It was chosen on the CPU (tests/test_error_budget.py::test_c_acc_covers_cpu_dot_products):
a sequential fp32 dot product (the order of a chain of v_mfma_f32_* accumulating one K-step after another) and torch's
CPU fp32 matmul stay below C_ACC / 2 at every K from 64 to 4096 on the tests' operand distributions.
The split forms (split activations, split weights) run chains of 2K and 4K products in one fp32 accumulator (2 x 4096 at
L/14 fc2, 4 x 3072 at B/16 fc2 with both split); C_ACC = 16 covers them unchanged: the kernel-order chain stays below
6.6 u32 * sum |x||w| there (tests/test_error_budget.py::test_c_acc_covers_split_chains).
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


def layernorm_budget(x, g, b, out: str, eps=1e-5, depth=None):
    """(ref, budget) of the LayerNorm kernel (ln_row.hpp: fp32 two-pass statistics, one wave per row).
    depth: the depth of the summation tree when it is not the row kernel's (pool_project_budget)."""
    x64 = np.asarray(x, np.float64)
    D = x64.shape[1]
    ref = layernorm_reference(x, g, b, eps)
    mu = x64.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x64 - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    g64, b64 = np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(b, np.float64))
    if depth is None:
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


# ---- Mahalanobis --------------------------------------------------------------------------------------------------------
U64 = 2.0 ** -53    # unit roundoff of fp64
# An fp64 dot product of P terms is off by at most P u64 sum |a||b| whatever the order (gamma_P).  Each of the three terms of
# d = q - W.f + k is two such levels deep: q = sum_p f_p (P f)_p and k = sum_p mu_p (P mu)_p are a sum of P inner dot
# products, W.f a dot product with a W whose elements are themselves P-term dot products: 2 P u64 of the absolute sums.
# The score is 0.5 d (an exact product), so in terms of the score the constant is 0.5 * 2.
C_MAHA = 1.0


def maha_reference(feats, means, prec):
    """fp64 min_c 0.5 (f - mu_c)^T P (f - mu_c), the direct form of reference utils/detection_util.py:176-207 on the fp32
    inputs (the differences are taken in fp64; P is used as given, not symmetrised).  Returns (score [B], argmin [B])."""
    f64, m64, p64 = (np.asarray(a, np.float64) for a in (feats, means, prec))
    score, arg = np.empty(f64.shape[0]), np.empty(f64.shape[0], np.int64)
    for b in range(f64.shape[0]):
        d = f64[b][None, :] - m64                                     # [C, P]
        v = 0.5 * np.einsum("cp,cp->c", d @ p64, d)
        arg[b] = int(np.argmin(v))
        score[b] = v[arg[b]]
    return score, arg


def maha_budget(feats, means, prec):
    """(ref, budget) of maha_prepare_kernel + maha_score_kernel (score.hip): W_c = P mu_c + P^T mu_c and k_c = mu_c^T P mu_c
    accumulated in fp64 once per class, then per feature q = f^T P f and W_c . f in fp64, d_c = q - W_c . f + k_c (the three
    terms cancel when f is near mu_c: the error is relative to the terms, not to d), the minimum over the classes, one
    product with 0.5 (exact) and one rounding to fp32:
      0.5 ulp32(ref) + C_MAHA P u64 (|f|^T |P| |f| + |W_c| . |f| + |mu_c|^T |P| |mu_c|) at the reference's arg-min class c,
    the accumulation term with score_budget's 1 % slack."""
    f64, m64, p64 = (np.asarray(a, np.float64) for a in (feats, means, prec))
    P = p64.shape[0]
    ref, arg = maha_reference(feats, means, prec)
    pa = np.abs(p64)
    mu = m64[arg]                                                     # [B, P]
    w = mu @ p64.T + mu @ p64                                         # P mu + P^T mu per row
    fa, ma = np.abs(f64), np.abs(mu)
    terms = np.einsum("bp,bp->b", fa @ pa.T, fa) + np.einsum("bp,bp->b", np.abs(w), fa) + np.einsum("bp,bp->b", ma @ pa.T, ma)
    return ref, 0.5 * ulp(ref, "fp32") + C_MAHA * P * U64 * terms * 1.01


def maha_case(P: int, C: int, B: int, where: str, pkind: str, seed: int = 0):
    """(feats [B, P], means [C, P], prec [P, P]) fp32 for the Mahalanobis checks.
    pkind "asym": a well-conditioned A A^T / P + I with asymmetric perturbations (P[0, 1] += 0.01 and 1 % noise on the upper
    triangle only); "scaled": a diagonal spanning 1e-3 .. 1e3 plus small off-diagonal noise.
    where "far": features unrelated to any mean; "near": a class mean + 1e-2 noise; "equal": a class mean exactly; "mixed":
    rows cycling through the three.  Row b of the near / equal kinds sits at class (C - 1 - b) % C: the last class first."""
    rng = np.random.default_rng(seed + 7 * P + 13 * C)                # means and precision depend on (P, C, pkind) alone
    means = (3.0 * rng.standard_normal((C, P))).astype(np.float32)
    if pkind == "asym":
        a = rng.standard_normal((P, P))
        prec = a @ a.T / P + np.eye(P)
        prec += np.triu(0.01 * rng.standard_normal((P, P)), 1)
        prec[0, 1] += 0.01
    else:
        prec = np.diag(np.logspace(-3, 3, P)) + 1e-4 * rng.standard_normal((P, P))
    prec = prec.astype(np.float32)
    cls = (C - 1 - np.arange(B)) % C
    rng = np.random.default_rng([seed, P, C, B])
    far = (3.0 * rng.standard_normal((B, P))).astype(np.float32)
    near = (means[cls] + 0.01 * rng.standard_normal((B, P))).astype(np.float32)
    rows = {"far": far, "near": near, "equal": means[cls].copy()}
    if where == "mixed":
        feats = np.stack([rows[("far", "near", "equal")[b % 3]][b] for b in range(B)])
    else:
        feats = rows[where]
    return np.ascontiguousarray(feats), means, prec


# ---- split forms: one value as an fp16 pair hi + lo (split activations, split outputs, split weights) -------------------
FP16_SAT = 65520.0    # the first |v| that rounds above 65504: what sat_report counts (common.hpp)
U_SPLIT = 2.0 ** -22  # relative representation error of a split in fp16's normal range (split_repr)


def f16_sat(a) -> np.ndarray:
    """fp32 -> fp16 as v_cvt_pk_f16_f32 does it under MODE.FP16_OVFL (common.hpp enter_precision_mode): round to nearest
    even, fp16 subnormals included; finite values beyond the range saturate to +-65504."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    return np.where(np.isinf(h) & np.isfinite(a), np.copysign(np.float16(FP16_MAX), a).astype(np.float16), h)


def split2_f16(v):
    """common.hpp split2<MCM_PREC_F16> bit for bit: hi = f16_sat(v), lo = f16_sat(v - hi), the difference taken in fp32
    (exact below the range edge).  Returns (hi, lo) as float16 arrays."""
    v = np.asarray(v, np.float32)
    hi = f16_sat(v)
    lo = f16_sat(v - hi.astype(np.float32))
    return hi, lo


def split_image(x) -> np.ndarray:
    """fp32 [M, K] (K % 64 == 0) -> the split image [M, 2K] as float16 (split2_f16's bits): per 64 columns hi[64] then
    lo[64]."""
    x = np.asarray(x, np.float32)
    M, K = x.shape
    hi, lo = split2_f16(x)
    out = np.empty((M, K // 64, 2, 64), np.float16)
    out[:, :, 0, :] = hi.reshape(M, K // 64, 64)
    out[:, :, 1, :] = lo.reshape(M, K // 64, 64)
    return out.reshape(M, 2 * K)


def image_parts(y):
    """split image [M, 2N] (16-bit values in any float dtype) -> (hi, lo), each [M, N] float64."""
    y = np.asarray(y)
    M, N2 = y.shape
    v = y.reshape(M, N2 // 128, 2, 64).astype(np.float64)
    return v[:, :, 0, :].reshape(M, N2 // 2), v[:, :, 1, :].reshape(M, N2 // 2)


def merge_image(y) -> np.ndarray:
    """split image [M, 2N] -> hi + lo [M, N] (exact in fp64, returned as float64)."""
    hi, lo = image_parts(y)
    return hi + lo


def split_repr(a) -> np.ndarray:
    """Representation term of a split: |v - hi - lo| for any v with |v| <= a, i.e. 1/2 ulp16 of the remainder v - hi.
    In fp16's normal range the remainder is at most 1/2 ulp16(v), so the term is 2^-22 |v| at the bottom of a binade and
    2^-23 |v| at its top (U_SPLIT).  Below |v| = 2^-3 the remainder is under 2^-14 and lo lands on fp16's subnormal grid
    (spacing 2^-24): an absolute floor of 2^-25.  Past the range edge hi saturates at 65504 (FP16_OVFL) and lo carries
    v - 65504 at fp16 precision, up to 131008 (+ its half ulp); beyond that lo saturates as well: no bound (infinite)."""
    a = np.abs(np.asarray(a, np.float64))
    rem = np.where(a < FP16_MAX, 0.5 * ulp(a, "fp16"), np.maximum(a - FP16_MAX, 16.0))
    return np.where(rem <= FP16_MAX + 16.0, 0.5 * ulp(rem, "fp16"), np.inf)


def gemm_split_budget(lin, s, epi: int, out_split: bool, resid0=None, din=0.0):
    """(ref, budget) of a split GEMM (mcm_op_linear_ex with MCM_LINEAR_SPLIT_X and / or SPLIT_W).

    lin, s: gemm_reference on the MERGED operands (hi + lo, exact in fp64), as the other budgets use the operands as given.
    Every pass of a logical K-step (X_hi W, X_lo W; with split weights four: X_hi W_hi, X_lo W_hi, X_hi W_lo, X_lo W_lo) is
    one more stretch of the same fp32 MFMA chain, so the accumulation term is C_ACC u32 sum |x||w| over the merged operands
    for a chain of 2K or 4K products (test_error_budget.py::test_c_acc_covers_split_chains).
      epi 2: the fp32 residual, gemm_budget's rule;
      epi 0 / 1 with a plain fp16 output (SPLIT_X without SPLIT_OUT): gemm_budget's fp16 rule (EPI_GELU: quick_gelu_fast);
      out_split (EPI_STORE_X2 / EPI_GELU_X2): the fp32-grade value plus split_repr of the stored pair.  EPI_GELU_X2 runs the
      exact QuickGELU of the fp32 arm, x / (1 + __expf(-1.702 x)) with an IEEE division: gemm_budget's fp32 GELU term (C_GELU
      ulps of the result and the rounding of the exponent argument) covers it.
    din: an error of the operands themselves, carried into lin (gemm_unsplit_budget)."""
    lin = np.asarray(lin, np.float64)
    acc = C_ACC * U32 * s + U32 * np.abs(lin) + din
    if epi == 2:
        ref = np.asarray(resid0, np.float64) + lin
        return ref, ulp(ref, "fp32") + acc
    if epi == 1:
        ref = quick_gelu64(lin)
        pre = GELU_DERIV * acc + U32 * np.abs(ref) * (C_GELU + 1.702 * np.abs(lin))
    else:
        ref, pre = lin, acc
    if not out_split:
        bud = 0.5 * ulp(np.abs(ref) + pre, "fp16") + pre
        return ref, np.where(np.abs(ref) + pre < FP16_MAX, bud, np.inf)
    bud = ulp(ref, "fp32") + pre
    return ref, bud + split_repr(np.abs(ref) + bud)


def gemm_unsplit_budget(x, w, bias, epi: int, out_split: bool, resid0=None, x_split=True, w_split=False):
    """The split arm's own claim, fp32 round-off of the UNSPLIT fp32 operands, as a budget: (ref, budget) against the fp64
    product of the fp32 x [M, K] and w [N, K], with the representation error of each split input (split_repr per element)
    carried through the product: sum_k |dx_k| |w_k| + |x_k| |dw_k| + |dx_k| |dw_k|.  An unsplit input is taken as given."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    lin, s = gemm_reference(x64, w64, bias)
    dx = split_repr(x64) if x_split else np.zeros_like(x64)
    dw = split_repr(w64) if w_split else np.zeros_like(w64)
    din = dx @ np.abs(w64).T + np.abs(x64) @ dw.T + dx @ dw.T
    return gemm_split_budget(lin, s, epi, out_split, resid0, din)


def layernorm_split_budget(x, g, b, eps=1e-5):
    """(ref, budget) of mcm_op_layernorm_split (ln_row_store<X2>): the fp32 LayerNorm value, stored as a split pair."""
    ref, bud = layernorm_budget(x, g, b, "fp32", eps)
    return ref, bud + split_repr(np.abs(ref) + bud)


P_SCALE_LOG2 = 12   # the split attention kernels split P after a scale of 2^12 (attention.hip: msc = m * SC - 12)


def attention_split_rows(qh, ql, kh, kl, vh, vl, scale=0.125):
    """Terms of split attention (attn_tr_kernel<X2>, attn_long_kernel<X2>) for the query rows of qh / ql against all keys,
    from the hi and lo halves [*, 64] of q, k, v.  The reference is fp64 softmax attention on the merged operands hi + lo.
    Returns (ref, bud, dev, pv, smax), bud before the output is stored.
      S = K_lo Q_hi + K_hi Q_lo + K_hi Q_hi, one fp32 chain of 3 x 64 products; the dropped Q_lo K_lo joins the logit
        perturbation as scale |Q_lo| |K_lo|^T;
      P = exp2(s SC - m SC + 12), 2^12 times the unnormalised softmax, split: relative U_SPLIT and the subnormal floor 2^-25
        of the scaled value, i.e. 2^-37 of P.  There is no L 2^-25 max|v| term of the fp16 arm here: the scale removes it;
      O = V_lo P_hi + V_hi P_lo + V_hi P_hi in one fp32 chain; the dropped P_lo V_lo (|P_lo| <= 2^-11 P + the floor) is a
        term of its own; the row sum runs over P_lo and P_hi (the all-ones MFMA: two passes per 32-key step)."""
    qh, ql, kh, kl, vh, vl = (np.asarray(a, np.float64) for a in (qh, ql, kh, kl, vh, vl))
    q, k, v = qh + ql, kh + kl, vh + vl
    L = k.shape[0]
    s = scale * (q @ k.T)
    sa = scale * ((np.abs(qh) + np.abs(ql)) @ (np.abs(kh) + np.abs(kl)).T)
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    p = e / e.sum(axis=1, keepdims=True)
    ref = p @ v
    va = np.abs(vh) + np.abs(vl)
    pv = p @ va
    dev = np.einsum("qj,qjd->qd", p, np.abs(v[None, :, :] - ref[:, None, :]))
    ds = (C_ACC * U32 * sa + U32 * (np.abs(s) + np.abs(m)) * 2.0 + C_EXP * U32
          + scale * (np.abs(ql) @ np.abs(kl).T))                   # the dropped Q_lo K_lo
    dsmax = ds.max(axis=1, keepdims=True)
    p_floor = 2.0 ** (-25 - P_SCALE_LOG2)                          # per key, in units of the row's largest P (1)
    bud = (2.0 * U_SPLIT * pv + 2.0 * L * p_floor * va.max()       # P's split, in O and in the row sum
           + dsmax * dev                                           # logit / exp error, carried through the softmax
           + C_ACC * U32 * pv                                      # fp32 accumulation of the three P.V passes
           + 2.0 ** -11 * (p @ np.abs(vl)) + L * p_floor * np.abs(vl).max()   # the dropped P_lo V_lo
           + (2 * math.ceil(L / 16) + 4) * U32 * np.abs(ref)      # the row sum over P_lo and P_hi
           + 2.0 * U32 * np.abs(ref))                              # 1 / rowsum and the final product
    return ref, bud, dev, pv, np.abs(s).max(axis=1, keepdims=True)


def attention_split_budget(qh, ql, kh, kl, vh, vl, scale=0.125, row_block=128):
    """(ref, budget) of one (sequence, head) of mcm_op_attention_split up to 288 keys: attention_split_rows plus the split
    of the stored output (split_repr).  The streaming form: online_softmax_budget.online_attention_split_budget."""
    refs, buds = [], []
    for r0 in range(0, np.shape(qh)[0], row_block):
        rb = slice(r0, r0 + row_block)
        ref, bud, _, _, _ = attention_split_rows(qh[rb], ql[rb], kh, kl, vh, vl, scale)
        refs.append(ref)
        buds.append(bud + split_repr(np.abs(ref) + bud))
    return np.concatenate(refs), np.concatenate(buds)


def head_parts(img, L, heads, n, h):
    """(qh, ql, kh, kl, vh, vl), each [L, 64] float64, of (sequence n, head h) of a split qkv image [nseq L, 6 heads 64]."""
    hi, lo = image_parts(np.asarray(img)[n * L:(n + 1) * L])
    D = heads * 64
    return tuple(a[:, o + h * 64:o + (h + 1) * 64] for o in (0, D, 2 * D) for a in (hi, lo))


def coherent_small_p_qkv(L, heads, nseq=1):
    """The input on which P split WITHOUT the 2^12 scale breaks the split attention budget.  In every (sequence, head) key 0
    dominates every query: raw logits q.k = +2t for key 0 and -2t for the L - 1 others (t ~ 25: after the 0.125 scale a gap
    of 12.5, P ~ 2^-18 against key 0).  All those P are equal, so their rounding errors add up instead of cancelling, and t
    is chosen (on a grid of 1/64, exact in fp16) so that the unscaled P's remainder after hi falls halfway between two points
    of fp16's subnormal grid: each lo then misses by nearly 2^-25, the largest error there is.  V is 0 for key 0 and 1 for
    the others (one sign).  Returns the fp32 qkv [nseq L, 3 heads 64]."""
    D = heads * 64
    SC = np.float32(0.125 * 1.4426950408889634)
    best = None
    for i in range(128):
        t = 24.0 + i / 64.0
        msc = np.float32(np.float64(2.0 * t) * np.float64(SC))             # the kernel's m * SC, unscaled
        arg = np.float32(np.float64(-2.0 * t) * np.float64(SC) - np.float64(msc))   # fmaf(s, SC, -msc)
        c = np.float32(np.exp2(np.float64(arg)))
        r = (np.float64(c) - np.float64(np.float16(c))) / 2.0 ** -24
        miss = abs(r - np.floor(r) - 0.5)
        if best is None or miss < best[0]:
            best = (miss, t)
    t = best[1]
    qkv = np.zeros((nseq * L, 3 * D), np.float32)
    for h in range(heads):
        qkv[:, h * 64] = 4.0
        qkv[:, D + h * 64] = -0.5 * t
        qkv[:, 2 * D + h * 64:2 * D + (h + 1) * 64] = 1.0
        for n in range(nseq):
            qkv[n * L, D + h * 64] = 0.5 * t
            qkv[n * L, 2 * D + h * 64:2 * D + (h + 1) * 64] = 0.0
    return qkv


# ---- the two ends of the towers: pixels / token ids -> residual stream, residual stream -> unit vectors -----------------
# preprocess constants of the reference (utils/train_eval_util.py:27-28), as fp32 (mcm_api.hip kClipMean / kClipStd)
CLIP_MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)
CLIP_STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)


def patchify_reference(px, P: int, kpad: int) -> np.ndarray:
    """fp32 NCHW pixels [B, 3, S, S] -> the patch matrix [B * np, kpad] (values unchanged): row b * np + gy * g + gx, column
    k = (c * P + py) * P + px, the [D, 3, P, P] weight's own flattening (embed.hip patchify_kernel); columns from 3 P P on
    are zero (L/14: 588 -> 640)."""
    px = np.asarray(px, np.float32)
    B, C, S, _ = px.shape
    g = S // P
    m = px.reshape(B, C, g, P, g, P).transpose(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P)
    out = np.zeros((B * g * g, kpad), np.float32)
    out[:, :C * P * P] = m
    return out


def u8_normalise(u8) -> np.ndarray:
    """uint8 NHWC [B, S, S, 3] -> fp32 NCHW: ((float32(u8) / 255f) - mean) / std, each operation rounded to fp32 in that
    order (patchify_u8_kernel; torchvision's ToTensor then Normalize).  HIP's fp32 division is correctly rounded, so is
    numpy's: the kernel's operand is expected to equal this bit for bit."""
    t = np.asarray(u8, np.uint8).astype(np.float32) / np.float32(255.0)
    v = (t - CLIP_MEAN) / CLIP_STD
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2), dtype=np.float32)


def operand_values(v, mode: str, x2: bool = False) -> np.ndarray:
    """The values an fp32 activation is multiplied as (float64): itself in fp32 mode, rounded to nearest even in the 16-bit
    modes (fp16: f16_sat), hi + lo of split2_f16 with x2."""
    v = np.asarray(v, np.float32)
    if x2:
        hi, lo = split2_f16(v)
        return hi.astype(np.float64) + lo.astype(np.float64)
    if mode == "fp32":
        return v.astype(np.float64)
    if mode == "fp16":
        return f16_sat(v).astype(np.float64)
    return round_to(v, mode).astype(np.float64)


def weight_values(w, mode: str, split: bool) -> np.ndarray:
    """The values a handle multiplies for the fp32 master weight w (float64): w in fp32 mode, round(w) as one 16-bit operand,
    or hi + lo with hi = round(w), lo = round(w - hi) when the handle holds split weights (embed.hip cvt_weight_split_kernel)."""
    w = np.asarray(w, np.float32)
    if mode == "fp32":
        return w.astype(np.float64)
    if not split:
        return round_to(w, mode).astype(np.float64)
    if mode == "fp16":
        hi, lo = split2_f16(w)
        return hi.astype(np.float64) + lo.astype(np.float64)
    hi = round_to(w, mode)
    return hi.astype(np.float64) + round_to(w - hi, mode).astype(np.float64)


def patch_embed_budget(patches, w, pos, n_patches: int, rows=None):
    """(ref, budget) of the EPI_PATCH epilogue (gemm.hip wave_epilogue / the LDS-staged epilogue of gemm_p256_kernel, plain and
    pixel-gathering): out[b (np + 1) + 1 + p] = pos[1 + p] + patches[b np + p] . w^T in fp32.  patches [M, K] and w [D, K] are
    the operands as multiplied (operand_values / weight_values, the K padding included), pos [np + 1, D] fp32; rows: the
    patch-matrix rows given (all M by default).  Returns arrays over those rows, in patch-matrix order.
    The terms are gemm_budget's residual rule with the position row in the residual's place: the fp32 add of the position
    row (<= 1/2 ulp, and the result may sit in the next binade: 1 ulp), the fp32 MFMA chain over the K-steps (2 K or 4 K
    products with a split operand: C_ACC covers them, test_c_acc_covers_split_chains), and the rounding of the chain's value
    (the epilogue's acc + 0 bias is exact)."""
    rows = np.arange(np.shape(patches)[0]) if rows is None else np.asarray(rows)
    lin, s = gemm_reference(patches, w, np.zeros(np.shape(w)[0]))
    return gemm_budget(lin, s, "fp32", 2, np.asarray(pos, np.float64)[1 + rows % n_patches])


def token_rows(B: int, n_patches: int, rows=None) -> np.ndarray:
    """Residual-stream row of each patch-matrix row: b np + p -> b (np + 1) + 1 + p."""
    rows = np.arange(B * n_patches) if rows is None else np.asarray(rows)
    return rows // n_patches * (n_patches + 1) + 1 + rows % n_patches


def cls_row(cls, pos) -> np.ndarray:
    """The CLS row layernorm_pre_kernel synthesises in registers: float32(class_embedding + position_embedding[0]), one
    correctly rounded add per element: exact, no budget."""
    return np.asarray(cls, np.float32) + np.asarray(pos, np.float32)[0]


def pre_ln_budgets(x0, x1, g0, b0, g1, b1, mode: str, x2: bool = False, eps=1e-5):
    """The fused pass of layernorm_pre_kernel as two applications of layernorm_budget.
      x0: the kernel's own fp32 input rows (the patch GEMM's rows, the CLS rows replaced by cls_row); pre_layrnorm of them is
          written back in fp32: budget 1, output format "fp32";
      x1: the fp32 rows the kernel wrote back.  It normalises exactly those values again (still in registers: ln_row_store
          <MCM_PREC_F32> stores v unchanged), into the mode's operand format: budget 2, or the split budget with x2.
    Both passes are ln_row_apply<0> (ln_row.hpp), the function layernorm_kernel calls: ln_part_sum adds (x + y) + (z + w) of up
    to four float4 per lane (depth <= 2 + 4), wave_sum is a 6-step butterfly: at most 12 <= ceil(log2 D) + 4 for every D from
    128 on, and D = 64 has one float4 in 16 lanes (depth 2 + 6 = 8 <= 10): layernorm_budget's depth term describes it.
    Returns ((ref_pre, bud_pre), (ref_ln1, bud_ln1))."""
    first = layernorm_budget(x0, g0, b0, "fp32", eps)
    second = layernorm_split_budget(x1, g1, b1, eps) if x2 else layernorm_budget(x1, g1, b1, mode, eps)
    return first, second


def eos_rows(ids) -> np.ndarray:
    """Pooled row of every prompt of ids [K, S]: k S + the FIRST position of the largest id (HF modeling_clip.py:561-581;
    mcm_encode_text_ex)."""
    ids = np.asarray(ids)
    return np.arange(ids.shape[0]) * ids.shape[1] + ids.argmax(axis=1)


POOL_WAVES = 16   # embed.hip NWP: waves of a pool_project workgroup


def l2_normalise_budget(o, do, n_add: int):
    """(ref, budget) of out = o / ||o||_2 per row, o known to within do per element, the sum of squares an fp32 sum of
    positive terms with at most n_add additions on any path.
      do / ||o||                      the element's own error, scaled;
      |out| ||do||_2 / ||o||          the norm's error from the elements' errors: | ||o + e|| - ||o|| | <= ||e||_2;
      |out| (n_add / 2 + 3) u32       the squares and their fp32 sum (relative (n_add + 1) u32 of the sum, half of it after the
                                      square root), sqrtf, 1 / . (both correctly rounded) and the product o * rn.
    A row of norm 0 has no finite budget (the kernels return 0 * inf there, as the reference's x / x.norm() does)."""
    o64, do = np.asarray(o, np.float64), np.asarray(do, np.float64)
    nrm = np.sqrt((o64 * o64).sum(axis=1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = o64 / nrm
        bud = do / nrm + np.abs(ref) * np.sqrt((do * do).sum(axis=1, keepdims=True)) / nrm \
            + np.abs(ref) * (0.5 * n_add + 3.0) * U32
    return ref, np.where(nrm > 0, bud + 0.5 * ulp(np.where(nrm > 0, ref, 0.0), "fp32"), np.inf)


def pool_project_budget(x, g, b, proj, normalize: bool, eps=1e-5):
    """(ref, budget) of pool_project_kernel (embed.hip) on the pooled fp32 rows x [n, D]; proj [P, D] fp32.
      LayerNorm   one element per thread, wave_sum (6 steps), the 16 wave partials added one after another by every thread:
                  a tree of depth 6 + 16 whatever D is (threads past D add exact zeros), against the row kernel's
                  ceil(log2 D) + 4 -> layernorm_budget with that depth, fp32 output (y in LDS): dy;
      projection  o_p = sum_d w_pd y_d, an fmaf chain of D / 64 terms per lane and the butterfly:
                  do = sum_d |w| dy + C_ACC u32 sum_d |w| |y|.  C_ACC is the file's one accumulation constant, chosen on
                  the CPU for fp32 dot products (test_c_acc_covers_cpu_dot_products); it is NOT a strict worst-case bound
                  here once D > 640: a path then has up to 16 fmaf roundings and 6 butterfly adds, 22 > 16.  The kernel-order
                  emulation stays below 0.14 of the whole budget at every D (test_pool_project_emulation_within_budget);
      normalise   the squares of a wave's outputs (every 16th p) summed by its lane 0 one after another (ceil(P / 16) terms),
                  then the 16 partials: l2_normalise_budget with n_add = ceil(P / 16) + 16.
    1024 < D <= 1280 (pool_project_kernel<WIDE>): a thread adds its two elements, t and t + 1024, before the wave_sum: one more
    level of the LayerNorm's tree; the rest as above."""
    wide = int(np.shape(x)[1] > 1024)
    y, dy = layernorm_budget(x, g, b, "fp32", eps, depth=wide + 6 + POOL_WAVES)
    w64 = np.asarray(proj, np.float64)
    o = y @ w64.T
    do = dy @ np.abs(w64).T + C_ACC * U32 * (np.abs(y) @ np.abs(w64).T)
    if not normalize:
        return o, do + 0.5 * ulp(o, "fp32")
    return l2_normalise_budget(o, do, math.ceil(w64.shape[0] / POOL_WAVES) + POOL_WAVES)


def bank_reduce_budget(feats, K: int, T: int):
    """(ref, budget) of bank_reduce_kernel (embed.hip): feats [K T, P] fp32, class-major.  a = (sum_t f_t) / T with the sum
    taken one term after another in fp32 (T - 1 roundings, each at most u32 of sum_t |f_t|) and one correctly rounded
    division; then the normalise term: a lane sums the squares of its ceil(P / 64) elements, then the 6-step butterfly."""
    f = np.asarray(feats, np.float64).reshape(K, T, -1)
    a = f.mean(axis=1)
    da = (T - 1) * U32 * np.abs(f).sum(axis=1) / T + U32 * np.abs(a)
    return l2_normalise_budget(a, da, math.ceil(f.shape[2] / 64) + 6)


def worst(got, ref, bud):
    """max |got - ref| / budget over the elements, and the flat index of the worst one (NaN in got counts as infinite)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    ratio = np.where(np.isinf(bud), 0.0, err / bud)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i
