"""Error budget of the streaming attention kernels (attention.hip attn_long_kernel / attn_long_f32_kernel, L = 289 ... 1025):
tests/error_budget.py's attention budget plus the terms of the online softmax (pure numpy, no GPU).

error_budget.attention_budget models a softmax taken against the row's final max.  The streaming kernels instead keep a
running max m per query and, at every 64-key tile whose max exceeds it, multiply O and the row sum l by a = exp(m_old - m_new).
What that adds, per rescale (at most one per tile, nt = ceil(L / 64) of them):
  * the factor a itself: its fp32 argument ((m_old - m_new) rounded, then times scale * log2 e in the 16-bit kernels: a
    relative error of 2 u32 |m_old - m_new| <= 4 u32 max_j |s_j|) and v_exp_f32 / expf (C_EXP u32).  O and l see the same a,
    but it multiplies only the tiles summed so far: its error moves the weights of the earlier tiles against the later
    ones, like a logit error of that size — carried through the softmax as sum_j p_j |v_j - ref|, the dsmax * dev term of the base budget;
  * the fp32 products O * a and l * a: one rounding of each, relative to the partial sums (<= sum_j p_j |v_j| and |ref|).
P is rounded against the running max, which is never above the final one: each P is at least as large relative to its
rounding grid as in the base model, so the base budget's P terms (and fp16's subnormal term) still bound it.

The base terms are computed here on row blocks (the [L, L, 64] temporary of error_budget.attention_budget is 538 MB at
L = 1025); tests/test_online_softmax_budget.py checks that they equal error_budget.attention_budget's to fp64 round-off."""
from __future__ import annotations

import math

import numpy as np

from tests import error_budget as eb

KT = 64          # keys per streamed tile (attention.hip LONG_KT)
ROW_BLOCK = 128  # query rows per block of the fp64 reference


def _base_terms(q64, k64, v64, out, scale):
    """error_budget.attention_budget's bidirectional terms for the query rows q64 against all keys (before the final
    output rounding).  Returns (ref, bud, dev, pv, smax)."""
    L = k64.shape[0]
    s = scale * (q64 @ k64.T)
    sa = scale * (np.abs(q64) @ np.abs(k64).T)
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    p = e / e.sum(axis=1, keepdims=True)
    ref = p @ v64
    pv = p @ np.abs(v64)
    dev = np.einsum("qj,qjd->qd", p, np.abs(v64[None, :, :] - ref[:, None, :]))
    sfin = np.abs(s)
    ds = eb.C_ACC * eb.U32 * sa + eb.U32 * (sfin + np.abs(m)) * 2.0 + eb.C_EXP * eb.U32
    dsmax = ds.max(axis=1, keepdims=True)
    uP = eb.U16.get(out, eb.U32)
    bud = (2.0 * uP * pv + dsmax * dev + eb.C_ACC * eb.U32 * pv
           + (math.ceil(L / 16) + 4) * eb.U32 * np.abs(ref) + 2.0 * eb.U32 * np.abs(ref))
    if out == "fp16":
        bud = bud + L * 2.0 ** -25 * np.abs(v64).max()
    return ref, bud, dev, pv, np.abs(s).max(axis=1, keepdims=True)


def _finish(ref, bud, out):
    """error_budget.attention_budget's last step: the rounding of the output to its format."""
    if out == "fp32":
        return bud + 0.5 * eb.ulp(ref, "fp32")
    return 0.5 * eb.ulp(np.abs(ref) + bud, out) + bud


def online_terms(L, dev, pv, ref, smax):
    """The rescale terms above for a row of L keys (nt = ceil(L / KT) rescales at most)."""
    nt = math.ceil(L / KT)
    rel_a = (eb.C_EXP + 2.0) * eb.U32 + 4.0 * eb.U32 * smax
    return nt * (rel_a * dev + eb.U32 * (pv + np.abs(ref)))


def online_attention_budget(q, k, v, out: str, scale=0.125, online=True):
    """(ref, budget) of one (sequence, head) of bidirectional attention: q, k, v [L, 64] (the rounded operands).
    online=False: error_budget.attention_budget's budget alone (to check the block computation against it)."""
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    L = k64.shape[0]
    refs, buds = [], []
    for r0 in range(0, q64.shape[0], ROW_BLOCK):
        ref, bud, dev, pv, smax = _base_terms(q64[r0:r0 + ROW_BLOCK], k64, v64, out, scale)
        if online:
            bud = bud + online_terms(L, dev, pv, ref, smax)
        refs.append(ref)
        buds.append(_finish(ref, bud, out))
    return np.concatenate(refs), np.concatenate(buds)


def online_attention_split_budget(qh, ql, kh, kl, vh, vl, scale=0.125):
    """(ref, budget) of one (sequence, head) of the streaming split kernel (attn_long_kernel<X2>): the split terms of
    error_budget.attention_split_rows, the rescale terms above, and the split of the stored output (error_budget.split_repr).
    P is split against the running max after the same 2^12 scale; relative to its final weight each P's subnormal floor is
    at most the whole-row model's (the running max is never above the final one)."""
    L = np.shape(kh)[0]
    refs, buds = [], []
    for r0 in range(0, np.shape(qh)[0], ROW_BLOCK):
        rb = slice(r0, r0 + ROW_BLOCK)
        ref, bud, dev, pv, smax = eb.attention_split_rows(qh[rb], ql[rb], kh, kl, vh, vl, scale)
        bud = bud + online_terms(L, dev, pv, ref, smax)
        refs.append(ref)
        buds.append(bud + eb.split_repr(np.abs(ref) + bud))
    return np.concatenate(refs), np.concatenate(buds)


def online_attention_qkv_budget(qkv, nseq, L, heads, out, pairs=None):
    """online_attention_budget over the (sequence, head) pairs of a [nseq * L, 3 * heads * 64] qkv (all pairs by default).
    Returns {(n, h): (ref [L, 64], budget [L, 64])}."""
    D = heads * 64
    res = {}
    for n, h in (pairs if pairs is not None else [(n, h) for n in range(nseq) for h in range(heads)]):
        rows = qkv[n * L:(n + 1) * L]
        res[(n, h)] = online_attention_budget(rows[:, h * 64:(h + 1) * 64], rows[:, D + h * 64:D + (h + 1) * 64],
                                              rows[:, 2 * D + h * 64:2 * D + (h + 1) * 64], out)
    return res
