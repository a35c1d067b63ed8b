"""fp64 reference and error budget of bidirectional attention for one head of ANY width hd (pure numpy, no GPU): the per-head
functions of tests/error_budget.py and tests/online_softmax_budget.py called with scale = hd^-0.5, the slicing helpers for a
[rows, 3 heads hd] qkv and for split images whose heads straddle the 64-column blocks, and a numpy emulation of the
head_dim-80 streaming kernels (attention.hip attn_hd80_kernel / attn_hd80_f32_kernel) in their order.

Nothing inside the per-head budgets hard-codes 64: they take q, k, v of any width and the scale as an argument.  What a width
other than a power of four adds is the scale itself, which is then not a power of two:
  * the 16-bit and split kernels fold it with log2 e into one fp32 constant.  So does the 64-wide kernel (log2 e is irrational),
    and the base budget's 2 u32 (|s| + |m|) covers that constant, the product m SC and the fma;
  * the fp32 kernels multiply every logit by the scale before the softmax.  At 0.125 that product is exact; at 80^-0.5 the
    constant is rounded once (relative 2^-24: it multiplies s and m alike, so it acts on s - m, at most u32 (|s| + |m|) <=
    2 u32 max|s|) and each product s * scale is rounded once more (u32 |s|).
  Both are logit perturbations, carried through the softmax like the others, as (3 u32 max_j |s_j|) * sum_j p_j |v_j - ref|:
  SCALE_TERM below, added in every mode when the scale is not a power of two (in the 16-bit modes it is slack).
At hd = 64 (scale 0.125) the term is absent and the helpers return exactly what the existing modules return."""
from __future__ import annotations

import math

import numpy as np

from tests import error_budget as eb
from tests import online_softmax_budget as ob

KT = ob.KT                     # keys per streamed tile
LOG2E = 1.4426950408889634
SCALE_TERM = 3.0               # u32 max|s| per logit for a scale that is not a power of two (see the module docstring)


def scale_of(hd: int) -> float:
    return float(hd) ** -0.5


def _pow2(x: float) -> bool:
    return math.frexp(x)[0] == 0.5


# ---- budgets -----------------------------------------------------------------------------------------------------------
def attention_budget(q, k, v, out: str, hd=None, online=True):
    """(ref, budget) of one (sequence, head): q [rows, hd], k, v [L, hd] (the rounded operands), scale hd^-0.5, under
    online_softmax_budget's streaming budget (online=False: error_budget.attention_budget's whole-row budget)."""
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    hd = k64.shape[1] if hd is None else hd
    scale = scale_of(hd)
    L = k64.shape[0]
    refs, buds = [], []
    for r0 in range(0, q64.shape[0], ob.ROW_BLOCK):
        ref, bud, dev, pv, smax = ob._base_terms(q64[r0:r0 + ob.ROW_BLOCK], k64, v64, out, scale)
        if online:
            bud = bud + ob.online_terms(L, dev, pv, ref, smax)
        if not _pow2(scale):
            bud = bud + SCALE_TERM * eb.U32 * smax * dev
        refs.append(ref)
        buds.append(ob._finish(ref, bud, out))
    return np.concatenate(refs), np.concatenate(buds)


def attention_split_budget(qh, ql, kh, kl, vh, vl, hd=None):
    """(ref, budget) of one (sequence, head) of the streaming split kernel at head width hd: error_budget.attention_split_rows
    with scale hd^-0.5, the rescale terms, the scale term and the split of the stored output."""
    hd = np.shape(kh)[1] if hd is None else hd
    scale = scale_of(hd)
    L = np.shape(kh)[0]
    refs, buds = [], []
    for r0 in range(0, np.shape(qh)[0], ob.ROW_BLOCK):
        rb = slice(r0, r0 + ob.ROW_BLOCK)
        ref, bud, dev, pv, smax = eb.attention_split_rows(qh[rb], ql[rb], kh, kl, vh, vl, scale)
        bud = bud + ob.online_terms(L, dev, pv, ref, smax)
        if not _pow2(scale):
            bud = bud + SCALE_TERM * eb.U32 * smax * dev
        refs.append(ref)
        buds.append(bud + eb.split_repr(np.abs(ref) + bud))
    return np.concatenate(refs), np.concatenate(buds)


# ---- slicing -----------------------------------------------------------------------------------------------------------
def head_qkv(qkv, L, heads, hd, n, h):
    """(q, k, v), each [L, hd], of (sequence n, head h) of a [nseq L, 3 heads hd] qkv: head h at column h hd of q, k and v."""
    rows = np.asarray(qkv)[n * L:(n + 1) * L]
    D = heads * hd
    return tuple(rows[:, o + h * hd:o + (h + 1) * hd] for o in (0, D, 2 * D))


def head_out(out, L, heads, hd, n, h):
    return np.asarray(out)[n * L:(n + 1) * L, h * hd:(h + 1) * hd]


def split_col(c):
    """Element offset of logical column c in a split row (per 64 columns hi[64] then lo[64]); the lo element is 64 further
    (common.hpp split_col)."""
    c = np.asarray(c)
    return (c // 64) * 128 + c % 64


def split_head_parts(img, L, heads, hd, n, h):
    """(qh, ql, kh, kl, vh, vl), each [L, hd] float64, of (sequence n, head h) of a split qkv image [nseq L, 6 heads hd]
    (heads hd a multiple of 64).  The image is blocked over the WHOLE row, so a head whose hd is not a multiple of 64
    straddles blocks: every column goes through split_col on its own."""
    rows = np.asarray(img)[n * L:(n + 1) * L].astype(np.float64)
    D = heads * hd
    parts = []
    for o in (0, D, 2 * D):
        c = split_col(o + h * hd + np.arange(hd))
        parts += [rows[:, c], rows[:, c + 64]]
    return tuple(parts)


def split_head_parts_contiguous(img, L, heads, hd, n, h):
    """THE MISTAKE split_head_parts guards against: the map of a head that does not straddle (hi = hd consecutive elements
    from the head's first column, lo 64 further) applied to any head.  Right for hd = 64; at hd = 80 right for no head but
    the first 64 columns of those that start a block."""
    rows = np.asarray(img)[n * L:(n + 1) * L].astype(np.float64)
    D = heads * hd
    parts = []
    for o in (0, D, 2 * D):
        c = int(split_col(o + h * hd)) + np.arange(hd)
        parts += [rows[:, c], rows[:, c + 64]]
    return tuple(parts)


def split_head_out(out_img, L, heads, hd, n, h):
    """hi + lo [L, hd] float64 of (sequence n, head h) of a split output image [nseq L, 2 heads hd]."""
    rows = np.asarray(out_img)[n * L:(n + 1) * L].astype(np.float64)
    c = split_col(h * hd + np.arange(hd))
    return rows[:, c] + rows[:, c + 64]


def coherent_small_p_qkv(L, heads, hd, nseq=1):
    """error_budget.coherent_small_p_qkv with the head width as a parameter (that function writes 64 and 0.125 out): the
    input on which P split WITHOUT the 2^12 scale breaks the split budget.  Key 0 dominates every query (raw logits +2t for
    key 0, -2t for the others; t near 3.125 / scale, so that the gap after the scale is 12.5 as there), every other P is the
    same ~2^-18 and t is chosen on a grid of 1/64 so that the unscaled P's remainder after hi falls halfway between two
    points of fp16's subnormal grid.  V is 0 for key 0 and 1 elsewhere.  Returns the fp32 qkv [nseq L, 3 heads hd]."""
    D = heads * hd
    scale = scale_of(hd)
    SC = np.float32(scale * LOG2E)
    t0 = math.floor(3.125 / scale) - 1.0
    best = None
    for i in range(128):
        t = t0 + i / 64.0
        msc = np.float32(np.float64(2.0 * t) * np.float64(SC))
        arg = np.float32(np.float64(-2.0 * t) * np.float64(SC) - np.float64(msc))
        c = np.float32(np.exp2(np.float64(arg)))
        r = (np.float64(c) - np.float64(np.float16(c))) / 2.0 ** -24
        miss = abs(r - np.floor(r) - 0.5)
        if best is None or miss < best[0]:
            best = (miss, t)
    t = best[1]
    qkv = np.zeros((nseq * L, 3 * D), np.float32)
    for h in range(heads):
        qkv[:, h * hd] = 4.0
        qkv[:, D + h * hd] = -0.5 * t
        qkv[:, 2 * D + h * hd:2 * D + (h + 1) * hd] = 1.0
        for n in range(nseq):
            qkv[n * L, D + h * hd] = 0.5 * t
            qkv[n * L, 2 * D + h * hd:2 * D + (h + 1) * hd] = 0.0
    return qkv


# ---- the kernels' order in numpy -----------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, np.float32)


def emulate(q, k, v, mode: str, scale=None, dims=None, ql=None, kl=None, vl=None):
    """attn_hd80_kernel (mode bf16 / fp16 / split) or attn_hd80_f32_kernel (fp32) for one head in numpy: 64-key tiles, the
    running max, a = exp2((m - m') SC), P rounded to the operand format (split: after the 2^12 scale, hi + lo), the row sum
    over the rounded P, O accumulated in fp32 tile by tile, O / l.  q, k, v: [*, hd] operand values (split: the hi halves,
    ql / kl / vl the lo halves).  Returns the stored output as float64 (split: hi + lo).
    Planted mistakes: scale (e.g. 0.125 for hd 80), dims (the logits summed over the first `dims` dims only)."""
    hd = np.shape(k)[1]
    scale = scale_of(hd) if scale is None else scale
    dims = hd if dims is None else dims
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    if mode == "split":
        ql64, kl64, vl64 = (np.asarray(a, np.float64) for a in (ql, kl, vl))
    L = k64.shape[0]
    R = q64.shape[0]
    SC = np.float32(scale * LOG2E)
    m = np.full((R, 1), -np.inf, np.float32)
    l = np.zeros((R, 1), np.float32)
    O = np.zeros((R, hd), np.float32)
    for k0 in range(0, L, KT):
        kt, vt = k64[k0:k0 + KT, :], v64[k0:k0 + KT, :]
        if mode == "split":   # cross terms first, then the leading one (fp32 accumulation: fp64 here, rounded once)
            klt = kl64[k0:k0 + KT]
            s = _f32(q64[:, :dims] @ klt[:, :dims].T + ql64[:, :dims] @ kt[:, :dims].T + q64[:, :dims] @ kt[:, :dims].T)
        else:
            s = _f32(q64[:, :dims] @ kt[:, :dims].T)
        if mode == "fp32":
            s = _f32(s * np.float32(scale))
            mn = np.maximum(m, s.max(axis=1, keepdims=True))
            with np.errstate(invalid="ignore"):
                a = np.where(np.isinf(m), np.float32(0), np.exp(_f32(m - mn), dtype=np.float32))
            p = np.exp(_f32(s - mn), dtype=np.float32)
            l = _f32(l * a) + _f32(p.astype(np.float64).sum(axis=1, keepdims=True))
            O = _f32(_f32(O * a) + _f32(p.astype(np.float64) @ vt))
            m = mn
            continue
        mn = np.maximum(m, s.max(axis=1, keepdims=True))
        with np.errstate(invalid="ignore"):
            a = np.where(np.isinf(m), np.float32(0), np.exp2(_f32(_f32(m - mn) * SC), dtype=np.float32))
        msc = _f32(mn * SC) - (np.float32(12.0) if mode == "split" else np.float32(0.0))
        arg = _f32(s.astype(np.float64) * np.float64(SC) - msc.astype(np.float64))   # fmaf(s, SC, -msc)
        e = np.exp2(arg, dtype=np.float32)
        if mode == "split":
            ph, pl = eb.split2_f16(e)
            ph, pl = ph.astype(np.float64), pl.astype(np.float64)
            vlt = vl64[k0:k0 + KT]
            l = _f32(l * a) + _f32((ph + pl).sum(axis=1, keepdims=True))
            O = _f32(_f32(O * a) + _f32(ph @ vlt + pl @ vt + ph @ vt))
        else:
            p = eb.round_to(e, mode).astype(np.float64)
            l = _f32(l * a) + _f32(p.sum(axis=1, keepdims=True))
            O = _f32(_f32(O * a) + _f32(p @ vt))
        m = mn
    res = _f32(O * _f32(np.float32(1.0) / l))
    if mode == "fp32":
        return res.astype(np.float64)
    if mode == "split":
        hi, lo = eb.split2_f16(res)
        return hi.astype(np.float64) + lo.astype(np.float64)
    return eb.round_to(res, mode).astype(np.float64)
