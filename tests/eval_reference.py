"""Exact reference for the evaluation tail: AUROC / AUPR / FPR@recall from integer counts (pure numpy + Python integers).

Independent of mcm_amd/metrics.py (no sklearn, no cumulative sums over a stable argsort) and of metrics.hip's formulation (no
per-example tp / fp / gt counts, no `2 n_neg - fp - gt`): the scores are sorted once, every count is a rank difference
(numpy.searchsorted on the sorted fp32 values, int64), and the three numbers are

  AUROC  U2 / (2 n_pos n_neg) with U2 = sum over positives p of (#{neg < p} + #{neg <= p}), a Python integer; one correctly
         rounded division (Python's int / int), which is what one fp64 division of the exactly represented integers gives;
  FPR    fp(t) / n_neg at the threshold t the reference's rule picks (utils/detection_util.py:100-106): among the distinct
         score values t >= min(pos), the smallest |tp(t) / n_pos - level|, the difference taken in fp64 as numpy takes it
         there, ties to the LOWEST t; again one division of exact integers;
  AUPR   sum over distinct thresholds, highest first, of (tp(t) - tp(previous)) / n_pos * tp(t) / (tp(t) + fp(t)), the terms
         in fp64 and their sum by math.fsum (correctly rounded).

tp(t) = #{pos >= t}, fp(t) = #{neg >= t}.  Comparisons are IEEE comparisons of the fp32 values: -inf and +inf are ordinary
ordered values, -0.0 == +0.0, subnormals are distinct numbers.  A NaN anywhere has no place in the order: all three outputs
are NaN (the contract of mcm_measures, include/mcm.h).

`measures_bruteforce` states the same counts by O(N^2) broadcasting, for small inputs; tests/test_eval_reference.py holds the
two to each other, to tests/golden/measures.npz and to mcm_amd.metrics.get_measures.
"""
from __future__ import annotations

import math

import numpy as np

U64 = 2.0 ** -53   # unit roundoff of fp64

# AUPR on the device (metrics.hip measures_kernel) is ap / n_pos with ap an fp64 sum of the n_pos terms tp_i / (tp_i + fp_i),
# each in (0, 1].  Worst case over every summation order: a term's division rounds once (<= U64 absolute), each of the
# n_pos - 1 additions rounds a partial sum that is at most n_pos (<= U64 n_pos each), the final division rounds once: after
# the division by n_pos that is at most (1 + (n_pos - 1) + 1) U64 = (n_pos + 1) U64.  The reference's own error: the two
# divisions and the product of each term (<= 3 U64 of a sum that is at most 1) and fsum's single rounding: <= 4 U64.  Together
# (n_pos + 5) U64, and at n_pos = 1 (no addition, a division by one) 2 U64: at most 4 n_pos U64 for every n_pos >= 1.
C_AUPR = 4.0


def aupr_bound(n_pos: int) -> float:
    """Bound on |device AUPR - measures_exact AUPR|: C_AUPR * n_pos * 2^-53 (derivation at C_AUPR)."""
    return C_AUPR * n_pos * U64


def _f32(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.float32:
        a = a.astype(np.float32)
    return a.reshape(-1)


def _pick(ts, tp, fp, n_pos, level, highest=False):
    """Index of the operating point the rule picks among thresholds ts (ascending) with counts tp, fp (Python ints)."""
    best, bd = None, None
    for i in range(len(ts)):           # ascending thresholds: a strict `<` keeps the lowest of a tie
        d = abs(tp[i] / n_pos - level)
        if bd is None or d < bd or (highest and d == bd):
            best, bd = i, d
    return best


def measures_exact(pos, neg, level: float = 0.95, _highest_tie=False):
    """(auroc, aupr, fpr) of ID scores `pos` (the positive class) against OOD scores `neg`, as module docstring."""
    pos, neg = _f32(pos), _f32(neg)
    n_pos, n_neg = int(pos.size), int(neg.size)
    if n_pos == 0 or n_neg == 0:
        raise ValueError("both score vectors must be non-empty")
    if np.isnan(pos).any() or np.isnan(neg).any():
        return math.nan, math.nan, math.nan
    ps, ns = np.sort(pos), np.sort(neg)
    # AUROC: pairs (p, n) with n < p count 2, n == p count 1
    below = np.searchsorted(ns, ps, side="left").astype(np.int64)
    upto = np.searchsorted(ns, ps, side="right").astype(np.int64)
    u2 = sum(int(v) for v in below) + sum(int(v) for v in upto)
    auroc = u2 / (2 * n_pos * n_neg)
    # one operating point per distinct value (-0.0 and +0.0 are one value: numpy.unique compares with ==)
    ts = np.unique(np.concatenate([ps, ns]))
    tp = [n_pos - int(v) for v in np.searchsorted(ps, ts, side="left")]
    fp = [n_neg - int(v) for v in np.searchsorted(ns, ts, side="left")]
    # AUPR: highest threshold first
    terms, prev = [], 0
    for i in range(len(ts) - 1, -1, -1):
        if tp[i] > prev:
            terms.append((tp[i] - prev) / n_pos * (tp[i] / (tp[i] + fp[i])))
            prev = tp[i]
    aupr = math.fsum(terms)
    # FPR: thresholds >= min(pos)
    first = int(np.searchsorted(ts, ps[0], side="left"))
    j = first + _pick(ts[first:], tp[first:], fp[first:], n_pos, level, highest=_highest_tie)
    return auroc, aupr, fp[j] / n_neg


def measures_bruteforce(pos, neg, level: float = 0.95):
    """The same three numbers from O(N^2) broadcast comparisons (small inputs only)."""
    pos, neg = _f32(pos), _f32(neg)
    n_pos, n_neg = int(pos.size), int(neg.size)
    if np.isnan(pos).any() or np.isnan(neg).any():
        return math.nan, math.nan, math.nan
    lt = int((neg[None, :] < pos[:, None]).sum(dtype=np.int64))
    eq = int((neg[None, :] == pos[:, None]).sum(dtype=np.int64))
    auroc = (2 * lt + eq) / (2 * n_pos * n_neg)
    ts = sorted(set(float(v) for v in np.concatenate([pos, neg])), reverse=True)   # set(): 0.0 == -0.0 hash alike
    terms, prev, cands = [], 0, []
    lo = float(pos.min())
    for t in ts:
        tp = int((pos >= np.float32(t)).sum())
        fp = int((neg >= np.float32(t)).sum())
        if tp > prev:
            terms.append((tp - prev) / n_pos * (tp / (tp + fp)))
            prev = tp
        if t >= lo:
            cands.append((abs(tp / n_pos - level), t, fp))
    d, t, fp = min(cands)              # smallest distance, then lowest threshold
    return auroc, math.fsum(terms), fp / n_neg


# ---- a numpy emulation of metrics.hip's counting, with the mistakes a kernel could make --------------------------------------
TILE = 4096   # metrics.hip: comparison values staged per LDS tile


def kernel_emulation(pos, neg, level: float = 0.95, mistake: str | None = None):
    """count_kernel + measures_kernel in numpy (O(N^2)), the per-example counts in uint32 and the Mann-Whitney numerator in
    uint64 as on the device.  mistake:
      None          the kernel as it should be
      "strict"      `>` where tp / fp need `>=`
      "ties_whole"  a tied (pos, neg) pair counted as a whole win, not half
      "inf_pad"     the tail of each 4096-value tile padded with -inf and compared like a score
      "highest"     the |recall - level| tie resolved to the highest threshold"""
    pos, neg = _f32(pos), _f32(neg)
    n_pos, n_neg = pos.size, neg.size
    ex = np.concatenate([pos, neg])
    ge = (lambda a, s: a[None, :] > s[:, None]) if mistake == "strict" else (lambda a, s: a[None, :] >= s[:, None])
    tp = ge(pos, ex).sum(axis=1).astype(np.uint32)
    fp = ge(neg, ex).sum(axis=1).astype(np.uint32)
    gt = (neg[None, :] > ex[:, None]).sum(axis=1).astype(np.uint32)
    if mistake == "inf_pad":           # every pad is >= a -inf score (and never > it)
        hit = (ex == -np.inf).astype(np.uint32)
        tp = tp + hit * np.uint32(-n_pos % TILE)
        fp = fp + hit * np.uint32(-n_neg % TILE)
    if mistake == "ties_whole":
        u2 = (np.uint64(2 * n_neg) - np.uint64(2) * gt[:n_pos].astype(np.uint64)).sum(dtype=np.uint64)
    else:
        with np.errstate(over="ignore"):
            u2 = (np.uint64(2 * n_neg) - fp[:n_pos].astype(np.uint64) - gt[:n_pos].astype(np.uint64)).sum(dtype=np.uint64)
    auroc = float(u2) / (2.0 * n_pos * n_neg)
    tpd, fpd = tp.astype(np.float64), fp.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        aupr = float((tpd[:n_pos] / (tpd[:n_pos] + fpd[:n_pos])).sum()) / n_pos
    cand = np.flatnonzero(ex >= pos.min())
    d = np.abs(tpd[cand] / n_pos - level)
    tie = cand[d == d.min()]
    t = ex[tie].max() if mistake == "highest" else ex[tie].min()
    pick = int(fp[ex == t].max())
    return auroc, aupr, pick / n_neg


def agrees(got, want, n_pos: int) -> bool:
    """The GPU tests' criterion: AUROC and FPR bit-equal, AUPR within aupr_bound."""
    return got[0] == want[0] and got[2] == want[2] and abs(got[1] - want[1]) <= aupr_bound(n_pos)
