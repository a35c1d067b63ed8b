"""Inputs, the fp64 reference and the error budget of the streamed tail of the MCM family (score_stream.hip,
mcm_score_features_stream): numpy only.

Definitions.  bank [K, P], s[b, k] the dot products, Td = (double) (float) T, m = max_k s, x_k = (s_k - m) / Td <= 0,
    Z = sum exp(x)      W = sum x exp(x)      Q = sum exp(2 x)      p_k = exp(x_k) / Z  (the softmax)
    MCM = -1 / Z   max-logit = -m   energy = -Td (m / Td + log Z)   entropy = log Z - W / Z   var = -(Q / Z^2 - 1 / K) / K
    prob_i = p_i at the rows of the topk largest s (value descending, then row ascending; a NaN is never a candidate).
The reference is fp64 from the fp32 inputs.

Inputs:
  * lattice_case: tests/knn_budget.py's — entries are integers in [-63, 63] times 2^-11, so every similarity is EXACT in fp32 in
    any summation order, and bank rows K // 2 and K - 1 are bitwise copies of rows 0 and 1 (ties for the top-k order); the result
    is then held to the arithmetic term plus one ulp alone;
  * unit_case: seeded unit rows; queries 0 .. 9 are pulled toward one bank row each (row 0, K - 1, K // 2, ...: cosine about 0.8,
    then 0.3), so that at T = 0.01 one logit dominates and a row dropped, or merged at the wrong scale, moves a result by far
    more than the budget.

Budget = similarity term + arithmetic term + one fp32 ulp of the result, per output.  u = 2^-53, u32 = 2^-24.

Similarity term.  E[b, k] = gamma_P sum_i |f_bi bank_ki|, gamma_P = P u32 / (1 - P u32), bounds the error of an fp32 dot product of P
single-rounded products in any order (tests/knn_budget.py, per element as in tests/vim_budget.py).  With eps = max_k E[b, k] / Td
every logit moves by at most eps, so log p_k moves by at most 2 eps (the logit and the log-sum-exp, which is 1-Lipschitz in the
sup norm): p'_k = p_k r_k with exp(-2 eps) <= r_k <= exp(2 eps).  No first-order approximation below:
  * max-logit: a maximum is 1-Lipschitz in the sup norm: max_k E[b, k];
  * energy = -Td lse: Td eps = max_k E[b, k];
  * MCM = -max_k p_k: every p_k moves by at most the factor exp(2 eps), so does their maximum: |MCM| (exp(2 eps) - 1);
  * entropy H = -sum p log p.  With log p'_k = log p_k + eta_k, |eta_k| <= 2 eps:
        H' - H = -sum (p'_k - p_k) (log p_k + H) - sum p'_k eta_k          (sum (p'_k - p_k) = 0 lets the constant H in)
    and |p'_k - p_k| <= p_k (exp(2 eps) - 1), so |H' - H| <= (exp(2 eps) - 1) sum p_k |log p_k + H| + 2 eps;
  * var = -(sum p^2 - 1 / K) / K: sum p^2 moves by at most the factor exp(4 eps): (exp(4 eps) - 1) sum p^2 / K;
  * prob_i: p_i (exp(2 eps) - 1).

Arithmetic term, from what the kernels do (X[b] = 2 max_k |s[b, k]| / Td >= every |x|).  The pair (m, Z) is lse_fold's and
lse_merge's of tests/neglabel_budget.py with Z kept in fp64: steps (a) - (e) there give the relative error of the merged Z,
        rel_Z = u (K + (K / 256 + 4) (3 X + 3) + 31)
(K additions of non-negative terms in any association; every term's exp, every rescale by a = exp((m - m') / Td) in the fold —
at most K / 256 + 2 of them — and the one in the merge each cost at most (3 X + 3) u; 31 additions over the splits), and
dL(K, X) of that module (used as it stands: it also holds the u32 of a sum stored as fp32, which this kernel does not spend)
bounds the error of L = m / Td + log Z.  W and Q are counted the same way:
  * x = fl(fl(s - m) * fl(1 / Td)) has a RELATIVE error of 3 u (and so an absolute one of 3 u X, which is what exp sees);
  * a term of W is fma(x, e, .): e within (3 X + 2) u, x within 3 u, the fma u: (3 X + 6) u.  A rescale is W <- a fma(d, Z, W)
    with d = (m - m') / Td <= 0 within 3 u, a within (3 X + 2) u, two roundings: (3 X + 7) u; the merge's is the same.  Every
    term of W, d Z included, is non-positive (x <= 0, d <= 0, Z >= 0), so relative errors add along a term's path:
        rel_W = u (K + (K / 256 + 4) (3 X + 8) + 31);
  * a term of Q is fma(e, e, .): 2 (3 X + 2) u + u; a rescale by a a: 2 (3 X + 2) u + 2 u:
        rel_Q = u (K + (K / 256 + 4) (6 X + 6) + 31).
The outputs, all formed in fp64 and rounded once to fp32:
  * MCM = -fl(1 / Z):                                A = |MCM| (rel_Z + 2 u);
  * max-logit = -m: a maximum of fp32 values:        A = 0;
  * energy = -fl(Td L):                              A = Td dL(K, X) + 2 u |energy|;
  * entropy = fl(log Z - fl(W / Z)): log Z (a 1 ulp log of a value in [1, K]) within rel_Z + 2 u (log K + 1), W / Z within
    |W / Z| (rel_W + rel_Z + 2 u), the subtraction u |H|:
                                                     A = rel_Z + 2 u (log K + 1) + |W / Z| (rel_W + rel_Z + 2 u) + 2 u |H|;
  * var = -fl(fl(fl(Q / fl(Z Z)) - fl(1 / K)) / K).  It CANCELS: Q / Z^2 = sum p^2 >= 1 / K with equality at the uniform softmax,
    so its budget is absolute — (rel_Q + 2 rel_Z + 4 u) of Q / Z^2, not of the difference — and 2 u / K, divided by K:
                                                     A = ((rel_Q + 2 rel_Z + 4 u) Q / Z^2 + 2 u / K) / K;
  * prob_i = fl(exp(x_i) / Z):                       A = p_i ((3 X + 2) u + rel_Z + 2 u),
each taken times (1 + 2^-20) for the second-order terms.  The fp32 rounding of an output is the "one ulp of the result" (taken at
the far end of the interval); 2^-126 is added for a result below the fp32 normal range.  There is no empirical margin."""
import numpy as np

from tests.knn_budget import LATTICE, U, lattice_case, similarities  # noqa: F401  (shared definitions)
from tests.neglabel_budget import MAX_SPLITS, TILE, U64, _dl, ratio, t_double  # noqa: F401
from tests.vim_budget import eps_elements, planted_prompts  # noqa: F401

KINDS = ("MCM", "max-logit", "energy", "entropy", "var")   # mcm_amd.config.SCORE_KINDS order: the columns of parts
TOPK_MAX = 8


def unit_case(B, K, P, seed):
    """(f [B,P], bank [K,P]) fp32 rows of unit norm (to fp32 round-off); see the module docstring for the planted rows."""
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal((K, P))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    f = rng.standard_normal((B, P))
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    for i, row in enumerate(planted_prompts(K)[:min(10, B)]):
        a = 0.8 if i < 5 else 0.3
        f[i] = a * bank[row] + np.sqrt(1.0 - a * a) * f[i]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32), bank.astype(np.float32)


def _moments(s64, T):
    s64 = np.asarray(s64, np.float64)
    Td = t_double(T)
    m = s64.max(axis=1)
    x = (s64 - m[:, None]) / Td
    e = np.exp(x)
    return Td, m, x, e, e.sum(axis=1), (x * e).sum(axis=1), (e * e).sum(axis=1)


def reference_from_similarities(s64, T):
    """{kind: [B]} in fp64 from similarities [B, K]."""
    Td, m, _x, _e, Z, W, Q = _moments(s64, T)
    K = np.asarray(s64).shape[1]
    return {"MCM": -1.0 / Z, "max-logit": -m, "energy": -Td * (m / Td + np.log(Z)), "entropy": np.log(Z) - W / Z,
            "var": -(Q / (Z * Z) - 1.0 / K) / K}


def reference(f, bank, T):
    return reference_from_similarities(similarities(f, bank), T)


def topk_reference(s64, T, topk):
    """(idx [B,topk] int64, prob [B,topk] fp64): numpy.argsort(-s, kind="stable") of the fp64 similarities with a NaN never a
    candidate; -1 / NaN where nothing is left.  prob is the softmax over the whole row (NaN for a row that holds a NaN)."""
    s64 = np.asarray(s64, np.float64)
    B, K = s64.shape
    order = np.argsort(-s64, axis=1, kind="stable")[:, :topk]             # NaN sorts last
    idx = np.full((B, topk), -1, np.int64)
    idx[:, :order.shape[1]] = order
    took = np.take_along_axis(s64, np.maximum(idx, 0), axis=1)
    idx[(idx < 0) | np.isnan(took)] = -1
    with np.errstate(invalid="ignore"):
        Td = t_double(T)
        m = np.fmax.reduce(s64, axis=1)
        e = np.exp((s64 - m[:, None]) / Td)
        p = e / e.sum(axis=1, keepdims=True)
    prob = np.where(idx >= 0, np.take_along_axis(p, np.maximum(idx, 0), axis=1), np.nan)
    return idx, prob


def _with_ulp(ref, room):
    tiny = float(np.finfo(np.float32).tiny)
    far = np.maximum(np.abs(ref) + room, tiny).astype(np.float32)
    far = np.where(far.astype(np.float64) < np.abs(ref) + room, np.nextafter(far, np.float32(np.inf)), far)
    return room + np.spacing(far).astype(np.float64) + tiny


def budgets_from_similarities(s64, E, T, ulp=True, prob_idx=None):
    """{kind: budget [B]} around reference_from_similarities() from the fp64 similarities [B, K] and E [B, K] (eps_elements, or
    zeros).  ulp=False: the budget of the fp64 values before they are rounded to fp32.  prob_idx [B, topk] (rows, -1 = none):
    also "prob" [B, topk], around topk_reference()'s."""
    s64 = np.asarray(s64, np.float64)
    K = s64.shape[1]
    Td, m, x, e, Z, W, Q = _moments(s64, T)
    ref = reference_from_similarities(s64, T)
    two = 1.0 + 2.0 ** -20
    p = e / Z[:, None]
    logp = x - np.log(Z)[:, None]
    Emax = np.asarray(E, np.float64).max(axis=1)
    eps = Emax / Td
    g2, g4 = np.expm1(2.0 * eps), np.expm1(4.0 * eps)
    sum_p2 = Q / (Z * Z)
    sim = {"MCM": np.abs(ref["MCM"]) * g2, "max-logit": Emax, "energy": Emax,
           "entropy": g2 * (p * np.abs(logp + ref["entropy"][:, None])).sum(axis=1) + 2.0 * eps, "var": g4 * sum_p2 / K}
    X = 2.0 * np.abs(s64).max(axis=1) / Td
    tiles = K / TILE + 4.0
    rel_z = U64 * (K + tiles * (3.0 * X + 3.0) + (MAX_SPLITS - 1))
    rel_w = U64 * (K + tiles * (3.0 * X + 8.0) + (MAX_SPLITS - 1))
    rel_q = U64 * (K + tiles * (6.0 * X + 6.0) + (MAX_SPLITS - 1))
    arith = {"MCM": np.abs(ref["MCM"]) * (rel_z + 2.0 * U64), "max-logit": np.zeros_like(Z),
             "energy": Td * _dl(K, X) + 2.0 * U64 * np.abs(ref["energy"]),
             "entropy": (rel_z + 2.0 * U64 * (np.log(K) + 1.0) + np.abs(W / Z) * (rel_w + rel_z + 2.0 * U64)
                         + 2.0 * U64 * np.abs(ref["entropy"])),
             "var": ((rel_q + 2.0 * rel_z + 4.0 * U64) * sum_p2 + 2.0 * U64 / K) / K}
    room = {k: sim[k] + two * arith[k] for k in KINDS}
    out = {k: _with_ulp(ref[k], room[k]) for k in KINDS} if ulp else room
    if prob_idx is not None:
        ix = np.asarray(prob_idx, np.int64)
        pi = np.where(ix >= 0, np.take_along_axis(p, np.maximum(ix, 0), axis=1), 0.0)
        rm = pi * (g2[:, None] + two * ((3.0 * X + 2.0) * U64 + rel_z + 2.0 * U64)[:, None])
        out["prob"] = _with_ulp(pi, rm) if ulp else rm
    return out


def budgets(f, bank, T, exact=False, prob_idx=None):
    """budgets_from_similarities() of f, bank.  exact=True (lattice inputs: the similarities carry no error): without the
    similarity term."""
    s64 = similarities(f, bank)
    return budgets_from_similarities(s64, np.zeros_like(s64) if exact else eps_elements(f, bank), T, prob_idx=prob_idx)


def worst_ratio(got, ref, budget):
    """(max over the kinds of max |got - ref| / budget, the kind it is reached at); inf where got is not finite."""
    r = {k: ratio(got[k], ref[k], budget[k]) for k in KINDS}
    k = max(r, key=r.get)
    return r[k], k


def prob_ratio(got_prob, ref_prob, budget_prob):
    """max |got - ref| / budget over the slots that hold a candidate; the others must be NaN in both (inf otherwise)."""
    got, ref = np.asarray(got_prob, np.float64), np.asarray(ref_prob, np.float64)
    have = ~np.isnan(ref)
    if got.shape != ref.shape or not np.isnan(got[~have]).all() or not np.isfinite(got[have]).all():
        return np.inf
    return float((np.abs(got[have] - ref[have]) / np.asarray(budget_prob)[have]).max()) if have.any() else 0.0


def _best(vals, rows, topk, tie_high):
    """The topk best (value, row) pairs of every row of vals [B, n] with bank rows `rows` [n] (ascending), in the selection
    order: value descending, then row ascending (tie_high: descending); NaN never; (NaN, -1) where nothing is left."""
    B, n = vals.shape
    if tie_high:
        vals, rows = vals[:, ::-1], rows[::-1]
    order = np.argsort(-vals, axis=1, kind="stable")[:, :topk]
    v = np.full((B, topk), np.nan, np.float32)
    i = np.full((B, topk), -1, np.int64)
    v[:, :order.shape[1]] = np.take_along_axis(vals, order, axis=1)
    i[:, :order.shape[1]] = rows[order]
    i[np.isnan(v)] = -1
    return v, i


def restate_fp32(f, bank, T, splits=1, topk=0, *, sims=None, w_no_dz=False, q_scale_a=False, var_split_rows=False,
                 drop_ragged=False, no_rescale=False, tie_high=False):
    """What the two kernels compute, in numpy: fp32 similarities (numpy's fp32 matmul unless `sims` is given), the bank in
    `splits` ranges of ceil(K / splits) rows walked in tiles of 256, one slot (fp32 max; Z, W, Q in fp64) and one list of the
    topk best (value, row) pairs per split that holds rows, the merge in split order and everything behind it in fp64.
    Returns {kind: [B] fp32} and, with topk > 0, "idx" [B,topk] int64 and "prob" [B,topk] fp32.  The keyword switches are the
    deliberate mistakes of tests/test_score_stream_budget.py:
      w_no_dz         a rising maximum rescales W by a alone, without the (m - m') / Td Z term (fold and merge);
      q_scale_a       ... and Q by a instead of a^2;
      var_split_rows  var divided by the rows the first split saw instead of K;
      drop_ragged     a tile of fewer than 256 rows is skipped;
      no_rescale      the splits' sums added as they are, not rescaled to the common maximum;
      tie_high        between equal similarities the higher row is taken."""
    s = np.asarray(sims if sims is not None else np.asarray(f, np.float32) @ np.asarray(bank, np.float32).T, np.float32)
    B, K = s.shape
    Td = t_double(T)
    inv = 1.0 / Td
    per = -(-K // splits)

    def rescaled(m_old, m_new, Z, W, Q):
        """(Z, W, Q) at the maximum m_old brought to m_new >= m_old (fp32 arrays); nothing moves where they are equal."""
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.where(m_old == m_new, 0.0, (m_old.astype(np.float64) - m_new.astype(np.float64)) * inv)
            d = np.where(np.isneginf(m_old), 0.0, d)                     # nothing folded yet: the sums are 0
            a = np.exp(d)
            return a * Z, a * (W + (0.0 if w_no_dz else d * Z)), (a if q_scale_a else a * a) * Q

    slots, lists = [], []
    for sp in range(splits):
        lo, hi = min(K, sp * per), min(K, (sp + 1) * per)
        if lo == hi:
            continue
        m, Z, W, Q = np.full(B, -np.inf, np.float32), np.zeros(B), np.zeros(B), np.zeros(B)
        cv = np.full((B, max(topk, 1)), np.nan, np.float32)
        ci = np.full((B, max(topk, 1)), -1, np.int64)
        for n0 in range(lo, hi, TILE):
            n1 = min(n0 + TILE, hi)
            if drop_ragged and n1 - n0 < TILE:
                continue
            seg = s[:, n0:n1]
            M = np.fmax(m, np.fmax.reduce(seg, axis=1))
            Z, W, Q = rescaled(m, M, Z, W, Q)
            with np.errstate(invalid="ignore"):
                x = (seg.astype(np.float64) - M.astype(np.float64)[:, None]) * inv
            e = np.exp(x)
            Z, W, Q, m = Z + e.sum(axis=1), W + (x * e).sum(axis=1), Q + (e * e).sum(axis=1), M
            if topk:   # the old list's rows lie below the tile's: old entries first keeps "row ascending" under a stable sort
                vals = np.concatenate([cv, seg], axis=1)
                rows = np.arange(n0, n1)
                v2 = np.full((B, topk), np.nan, np.float32)
                i2 = np.full((B, topk), -1, np.int64)
                for b in range(B):
                    r_b = np.concatenate([ci[b], rows])
                    have = r_b >= 0
                    v_b, i_b = _best(vals[b:b + 1, have], r_b[have], topk, tie_high)
                    v2[b], i2[b] = v_b[0], i_b[0]
                cv, ci = v2, i2
        slots.append((m, Z, W, Q, hi - lo))
        lists.append((cv, ci))
    if not slots:                                                       # (only a mistake can leave the bank without rows)
        nan = np.full(B, np.nan, np.float32)
        return {k: nan for k in KINDS}
    M = np.fmax.reduce([sl[0] for sl in slots], axis=0)
    Z, W, Q = np.zeros(B), np.zeros(B), np.zeros(B)
    for m_s, z_s, w_s, q_s, _n in slots:
        z_s, w_s, q_s = (z_s, w_s, q_s) if no_rescale else rescaled(m_s, M, z_s, w_s, q_s)
        Z, W, Q = Z + z_s, W + w_s, Q + q_s
    Kv = slots[0][4] if var_split_rows else K
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"MCM": -(1.0 / Z), "max-logit": np.where(np.isnan(Z), np.nan, -M.astype(np.float64)),
               "energy": -(Td * (M.astype(np.float64) * inv + np.log(Z))), "entropy": np.log(Z) - W / Z,
               "var": -((Q / (Z * Z) - 1.0 / Kv) / Kv)}
    out = {k: v.astype(np.float32) for k, v in out.items()}
    if topk:
        idx = np.full((B, topk), -1, np.int64)
        prob = np.full((B, topk), np.nan, np.float32)
        for b in range(B):
            v_all = np.concatenate([l[0][b] for l in lists])
            i_all = np.concatenate([l[1][b] for l in lists])
            have = i_all >= 0
            v_b, i_b = _best(v_all[None, have], i_all[have], topk, tie_high)
            idx[b] = i_b[0]
            with np.errstate(invalid="ignore"):
                pr = np.exp((v_b[0].astype(np.float64) - float(M[b])) * inv) / Z[b]
            prob[b] = np.where(i_b[0] >= 0, pr, np.nan).astype(np.float32)
        out["idx"], out["prob"] = idx, prob
    return out
