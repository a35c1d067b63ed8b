"""Inputs, the fp64 reference and the error budget of the NegLabel score (neglabel.hip, mcm_neglabel_score_features): numpy only.

Definitions.  bank [N, P], N = K + G gs: rows [0, K) the ID prompts, rows [K + g gs, K + (g + 1) gs) negative group g.  With
s[b, n] the dot products and Td = (double) (float) T: logit = s / Td, LI = logsumexp(logit[:, :K]), LN[g] = logsumexp over group g,
S[b, g] = 1 / (1 + exp(LN[g] - LI)), scores[b] = -mean_g S[b, g].  The reference is fp64 from the fp32 inputs.

Inputs:
  * lattice_case: entries are integers in [-63, 63] times 2^-11, so every similarity is EXACT in fp32 in any summation order
    (tests/knn_budget.py); the result is then held to the arithmetic term plus one ulp alone;
  * unit_case: seeded unit rows; 20 queries are pulled, with graded strength, toward chosen bank rows (ID rows, the first row of
    group 0, the bank's last row, rows inside groups), so that S spans about 1e-4 ... 1 and a row counted into the wrong range, or
    not at all, moves a result by far more than the budget.

Budget of S[b, g] (and of the score, the mean of G of them) = similarity term + arithmetic term + one fp32 ulp of the result.

Similarity term.  eps[b] = gamma_P max_n sum_i |f_bi bank_ni|, gamma_P = P u32 / (1 - P u32), bounds the error of an fp32 dot product
of P single-rounded products in any order.  Log-sum-exp is 1-Lipschitz in the sup norm, so LN - LI moves by at most 2 eps / Td;
the logistic function is 1/4-Lipschitz, so S moves by at most eps[b] / (2 Td); the mean of G such values by no more.

Arithmetic term, from what the kernels do (u = 2^-53, u32 = 2^-24, X[b] = 2 max_n |s[b, n]| / Td >= every |(s - max) / Td|).
First launch, the pair (m, sum) of the rows of one range inside one split (at most `len` rows, len = K or gs):
  (a) m is a maximum of fp32 values: exact;
  (b) x = fl(fl((double) s - (double) m) * invT), invT = fl(1 / Td): three roundings, |dx| <= 3 u X;
  (c) exp is the fp64 library exp, stated at 1 ulp = 2 u: every term carries a relative error of at most 3 u X + 2 u;
  (d) the terms are non-negative and summed in fp64 (a lane's strided share, a 6-step butterfly, the carried sum): at most
      len - 1 additions deep in any order, relative error <= len u;
  (e) when a later segment raises the maximum the carried sum is multiplied by exp(fl(fl(m - M) * invT)): 3 u X + 3 u each time,
      at most len / 256 + 2 times (the segments of the range inside the split);
  (f) the sum is stored as fp32: relative u32.  (m is stored as it is.)
Second launch, per range over the at most 32 splits: M = max m exact; tot = sum_s (double) sum_s * exp(fl(fl(m_s - M) * invT)):
3 u X + 3 u per term and 31 u for the additions.  So tot carries a relative error of at most
      rel = u32 + u (len + (len / 256 + 4) (3 X + 3) + 31).
L = fl(fl(M * invT) + log(tot)): the product is off by at most u X (|M / Td| <= X / 2, two roundings), the fp64 log (1 ulp) by
rel + 2 u log(len) (1 <= tot <= len up to rounding), the sum by u |L| <= u (X / 2 + log(len)):
      dL(len) = u32 + u (len + (len / 256 + 4) (3 X + 3) + 31 + 1.5 X + 3 log(len)),
taken times (1 + 2^-20) for the second-order terms.  d = fl(LN - LI) is off by dL(gs) + dL(K) + u |d|; exp(d) within 2 u is a
shift of d by 2 u; 1 / (1 + E) adds two roundings of S <= 1:
      A_S[b, g] = (dL(gs) + dL(K) + u |d|) / 4 + 3 u.
The score is the mean of the S values as group_dev holds them, so that the two outputs agree: every S is rounded to fp32 first
(at most u32 |S| each, u32 times their mean in the mean), then a fp64 tree sum over G (relative G u), a division and a negation:
      A_score[b] = mean_g A_S + u32 mean_g |S| + (G + 1) u.
The fp32 rounding of either output is the "one ulp of the result" (taken at the far end of the interval); 2^-126 is added for
an S below the fp32 normal range.  There is no empirical margin."""
import numpy as np

from tests.knn_budget import LATTICE, U, bf16_round, eps_rows, similarities  # noqa: F401  (shared definitions)

U64 = 2.0 ** -53
TILE = 256
MAX_SPLITS = 32


def t_double(T):
    """The temperature the library divides by: the fp32 argument, widened."""
    return float(np.float32(T))


def lattice_case(B, K, G, gs, P, seed):
    """(f [B,P], bank [K + G gs, P]) fp32 on the lattice: every similarity exact in fp32."""
    assert P <= 1024
    rng = np.random.default_rng(seed)
    N = K + G * gs
    f = (rng.integers(-63, 64, size=(B, P)) * LATTICE).astype(np.float32)
    bank = (rng.integers(-63, 64, size=(N, P)) * LATTICE).astype(np.float32)
    s64 = similarities(f, bank)
    assert np.array_equal((f @ bank.T).astype(np.float64), s64), "lattice similarities must be exact in fp32"
    return f, bank


def planted_rows(K, G, gs):
    """The bank rows the first 20 queries of unit_case are pulled toward: on either side of every kind of boundary."""
    N = K + G * gs
    rows = [0, K - 1, K, N - 1, K + gs - 1, K + gs if G > 1 else K, K // 2, K + (G // 2) * gs + gs // 2, N - 2 if N > 1 else 0, 1 % K]
    return [min(max(r, 0), N - 1) for r in rows] * 2


def unit_case(B, K, G, gs, P, seed):
    """(f [B,P], bank [N,P]) fp32 rows of unit norm (to fp32 round-off).  Query i < min(20, B) is pulled toward bank row
    planted_rows()[i], the first ten strongly (cosine about 0.8), the second ten weakly (about 0.3)."""
    rng = np.random.default_rng(seed)
    N = K + G * gs
    bank = rng.standard_normal((N, P))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    f = rng.standard_normal((B, P))
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    for i, row in enumerate(planted_rows(K, G, gs)[:min(20, B)]):
        a = 0.8 if i < 10 else 0.3
        f[i] = a * bank[row] + np.sqrt(1.0 - a * a) * f[i]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32), bank.astype(np.float32)


def _lse(x):
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def reference_from_similarities(s64, K, G, gs, T):
    """(S [B,G], scores [B], d [B,G] = LN - LI) in fp64 from similarities [B, K + G gs]."""
    logit = np.asarray(s64, np.float64) / t_double(T)
    LI = _lse(logit[:, :K])
    LN = _lse(logit[:, K:K + G * gs].reshape(logit.shape[0], G, gs))
    d = LN - LI[:, None]
    with np.errstate(over="ignore"):
        S = 1.0 / (1.0 + np.exp(d))
    return S, -S.mean(axis=1), d


def reference(f, bank, K, G, gs, T):
    return reference_from_similarities(similarities(f, bank), K, G, gs, T)


def _dl(length, X):
    return (1.0 + 2.0 ** -20) * (U + U64 * (length + (length / TILE + 4.0) * (3.0 * X + 3.0) + (MAX_SPLITS - 1) + 1.5 * X
                                            + 3.0 * np.log(length)))


def budgets(f, bank, K, G, gs, T, exact=False):
    """(budget_S [B,G], budget_score [B]) around reference(): similarity term + arithmetic term + one fp32 ulp of the result.
    exact=True (lattice inputs: the similarities carry no error): without the similarity term."""
    return budgets_from_similarities(similarities(f, bank), 0.0 if exact else eps_rows(f, bank), K, G, gs, T)


def budgets_from_similarities(s64, eps, K, G, gs, T):
    """budgets() from the fp64 similarities [B, N] and eps [B] (eps_rows, or 0)."""
    S, score, d = reference_from_similarities(s64, K, G, gs, T)
    Td = t_double(T)
    X = 2.0 * np.abs(s64).max(axis=1) / Td
    sim = np.broadcast_to(np.asarray(eps, np.float64), X.shape) / (2.0 * Td)
    a_s = (_dl(gs, X)[:, None] + _dl(K, X)[:, None] + U64 * np.abs(d)) / 4.0 + 3.0 * U64
    a_score = a_s.mean(axis=1) + U * (np.abs(score) + sim + a_s.mean(axis=1)) + (G + 1) * U64
    tiny = float(np.finfo(np.float32).tiny)

    def with_ulp(ref, room):
        far = np.maximum(np.abs(ref) + room, tiny).astype(np.float32)
        far = np.where(far.astype(np.float64) < np.abs(ref) + room, np.nextafter(far, np.float32(np.inf)), far)
        return room + np.spacing(far).astype(np.float64) + tiny

    return with_ulp(S, sim[:, None] + a_s), with_ulp(score, sim + a_score)


def ratio(got, ref, budget):
    """max |got - ref| / budget; inf where got is not finite (the references here are)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return np.inf
    return float((np.abs(got - ref) / budget).max()) if got.size else 0.0


def restate_fp32(f, bank, K, G, gs, T, splits=1, *, sims=None, shift=0, drop_ragged=False, pooled=False, use_T=True):
    """What the two kernels compute, in numpy: fp32 similarities (numpy's fp32 matmul unless `sims` is given), the bank in
    `splits` ranges of ceil(N / splits) rows walked in tiles of 256, one (fp32 max, fp64 sum) pair per (split, range) folded
    segment by segment and stored as fp32, the combination and everything behind it in fp64.  Returns (scores [B] fp32,
    S [B,G] fp32).  The keyword switches are the deliberate mistakes of tests/test_neglabel_budget.py:
      shift        every boundary between ranges moved by `shift` rows;
      drop_ragged  a tile of fewer than 256 rows is skipped;
      pooled       one softmax over all negatives instead of the mean over the groups;
      use_T=False  the temperature taken as 1."""
    s = np.asarray(sims if sims is not None else np.asarray(f, np.float32) @ np.asarray(bank, np.float32).T, np.float32)
    B, N = s.shape[0], K + G * gs
    inv = 1.0 / (t_double(T) if use_T else 1.0)
    per = -(-N // splits)
    cuts = [0] + [min(N, K + g * gs + shift) for g in range(G)] + [N]
    if pooled:
        cuts = [0, K, N]

    def lse_of_range(lo, hi):
        pairs = []
        for sp in range(lo // per, (hi - 1) // per + 1):
            s_lo, s_hi = sp * per, min(N, (sp + 1) * per)
            m, acc, seen = np.full(B, -np.inf, np.float32), np.zeros(B), False
            for n0 in range(s_lo, s_hi, TILE):
                n1 = min(n0 + TILE, s_hi)
                a, e = max(lo, n0), min(hi, n1)
                if a >= e or (drop_ragged and n1 - n0 < TILE):
                    continue
                seg = s[:, a:e]
                M = np.maximum(m, seg.max(axis=1))
                with np.errstate(invalid="ignore"):
                    scale = np.where(m == M, 1.0, np.exp((m.astype(np.float64) - M.astype(np.float64)) * inv))
                acc = acc * scale + np.exp((seg.astype(np.float64) - M.astype(np.float64)[:, None]) * inv).sum(axis=1)
                m, seen = M, True
            if seen:
                pairs.append((m, acc.astype(np.float32)))
        if not pairs:                                         # (only a mistake can leave a range without rows)
            return np.full(B, -np.inf)
        M = np.max([p[0] for p in pairs], axis=0)
        tot = sum(p[1].astype(np.float64) * np.exp((p[0].astype(np.float64) - M.astype(np.float64)) * inv) for p in pairs)
        return M.astype(np.float64) * inv + np.log(tot)

    LI = lse_of_range(cuts[0], cuts[1])
    LN = np.stack([lse_of_range(cuts[i], cuts[i + 1]) for i in range(1, len(cuts) - 1)], axis=1)
    with np.errstate(over="ignore"):
        S = 1.0 / (1.0 + np.exp(LN - LI[:, None]))
    S = S.astype(np.float32).astype(np.float64)                  # the mean is taken over the values as they are written
    score = (-S.mean(axis=1)).astype(np.float32)
    if pooled:
        S = np.repeat(S, G, axis=1)
    return score, S.astype(np.float32)
