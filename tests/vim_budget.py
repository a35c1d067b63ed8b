"""Inputs, the fp64 reference and the error budget of the ViM score (vim.hip, mcm_vim_score_features): numpy only.

Definitions.  bank [N, P], N = K + R: rows [0, K) the prompts, rows [K, K + R) the null-space basis.  With s[b, n] the dot
products, Td = (double) (float) T, off [R] fp64 (None = 0) and a = (double) (float) alpha:
    resid[b] = sqrt(sum_j (s[b, K + j] - off[j])^2)      lse[b] = logsumexp_k s[b, k] / Td      maxlogit[b] = max_k s[b, k] / Td
    score[b] = a resid[b] - lse[b].
The reference is fp64 from the fp32 inputs.

Inputs:
  * lattice_case: entries are integers in [-63, 63] times 2^-11, so every similarity is EXACT in fp32 in any summation order
    (tests/knn_budget.py); the result is then held to the arithmetic term plus one ulp alone.  The basis rows are lattice rows
    like the others (the kernel does not ask for an orthonormal basis);
  * unit_case: seeded unit rows.  The basis rows are unit rows too, except the first min(4, R), which are the standard basis
    vectors e_0 .. e_3; queries 0 and 1 are zero in those columns and, where R <= 4, lie exactly in the principal space: the
    reference's resid is exactly 0 and so must the kernel's be (every product is 0).  Queries 2 .. 11 are pulled toward one
    prompt row each (row 0, K - 1, K // 2, ...: cosine about 0.8, then 0.3), so that one logit dominates at T = 0.01 and a prompt
    counted as a basis row, dropped, or merged at the wrong scale moves a result by far more than the budget.

Budget = similarity term + arithmetic term + one fp32 ulp of the result, per output.  u = 2^-53, u32 = 2^-24.

Similarity term.  E[b, n] = gamma_P sum_i |f_bi bank_ni|, gamma_P = P u32 / (1 - P u32), bounds the error of an fp32 dot product of P
single-rounded products in any order (tests/knn_budget.py, per element here instead of per row).
  * resid: with v_j = s_j - off_j the kernel holds v'_j = fl(s'_j - off_j), |v'_j - v_j| <= E_j + u |v'_j| (s' widens exactly, the
    subtraction rounds once; no rounding at all without off).  The norm is 1-Lipschitz in the 2-norm — | |v'| - |v| | <= |v' - v| —
    so resid moves by at most |E[b, K:]|_2 + u resid (1 + ...): no first-order approximation is needed for this step;
  * lse: log-sum-exp is 1-Lipschitz in the sup norm: max_k E[b, k] / Td.  maxlogit: a maximum is too: the same.

Arithmetic term.
  * ssq = sum_j v'_j^2: every term is one fma (the square is not rounded on its own) onto a non-negative running sum; a term
    passes at most 4 (a lane's share of a 256-row tile) + 6 (the butterfly) + R / 256 + 2 (the tiles of a split, into the carried
    sum) + 31 (the splits, in the second launch) additions, each of relative error u: ssq is off by at most
    (R / 256 + 43) u relatively.  (A bound of one u per addition of non-negative terms holds for any association.)
    sqrt halves a relative error and rounds once:          A_resid = resid ((R / 256 + 43) / 2 + 2) u,
    taken times (1 + 2^-20) for the second-order terms;
  * lse: the pair (max, sum) per split and their combination are neglabel.hip's — the same functions, bank_sim::lse_fold /
    lse_merge — with one range of len = K rows: tests/neglabel_budget.py derives dL(len, X), X = 2 max_k |s[b, k]| / Td, for it (steps (a) - (f) there, the
    fp32 rounding of the stored sum included), and that function is used here as it stands:   A_lse = dL(K, X);
  * maxlogit = fl((double) M * fl(1 / Td)): two roundings of a value of at most X / 2:   A_max = 2 u |maxlogit|;
  * score = fl(fl(a resid') - lse'): |a| (E_resid + A_resid) + E_lse + A_lse + u (|a resid| + |score|), then rounded to fp32.
The fp32 rounding of an output is the "one ulp of the result" (taken at the far end of the interval); 2^-126 is added for a
result below the fp32 normal range.  There is no empirical margin."""
import numpy as np

from tests.knn_budget import LATTICE, U, similarities  # noqa: F401  (shared definitions)
from tests.neglabel_budget import MAX_SPLITS, TILE, U64, _dl, _lse, ratio, t_double  # noqa: F401

OUTPUTS = ("resid", "lse", "maxlogit", "score")


def a_double(alpha):
    """The scale the library multiplies by: the fp32 argument, widened."""
    return float(np.float32(alpha))


def lattice_case(B, K, R, P, seed):
    """(f [B,P], bank [K + R, P]) fp32 on the lattice: every similarity exact in fp32."""
    assert P <= 1024
    rng = np.random.default_rng(seed)
    f = (rng.integers(-63, 64, size=(B, P)) * LATTICE).astype(np.float32)
    bank = (rng.integers(-63, 64, size=(K + R, P)) * LATTICE).astype(np.float32)
    assert np.array_equal((f @ bank.T).astype(np.float64), similarities(f, bank)), "lattice similarities must be exact in fp32"
    return f, bank


def lattice_off(R, seed):
    """off [R] fp64 of the size of a lattice similarity, with all 53 bits in use."""
    return np.random.default_rng(seed).uniform(-0.02, 0.02, size=R)


def planted_prompts(K):
    rows = [0, K - 1, K // 2, 1 % K, max(K - 2, 0)]
    return rows * 2


def unit_case(B, K, R, P, seed):
    """(f [B,P], bank [K + R, P]) fp32 rows of unit norm (to fp32 round-off); see the module docstring for the planted rows."""
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal((K + R, P))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    ne = min(4, R, P)
    bank[K:K + ne] = np.eye(P)[:ne]
    f = rng.standard_normal((B, P))
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    for i, row in enumerate(planted_prompts(K)[:max(0, min(10, B - 2))]):
        a = 0.8 if i < 5 else 0.3
        f[2 + i] = a * bank[row] + np.sqrt(1.0 - a * a) * f[2 + i]
    if P > ne:
        f[:2, :ne] = 0.0
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32), bank.astype(np.float32)


def reference_from_similarities(s64, K, off, T, alpha):
    """{resid, lse, maxlogit, score} [B] in fp64 from similarities [B, K + R]."""
    s64 = np.asarray(s64, np.float64)
    v = s64[:, K:] - (0.0 if off is None else np.asarray(off, np.float64)[None, :])
    resid = np.sqrt((v * v).sum(axis=1))
    logit = s64[:, :K] / t_double(T)
    lse = _lse(logit)
    return {"resid": resid, "lse": lse, "maxlogit": logit.max(axis=1), "score": a_double(alpha) * resid - lse}


def reference(f, bank, K, off, T, alpha):
    return reference_from_similarities(similarities(f, bank), K, off, T, alpha)


def eps_elements(f, bank):
    """E[b, n]: the fp32 dot-product bound for any summation order, per element."""
    P = f.shape[1]
    gamma = P * U / (1.0 - P * U)
    return gamma * (np.abs(np.asarray(f, np.float64)) @ np.abs(np.asarray(bank, np.float64)).T)


def budgets(f, bank, K, off, T, alpha, exact=False):
    """{output: budget [B]} around reference(): similarity term + arithmetic term + one fp32 ulp of the result.
    exact=True (lattice inputs: the similarities carry no error): without the similarity term."""
    s64 = similarities(f, bank)
    return budgets_from_similarities(s64, np.zeros_like(s64) if exact else eps_elements(f, bank), K, off, T, alpha)


def budgets_from_similarities(s64, E, K, off, T, alpha, ulp=True):
    """budgets() from the fp64 similarities [B, N] and E [B, N] (eps_elements, or zeros).  ulp=False: the budget of the fp64
    values before they are rounded to fp32."""
    ref = reference_from_similarities(s64, K, off, T, alpha)
    R = s64.shape[1] - K
    Td, a = t_double(T), abs(a_double(alpha))
    two = 1.0 + 2.0 ** -20
    e_resid = np.sqrt((E[:, K:] ** 2).sum(axis=1)) + (0.0 if off is None else two * U64 * ref["resid"])
    a_resid = two * ref["resid"] * ((R / TILE + 43.0) / 2.0 + 2.0) * U64
    e_lse = E[:, :K].max(axis=1) / Td
    X = 2.0 * np.abs(s64[:, :K]).max(axis=1) / Td
    a_lse = _dl(K, X)
    a_max = 2.0 * U64 * np.abs(ref["maxlogit"])
    room = {"resid": e_resid + a_resid, "lse": e_lse + a_lse, "maxlogit": e_lse + a_max}
    room["score"] = a * room["resid"] + room["lse"] + two * U64 * (a * ref["resid"] + np.abs(ref["score"]))
    if not ulp:
        return room
    tiny = float(np.finfo(np.float32).tiny)

    def with_ulp(r, rm):
        far = np.maximum(np.abs(r) + rm, tiny).astype(np.float32)
        far = np.where(far.astype(np.float64) < np.abs(r) + rm, np.nextafter(far, np.float32(np.inf)), far)
        return rm + np.spacing(far).astype(np.float64) + tiny

    return {k: with_ulp(ref[k], room[k]) for k in OUTPUTS}


def worst_ratio(got, ref, budget):
    """max over the outputs of max |got - ref| / budget (inf where got is not finite)."""
    return max(ratio(got[k], ref[k], budget[k]) for k in OUTPUTS)


def restate_fp32(f, bank, K, off, T, alpha, splits=1, *, sims=None, ssq_fp32=False, ignore_off=False, shift=0, drop_ragged=False,
                 no_rescale=False, no_sqrt=False):
    """What the two kernels compute, in numpy: fp32 similarities (numpy's fp32 matmul unless `sims` is given), the bank in
    `splits` ranges of ceil(N / splits) rows walked in tiles of 256 that are cut at row K, one slot (fp32 max, fp64 exp-sum stored
    as fp32, fp64 sum of squares) per split, the combination in split order and everything behind it in fp64.  Returns
    {resid, lse, maxlogit, score} [B] fp32.  The keyword switches are the deliberate mistakes of tests/test_vim_budget.py:
      ssq_fp32     the sum of squares accumulated in fp32;
      ignore_off   off taken as 0;
      shift        the boundary between prompts and basis rows moved by `shift` rows (-1: the last prompt counted as a basis row);
      drop_ragged  a tile of fewer than 256 rows is skipped;
      no_rescale   the splits' exp-sums added as they are, not rescaled to the common max;
      no_sqrt      the sum of squares returned as resid."""
    s = np.asarray(sims if sims is not None else np.asarray(f, np.float32) @ np.asarray(bank, np.float32).T, np.float32)
    B, N = s.shape
    inv = 1.0 / t_double(T)
    per = -(-N // splits)
    cut = K + shift
    off_full = np.zeros(N)
    if off is not None and not ignore_off:
        off_full[K:] = np.asarray(off, np.float64)
    pairs, ssq_tot = [], (np.zeros(B, np.float32) if ssq_fp32 else np.zeros(B))
    for sp in range(splits):
        s_lo, s_hi = min(N, sp * per), min(N, (sp + 1) * per)
        m, acc, seen = np.full(B, -np.inf, np.float32), np.zeros(B), False
        ssq = np.zeros(B, np.float32) if ssq_fp32 else np.zeros(B)
        for n0 in range(s_lo, s_hi, TILE):
            n1 = min(n0 + TILE, s_hi)
            if drop_ragged and n1 - n0 < TILE:
                continue
            a, e = n0, min(cut, n1)
            if a < e:
                seg = s[:, a:e]
                M = np.maximum(m, seg.max(axis=1))
                with np.errstate(invalid="ignore"):
                    scale = np.where(m == M, 1.0, np.exp((m.astype(np.float64) - M.astype(np.float64)) * inv))
                acc = acc * scale + np.exp((seg.astype(np.float64) - M.astype(np.float64)[:, None]) * inv).sum(axis=1)
                m, seen = M, True
            a, e = max(cut, n0), n1
            if a < e:
                v = s[:, a:e].astype(np.float64) - off_full[None, a:e]
                if ssq_fp32:
                    v = v.astype(np.float32)
                    for j in range(v.shape[1]):                   # one rounding per addition, as a fp32 accumulator has
                        ssq = (ssq + v[:, j] * v[:, j]).astype(np.float32)
                else:
                    ssq = ssq + (v * v).sum(axis=1)
        if seen:
            pairs.append((m, acc.astype(np.float32)))
        ssq_tot = ssq_tot + ssq
    if pairs:
        M = np.max([p[0] for p in pairs], axis=0)
        with np.errstate(invalid="ignore"):
            tot = sum(p[1].astype(np.float64) * (1.0 if no_rescale else np.exp((p[0].astype(np.float64) - M.astype(np.float64)) * inv))
                      for p in pairs)
        maxlogit = M.astype(np.float64) * inv
        with np.errstate(divide="ignore"):
            lse = maxlogit + np.log(tot)
    else:                                                         # (only a mistake can leave the prompts without rows)
        maxlogit = lse = np.full(B, -np.inf)
    ssq_tot = ssq_tot.astype(np.float64)
    resid = ssq_tot if no_sqrt else np.sqrt(ssq_tot)
    score = a_double(alpha) * resid - lse
    return {"resid": resid.astype(np.float32), "lse": lse.astype(np.float32), "maxlogit": maxlogit.astype(np.float32),
            "score": score.astype(np.float32)}
