"""Inputs, references and the error model of the k-nearest-neighbour score (knn.hip, mcm_knn_score_features): numpy only.

Two kinds of input:
  * lattice_case: entries are integers in [-63, 63] times 2^-11.  A product is an integer multiple of 2^-22 of at most 3969
    units and a partial sum of at most P <= 1024 of them stays below 2^24 units, so every similarity is EXACT in fp32 in any
    summation order: a kernel's lists must equal the fp64 reference's value for value (checked here: numpy fp32 == fp64);
  * unit_case: seeded unit rows.  eps[b] = gamma_P max_n sum_i |f_bi bank_ni| with gamma_P = P u / (1 - P u), u = 2^-24, bounds
    the error of an fp32 dot product of P single-rounded products in any order.  Order statistics are 1-Lipschitz in the sup
    norm (the k-th largest of a vector moves by at most the largest move of an entry), so every slot of the sorted top-k list
    may differ from the fp64 reference's by at most eps[b], with no assumption on how the values are separated; the score may
    lie anywhere in the image of [v_k - eps, v_k + eps] under v -> sqrt(max(0, 2 - 2 v)), plus one fp32 ulp for its rounding."""
import numpy as np

U = 2.0 ** -24
LATTICE = 2.0 ** -11


def lattice_case(B, N, P, seed):
    """(f [B,P], bank [N,P]) fp32 on the lattice; bank rows N // 2 and N - 1 are bitwise copies of rows 0 and 1 (N >= 4)."""
    assert P <= 1024
    rng = np.random.default_rng(seed)
    f = (rng.integers(-63, 64, size=(B, P)) * LATTICE).astype(np.float32)
    bank = (rng.integers(-63, 64, size=(N, P)) * LATTICE).astype(np.float32)
    if N >= 4:
        bank[N // 2] = bank[0]
        bank[N - 1] = bank[1]
    s64 = f.astype(np.float64) @ bank.astype(np.float64).T
    s32 = f @ bank.T
    assert np.array_equal(s32.astype(np.float64), s64), "lattice similarities must be exact in fp32"
    assert np.abs(s64).max() <= 0.05
    return f, bank


def unit_case(B, N, P, seed):
    """(f [B,P], bank [N,P]) fp32 rows of unit norm (to fp32 round-off); every query has close neighbours in the bank."""
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal((N, P))
    f = bank[rng.integers(0, N, size=B)] + 0.7 * rng.standard_normal((B, P))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32), bank.astype(np.float32)


def similarities(f, bank):
    return np.asarray(f, np.float64) @ np.asarray(bank, np.float64).T


def eps_rows(f, bank):
    """eps[b]: the fp32 dot-product bound for any summation order, per query row."""
    P = f.shape[1]
    gamma = P * U / (1.0 - P * U)
    return gamma * (np.abs(np.asarray(f, np.float64)) @ np.abs(np.asarray(bank, np.float64)).T).max(axis=1)


def top_from_similarities(s, k):
    """[B,k] the k largest per row, descending; a NaN is never selected; -inf where nothing is left."""
    s = np.where(np.isnan(s), -np.inf, np.asarray(s, np.float64))
    srt = -np.sort(-s, axis=1)[:, :k]
    if srt.shape[1] < k:
        srt = np.concatenate([srt, np.full((s.shape[0], k - srt.shape[1]), -np.inf)], axis=1)
    return srt


def score_of(vk):
    """sqrt(max(0, 2 - 2 v)) in fp64 (-inf -> +inf)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.maximum(0.0, 2.0 - 2.0 * np.asarray(vk, np.float64)))


def knn_reference(f, bank, k):
    """(topv [B,k] fp64 descending, scores [B] fp64) from fp64 similarities."""
    topv = top_from_similarities(similarities(f, bank), k)
    return topv, score_of(topv[:, k - 1])


def tie_free_rows(f, bank, k):
    """Rows whose k-th and (k+1)-th largest similarities differ (k < N).  At least 90 % must be, so that taking k + 1 for k
    cannot hide behind ties."""
    srt = top_from_similarities(similarities(f, bank), k + 1)
    free = srt[:, k - 1] != srt[:, k]
    assert free.mean() >= 0.90, free.mean()
    return free


def list_ratio(got, ref, eps):
    """max |got - ref| / eps[b] over the finite slots of ref; a slot that is -inf in one must be -inf in the other
    (ratio inf otherwise).  eps may be 0 (lattice inputs): then any difference gives inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin]) or not np.isfinite(got[fin]).all():
        return np.inf
    d = np.zeros(ref.shape)
    d[fin] = np.abs(got[fin] - ref[fin])
    e = np.broadcast_to(np.asarray(eps, np.float64).reshape(-1, 1), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / e)
    return float(r.max()) if r.size else 0.0


def score_ratio(got, ref_vk, eps):
    """How far got[b] lies from the reference score, in units of the room the budget leaves on that side: the image of
    [v - eps, v + eps] under the score map, widened by one fp32 ulp.  <= 1 is inside."""
    got = np.asarray(got, np.float64)
    v, eps = np.asarray(ref_vk, np.float64), np.asarray(eps, np.float64)
    ref, lo, hi = score_of(v), score_of(v + eps), score_of(v - eps)
    out = np.zeros(got.shape)
    for b in range(got.shape[0]):
        if not np.isfinite(ref[b]):
            out[b] = 0.0 if got[b] == ref[b] else np.inf
            continue
        ulp = float(np.spacing(np.float32(max(hi[b], np.finfo(np.float32).tiny))))
        room = (hi[b] - ref[b] + ulp) if got[b] >= ref[b] else (ref[b] - lo[b] + ulp)
        out[b] = abs(got[b] - ref[b]) / room
    return float(out.max()) if out.size else 0.0


def bf16_round(x):
    """fp32 -> bf16 -> fp32, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)
