"""Inputs, the fp64 reference and the error budget of GL-MCM's local score (glmcm.hip, mcm_local_score_features): numpy only.

Definitions.  local [B, R, P] patch rows, text [K, P] the prompt bank, s[b, i, k] their dot products, Td = (double) (float) T:
patch[b, i] = max_k softmax_k(s[b, i, :] / Td) = 1 / sum_k exp((s[b, i, k] - max_k s[b, i, k]) / Td), S_L[b] = max_i patch[b, i],
local_scores[b] = -S_L[b].  The reference is fp64 from the fp32 inputs.

Inputs:
  * lattice_case: entries are integers in [-63, 63] times 2^-11, so every similarity is EXACT in fp32 in any summation order
    (tests/knn_budget.py); the result is then held to the arithmetic term plus one ulp alone;
  * unit_case: seeded unit rows; ONE (patch, prompt) cell per image is planted (plants()), with a strength that grows with the
    image index, so that a single cell decides S_L: a row or a prompt counted wrongly, or not at all, moves the result by far
    more than the budget.  It also hands back what the deliberate mistakes of tests/test_glmcm_budget.py need: a CLS row per
    image (planted more strongly than any patch) and the positive factors of the un-normalised rows.

Budget of patch[b, i] (and of S_L, the maximum of R of them: |max a - max b| <= max |a - b|) = similarity term + arithmetic
term + one fp32 ulp of the result.

Similarity term.  eps[b, i] = gamma_P max_k sum_c |l_bic t_kc|, gamma_P = P u32 / (1 - P u32), bounds the error of an fp32 dot
product of P single-rounded products in any order.  Every softmax probability is exp(s_k / Td) / sum_j exp(s_j / Td): moving
every s by at most eps moves the numerator and every term of the denominator by a factor within exp(+-eps / Td), hence every
probability, and their maximum, by a factor within exp(+-2 eps / Td):  sim = patch (exp(2 eps / Td) - 1).

Arithmetic term, from what glm_rows_kernel does (u = 2^-53, X[b, i] = 2 max_k |s| / Td >= every |(s - max) / Td|):
  (a) the maximum is one of the fp32 values: exact;
  (b) x = fl(fl((double) s - (double) m) * invT), invT = fl(1 / Td): three roundings, |dx| <= 3 u X;
  (c) exp is the fp64 library exp, stated at 1 ulp = 2 u: every term carries a relative error of at most 3 u X + 2 u;
  (d) the terms are non-negative and summed in fp64 (a lane's strided share, a 6-step butterfly, the carried sum): at most
      K - 1 additions deep in any order, relative error <= K u;
  (e) when a later tile raises the maximum the carried sum is multiplied by exp(fl(fl(m - M) * invT)): 3 u X + 3 u each time,
      at most K / 256 + 1 times;
  (f) 1 / sum in fp64: u.
      rel = u (K + (K / 256 + 2) (3 X + 3) + 1),  arith = patch rel (1 + 2^-20)  (the factor: second-order terms).
The conversion of 1 / sum to fp32 is the "one ulp of the result" (taken at the far end of the interval); the per-image maximum
of fp32 values is exact.  There is no empirical margin."""
import numpy as np

from tests.knn_budget import LATTICE, U  # noqa: F401  (shared definitions)
from tests.neglabel_budget import ratio, t_double  # noqa: F401

U64 = 2.0 ** -53
TILE = 256
QTILE = 64


def lattice_case(B, R, K, P, seed):
    """(local [B,R,P], text [K,P]) fp32 on the lattice: every similarity exact in fp32."""
    assert P <= 1024
    rng = np.random.default_rng(seed)
    local = (rng.integers(-63, 64, size=(B, R, P)) * LATTICE).astype(np.float32)
    text = (rng.integers(-63, 64, size=(K, P)) * LATTICE).astype(np.float32)
    s64 = similarities(local, text)
    assert np.array_equal((local.reshape(-1, P) @ text.T).astype(np.float64).reshape(s64.shape), s64)
    return local, text


def plants(B, R, K):
    """[(patch, prompt)] per image: the one cell that decides S_L.  Patches cycle through the first and the last patch of the
    image and the two patches on either side of a 64-row query-tile edge inside the image (rows of [B R, P]; the first patch
    where the image holds no edge); the last image takes its last patch.  Prompts cycle through 0, 255, 256 and K - 1 (clipped
    to the bank); the last image takes K - 1."""
    out = []
    for b in range(B):
        lo = b * R
        edge = (lo // QTILE + 1) * QTILE  # the first row of the next query tile
        below, above = (edge - 1 - lo, edge - lo) if edge < lo + R else (0, 0)
        patch = [0, R - 1, below, above][b % 4]
        prompt = min([0, 255, 256, K - 1][b % 4], K - 1)
        if b == B - 1:
            patch, prompt = R - 1, K - 1
        out.append((patch, prompt))
    return out


def unit_case(B, R, K, P, seed):
    """(local [B,R,P], text [K,P], cls [B,P], scale [B,R]) fp32.  Rows of unit norm (to fp32 round-off); image b's planted
    patch (plants()) is pulled toward its prompt with cosine about 0.6 + 0.3 b / max(B - 1, 1), its CLS row toward prompt
    1 % K with cosine about 0.97; scale: factors in [2, 6), the norms the rows had before they were normalised."""
    rng = np.random.default_rng(seed)
    text = rng.standard_normal((K, P))
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    local = rng.standard_normal((B, R, P))
    local /= np.linalg.norm(local, axis=2, keepdims=True)
    cls = rng.standard_normal((B, P))
    cls /= np.linalg.norm(cls, axis=1, keepdims=True)
    for b, (i, k) in enumerate(plants(B, R, K)):
        a = 0.6 + 0.3 * b / max(B - 1, 1)
        local[b, i] = a * text[k] + np.sqrt(1.0 - a * a) * local[b, i]
        cls[b] = 0.97 * text[1 % K] + np.sqrt(1.0 - 0.97 ** 2) * cls[b]
    local /= np.linalg.norm(local, axis=2, keepdims=True)
    cls /= np.linalg.norm(cls, axis=1, keepdims=True)
    scale = rng.uniform(2.0, 6.0, size=(B, R))
    return local.astype(np.float32), text.astype(np.float32), cls.astype(np.float32), scale.astype(np.float32)


def similarities(local, text):
    """[B, R, K] in fp64 from the fp32 inputs."""
    return np.asarray(local, np.float64) @ np.asarray(text, np.float64).T


def eps_cells(local, text):
    """eps[b, i]: the fp32 dot-product bound for any summation order, per patch row."""
    P = local.shape[-1]
    gamma = P * U / (1.0 - P * U)
    return gamma * (np.abs(np.asarray(local, np.float64)) @ np.abs(np.asarray(text, np.float64)).T).max(axis=-1)


def reference_from_similarities(s64, T):
    """(patch [B,R], local_scores [B] = -S_L) in fp64 from similarities [B, R, K]."""
    z = (s64 - s64.max(axis=-1, keepdims=True)) / t_double(T)
    patch = 1.0 / np.exp(z).sum(axis=-1)
    return patch, -patch.max(axis=1)


def reference(local, text, T):
    return reference_from_similarities(similarities(local, text), T)


def budgets(local, text, T, exact=False):
    """(budget_patch [B,R], budget_score [B]) around reference(): similarity term + arithmetic term + one fp32 ulp of the
    result.  exact=True (lattice inputs: the similarities carry no error): without the similarity term."""
    s64 = similarities(local, text)
    K = s64.shape[-1]
    patch, score = reference_from_similarities(s64, T)
    Td = t_double(T)
    X = 2.0 * np.abs(s64).max(axis=-1) / Td
    sim = 0.0 if exact else patch * np.expm1(2.0 * eps_cells(local, text) / Td)
    arith = patch * (1.0 + 2.0 ** -20) * U64 * (K + (K / TILE + 2.0) * (3.0 * X + 3.0) + 1.0)
    tiny = float(np.finfo(np.float32).tiny)

    def with_ulp(ref, room):
        far = np.maximum(np.abs(ref) + room, tiny).astype(np.float32)
        far = np.where(far.astype(np.float64) < np.abs(ref) + room, np.nextafter(far, np.float32(np.inf)), far)
        return room + np.spacing(far).astype(np.float64) + tiny

    room = sim + arith
    return with_ulp(patch, room), with_ulp(score, room.max(axis=1))


def restate_fp32(local, text, T, *, cls=None, mean=False, t_after=False, scale=None, first_tile_only=False, neighbour=False):
    """What the two kernels compute, in numpy: fp32 similarities (numpy's fp32 matmul), the bank walked in tiles of 256 with one
    (fp32 max, fp64 sum) pair per row, patch = (float)(1 / sum), the per-image maximum.  Returns (local_scores [B] fp32,
    patch [B,R] fp32).  The keyword switches are the deliberate mistakes of tests/test_glmcm_budget.py:
      cls              [B,P]: the CLS row counted as a local row of its image;
      mean             the mean over the patches instead of their maximum;
      t_after          the softmax taken at temperature 1 and its maximum divided by T;
      scale            [B,R]: the rows left un-normalised (row times its factor);
      first_tile_only  the prompts beyond the first 256-row tile dropped;
      neighbour        image b also counts the first patch of image b + 1."""
    local, text = np.asarray(local, np.float32), np.asarray(text, np.float32)
    if scale is not None:
        local = local * np.asarray(scale, np.float32)[:, :, None]
    if cls is not None:
        local = np.concatenate([np.asarray(cls, np.float32)[:, None, :], local], axis=1)
    B, R, P = local.shape
    K = text.shape[0] if not first_tile_only else min(TILE, text.shape[0])
    s = (local.reshape(B * R, P) @ text[:K].T).astype(np.float32)
    inv = 1.0 / (1.0 if t_after else t_double(T))
    m, acc = np.full(B * R, -np.inf, np.float32), np.zeros(B * R)
    for n0 in range(0, K, TILE):
        seg = s[:, n0:n0 + TILE]
        M = np.maximum(m, seg.max(axis=1))
        with np.errstate(invalid="ignore"):
            resc = np.where(m == M, 1.0, np.exp((m.astype(np.float64) - M.astype(np.float64)) * inv))
        acc = acc * resc + np.exp((seg.astype(np.float64) - M.astype(np.float64)[:, None]) * inv).sum(axis=1)
        m = M
    patch = (1.0 / acc).astype(np.float32).reshape(B, R)
    if t_after:
        patch = (patch.astype(np.float64) / t_double(T)).astype(np.float32)
    if mean:
        top = patch.astype(np.float64).mean(axis=1).astype(np.float32)
    else:
        top = patch.max(axis=1)
        if neighbour:
            top[:-1] = np.maximum(top[:-1], patch[1:, 0])
    if cls is not None:
        patch = patch[:, 1:]
    return -top, patch
