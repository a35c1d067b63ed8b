"""Error model of the device Mahalanobis fit (score.hip maha_fit_kernel, mcm_amd.detection.get_mean_prec_device): references
and per-entry budgets, pure numpy, in the style of tests/error_budget.py.

The fit keeps gram = sum_b x_b x_b^T and sum = sum_b x_b in fp64 over the shifted rows x_b = f_b - shift and closes with
cov = (gram - sum sum^T / n) / (n - 1) on the host.  The reference is the two-pass centred covariance in np.longdouble (63
mantissa bits on x86); its own error, 4 n 2^-64 |ref|, is part of every budget.  Where longdouble is no wider than that
the reference is taken on a fixed sample of 512 entries with math.fsum over error-free products instead.

u64 = 2^-53.  Per entry, with xa = |x - shift|, A = sum_b xa, Sa = |sum|, G = gram:

  [ n u64 (xa^T xa)                                   the gram recurrence: one rounding per row (fma), n rows
    + ( n u64 (A Sa^T + Sa A^T) + 3 u64 Sa Sa^T ) / n the sum recurrence (n u64 A per element), carried through the outer
                                                      product, and the product's and the division's own roundings
    + 2 u64 ( |G| + Sa Sa^T / n ) ]                   the closing subtraction and the division by n - 1
  / (n - 1) * 1.01                                    (1.01: the slack score_budget uses)
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests.error_budget import U64, ulp

LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63          # x86 extended precision (or better): the longdouble reference is usable
U_REF = 2.0 ** -64
SLACK = 1.01
N_SAMPLE = 512                            # entries of the fsum reference


def fit_case(n: int, P: int, offset: float, seed: int = 0, offset_kind: str = "sigma"):
    """fp32 features [n, P]: randn x a per-column scale in [0.05, 2], plus a column offset — `offset` standard deviations
    of the column with a random sign ("sigma"), or `offset` x randn ("randn")."""
    rng = np.random.default_rng([seed, n, P])
    scale = rng.uniform(0.05, 2.0, P)
    off = offset * scale * rng.choice([-1.0, 1.0], P) if offset_kind == "sigma" else offset * rng.standard_normal(P)
    return (rng.standard_normal((n, P)) * scale[None, :] + off[None, :]).astype(np.float32)


def first_batch_shift(x, batch: int = 8) -> np.ndarray:
    """The fit's shift: the fp32 column mean of the first batch."""
    return np.asarray(x, np.float32)[:batch].mean(axis=0, dtype=np.float32)


def shifted(x, shift) -> np.ndarray:
    """(double)f - (double)shift, the kernel's operand (shift None = 0)."""
    x64 = np.asarray(x, np.float64)
    return x64 if shift is None else x64 - np.asarray(shift, np.float64)[None, :]


def _ld_gram(a, block: int = 256):
    """a^T a in longdouble: upper-triangle blocks, mirrored (numpy has no BLAS for longdouble)."""
    a = np.asarray(a, LD)
    P = a.shape[1]
    g = np.empty((P, P), LD)
    for i in range(0, P, block):
        for j in range(i, P, block):
            t = a[:, i:i + block].T @ a[:, j:j + block]
            g[i:i + block, j:j + block] = t
            g[j:j + block, i:i + block] = t.T
    return g


def sample_entries(P: int, mag=None):
    """(rows, cols) of the fixed sample the fsum reference covers: the diagonal first (as much of it as fits), the largest and
    smallest |entry| of `mag`, the rest seeded."""
    rng = np.random.default_rng(P)
    pairs = [(i, i) for i in range(min(P, N_SAMPLE // 2))]
    if mag is not None:
        m = np.abs(np.asarray(mag, np.float64))
        pairs += [np.unravel_index(int(np.argmax(m)), m.shape), np.unravel_index(int(np.argmin(m)), m.shape)]
    while len(pairs) < N_SAMPLE:
        pairs.append((int(rng.integers(P)), int(rng.integers(P))))
    r, c = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    return r, c


def _fsum_dot(u, v) -> float:
    """sum_b u_b v_b, correctly rounded: each product as its rounded value plus its exact remainder, summed by math.fsum."""
    terms = []
    for a, b in zip(u.tolist(), v.tolist()):
        p = a * b
        terms += [p, float(Fraction(a) * Fraction(b) - Fraction(p))]
    return math.fsum(terms)


def gram_sum_reference(xs):
    """(gram, sum, own error of gram, own error of sum) of the shifted rows xs [n, P] (fp64 values): longdouble sums.
    Without a wide longdouble: math.fsum on sample_entries, NaN elsewhere (NaN never fails eb.worst-style comparisons here:
    use `covered`)."""
    xs = np.asarray(xs, np.float64)
    n, P = xs.shape
    if WIDE:
        g, s = _ld_gram(xs), xs.astype(LD).sum(axis=0)
        return g, s, n * U_REF * (np.abs(xs).T @ np.abs(xs)), n * U_REF * np.abs(xs).sum(axis=0)
    g = np.full((P, P), np.nan)
    r, c = sample_entries(P, xs.T @ xs)
    for i, j in zip(r, c):
        g[i, j] = _fsum_dot(xs[:, i], xs[:, j])
    s = np.array([math.fsum(xs[:, j].tolist()) for j in range(P)])
    return g, s, U64 * np.abs(g), U64 * np.abs(s)


def cov_reference(x):
    """(ref, own error): the two-pass centred covariance of the fp32 rows x.  n = 1 gives 0 / 0 = NaN, as torch.cov does."""
    x = np.asarray(x, np.float64)
    n, P = x.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        if WIDE:
            xl = x.astype(LD)
            c = xl - xl.sum(axis=0)[None, :] / LD(n)
            ref = _ld_gram(c) / LD(n - 1)
            return ref, 4.0 * n * U_REF * np.abs(ref).astype(np.float64)
        mean = np.array([math.fsum(x[:, j].tolist()) for j in range(P)]) / n
        c = x - mean[None, :]                  # two fp64 roundings per centred value: the own-error term below
        ref = np.full((P, P), np.nan)
        r, cc = sample_entries(P, c.T @ c)
        for i, j in zip(r, cc):
            ref[i, j] = _fsum_dot(c[:, i], c[:, j]) / (n - 1)
        return ref, (4.0 * U64 * (np.abs(c).T @ np.abs(c)) + 2.0 * U64 * np.abs(c.T @ c)) / (n - 1)


def gram_budget(xs):
    """First term: |gram - exact| <= n u64 xa^T xa (x 1.01)."""
    xa = np.abs(np.asarray(xs, np.float64))
    return xa.shape[0] * U64 * (xa.T @ xa) * SLACK


def sum_budget(xs):
    """Second term's source: |sum - exact| <= n u64 A (x 1.01)."""
    xa = np.abs(np.asarray(xs, np.float64))
    return xa.shape[0] * U64 * xa.sum(axis=0) * SLACK


def cov_budget(x, shift=None):
    """Per-entry budget of the fit's covariance for the fp32 rows x accumulated with `shift` (the formula of the module
    docstring), without the reference's own error."""
    xs = shifted(x, shift)
    n = xs.shape[0]
    xa = np.abs(xs)
    A, Sa, G = xa.sum(axis=0), np.abs(xs.sum(axis=0)), xs.T @ xs
    SS = np.outer(Sa, Sa)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (n * U64 * (xa.T @ xa) + (n * U64 * (np.outer(A, Sa) + np.outer(Sa, A)) + 3.0 * U64 * SS) / n
                + 2.0 * U64 * (np.abs(G) + SS / n)) / (n - 1) * SLACK


def _ratio(err, bud):
    """err / bud per entry; a zero budget (all-zero operands: B = 1 shifted by its own row) admits a zero error only."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bud > 0, err / bud, np.where(err == 0, 0.0, np.inf))


def cov_ratio(got, x, shift=None):
    """max |got - ref| / (budget + the reference's own error) over the entries the reference covers, and the flat index of
    the worst one; a non-finite `got` counts as infinite."""
    ref, own = cov_reference(x)
    bud = cov_budget(x, shift) + own
    covered = ~np.isnan(np.asarray(ref, np.float64))
    err = np.abs(np.asarray(got, LD) - ref).astype(np.float64)
    err = np.where(np.isfinite(np.asarray(got, np.float64)), err, np.inf)
    ratio = np.where(covered, _ratio(err, bud), 0.0)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i


def entry_ratio(got, ref, bud):
    """max |got - ref| / bud over the entries with a reference (NaN in ref = not covered); non-finite got = infinite."""
    refd = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, LD) - ref).astype(np.float64)
    err = np.where(np.isfinite(np.asarray(got, np.float64)), err, np.inf)
    ratio = np.where(np.isnan(refd), 0.0, _ratio(err, bud))
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i


def finalise(gram, fsum, n):
    """The host's closing step in fp64: (gram - sum sum^T / n) / (n - 1)."""
    gram, fsum = np.asarray(gram, np.float64), np.asarray(fsum, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (gram - np.outer(fsum, fsum) / np.float64(n)) / np.float64(n - 1)


def emulate_fit(x, shift=None, mutation: str | None = None):
    """Row-sequential emulation of the kernel and the closing step: gram and sum accumulate one shifted row after another
    (numpy rounds the product and the addition separately: two roundings where the kernel's fma has one — still n u64 of
    the absolute sum).  mutation: "fp32" accumulates in fp32, "sum_unshifted" drops the shift from sum but not from gram,
    "div_n" divides by n instead of n - 1."""
    x = np.asarray(x, np.float32)
    n, P = x.shape
    acc = np.float32 if mutation == "fp32" else np.float64
    sh = np.zeros(P) if shift is None else np.asarray(shift, np.float64)
    gram, fsum = np.zeros((P, P), acc), np.zeros(P, acc)
    for b in range(n):
        xb = x[b].astype(np.float64) - sh
        gram += np.outer(xb, xb).astype(acc)
        fsum += (x[b].astype(np.float64) if mutation == "sum_unshifted" else xb).astype(acc)
    cov = finalise(gram, fsum, n)
    if mutation == "div_n":
        cov = cov * (n - 1) / n
    return cov


def precision_bound(ref_cov, bud):
    """(ref precision, per-entry bound) for precision = fp32(inv(cov)), cov within `bud` (per entry) of ref_cov.
    First order, with a = ||ref^-1||_2 and d = ||bud||_F >= ||cov - ref||_2:  ||inv(cov) - inv(ref)||_2 <= a^2 d / (1 - a d),
    which bounds every entry; + 0.5 ulp32 for the cast.  Both inverses are fp64 LAPACK results (the reference's here too:
    numpy has no longdouble solver), each off by about P u64 cond a: twice that is the reference's own term."""
    ref64 = np.asarray(ref_cov, np.float64)
    P = ref64.shape[0]
    prec = np.linalg.inv(ref64)
    a = np.linalg.norm(prec, 2)
    d = np.linalg.norm(np.asarray(bud, np.float64), "fro")
    ad = a * d
    first = a * a * d / (1.0 - ad) if ad < 1.0 else np.inf
    own = 2.0 * P * U64 * np.linalg.cond(ref64) * a
    return prec, first + own + 0.5 * ulp(prec, "fp32")
