"""tests/knn_budget.py on the CPU: numpy fp32 similarities (one of the summation orders the bound covers) pass the unit budget
and equal the fp64 reference on lattice inputs, and three wrong implementations — k + 1 taken for k, a dropped ragged tail,
bf16-rounded operands — break the checks on the inputs the GPU tests use."""
import numpy as np
import pytest

from tests import knn_budget as kb

B, N = 65, 3001
KS = [1, 10, 200, 1000]


def _lists(s, k):
    t = kb.top_from_similarities(s, k)
    return t, kb.score_of(t[:, k - 1]).astype(np.float32)


@pytest.mark.parametrize("P", [64, 512, 1024])
def test_numpy_fp32_passes_the_unit_budget(P):
    f, bank = kb.unit_case(B, N, P, seed=P)
    eps = kb.eps_rows(f, bank)
    assert (eps > 0).all() and eps.max() < 2e-4
    for k in KS:
        ref, _ = kb.knn_reference(f, bank, k)
        got, sc = _lists((f @ bank.T).astype(np.float32), k)
        rl, rs = kb.list_ratio(got, ref, eps), kb.score_ratio(sc, ref[:, k - 1], eps)
        print(f"BUDGET knn numpy-fp32 {max(rl, rs):.3f} P={P} k={k}")
        assert rl <= 1.0 and rs <= 1.0, (P, k, rl, rs)


@pytest.mark.parametrize("P", [64, 512, 1024])
def test_lattice_lists_are_exact_in_fp32(P):
    f, bank = kb.lattice_case(B, N, P, seed=P)
    assert np.array_equal(bank[N // 2], bank[0]) and np.array_equal(bank[N - 1], bank[1])
    for k in [1, 10, 64, 200, 1000, 1024]:
        ref, sref = kb.knn_reference(f, bank, k)
        got, _ = _lists((f @ bank.T).astype(np.float32), k)
        assert np.array_equal(got, ref)
        assert kb.list_ratio(got, ref, 0.0) == 0.0
        free = kb.tie_free_rows(f, bank, k)
        assert 1.0 - free.mean() <= 0.062, (P, k, free.mean())


def test_k_larger_than_the_bank_pads_and_nan_is_never_selected():
    f, bank = kb.lattice_case(3, 5, 64, seed=1)
    ref, sc = kb.knn_reference(f, bank, 7)
    assert np.isfinite(ref[:, :5]).all() and np.isneginf(ref[:, 5:]).all() and np.isposinf(sc).all()
    s = kb.similarities(f, bank)
    s[:, 2] = np.nan
    t = kb.top_from_similarities(s, 5)
    assert np.isneginf(t[:, 4]).all() and not np.isnan(t).any()


def _k_plus_one(s, k):
    """The slip: the (k + 1)-th largest where the k-th belongs."""
    t = kb.top_from_similarities(s, k + 1)
    return np.concatenate([t[:, :k - 1], t[:, k:k + 1]], axis=1)


@pytest.mark.parametrize("k", [1, 10, 200, 1000])
def test_k_plus_one_for_k_is_caught(k):
    f, bank = kb.lattice_case(B, N, 512, seed=3)
    ref, _ = kb.knn_reference(f, bank, k)
    free = kb.tie_free_rows(f, bank, k)
    bad = _k_plus_one((f @ bank.T).astype(np.float32), k)
    assert (bad[free, k - 1] != ref[free, k - 1]).all()                  # exact inequality on every tie-free row
    assert kb.list_ratio(bad, ref, 0.0) == np.inf
    f, bank = kb.unit_case(B, N, 64, seed=64)
    eps = kb.eps_rows(f, bank)
    ref, _ = kb.knn_reference(f, bank, k)
    srt = kb.top_from_similarities(kb.similarities(f, bank), k + 1)
    clear = srt[:, k - 1] - srt[:, k] > 4 * eps
    assert clear.mean() >= 0.85, clear.mean()
    bad = _k_plus_one((f @ bank.T).astype(np.float32), k)
    assert kb.list_ratio(bad, ref, eps) > 1.0
    assert (np.abs(bad[clear, k - 1] - ref[clear, k - 1]) > eps[clear]).all()


@pytest.mark.parametrize("kind", ["lattice", "unit"])
def test_a_dropped_ragged_tail_is_caught(kind):
    """The best neighbours are planted in the last N % 256 rows: a walk that stops at the last whole tile loses them."""
    P, k = 64, 10
    f, bank = (kb.lattice_case if kind == "lattice" else kb.unit_case)(B, N, P, seed=5)
    tail = N % 256
    assert 0 < tail and B <= tail
    bank = bank.copy()
    bank[N - B:] = f                                                     # query b's nearest neighbour is itself, at row N - B + b
    eps = kb.eps_rows(f, bank) if kind == "unit" else np.zeros(B)
    ref, sref = kb.knn_reference(f, bank, k)
    good, _ = _lists((f @ bank.T).astype(np.float32), k)
    assert kb.list_ratio(good, ref, eps) <= 1.0
    bad, sbad = _lists((f @ bank[: N - tail].T).astype(np.float32), k)
    assert kb.list_ratio(bad, ref, eps) > 1.0
    assert (bad[:, 0] < ref[:, 0]).all()


@pytest.mark.parametrize("P", [64, 512, 1024])
def test_bf16_rounded_operands_are_caught(P):
    f, bank = kb.unit_case(B, N, P, seed=P)
    eps = kb.eps_rows(f, bank)
    for k in KS:
        ref, _ = kb.knn_reference(f, bank, k)
        bad, sc = _lists((kb.bf16_round(f) @ kb.bf16_round(bank).T).astype(np.float32), k)
        assert kb.list_ratio(bad, ref, eps) > 1.0, (P, k)
        assert kb.score_ratio(sc, ref[:, k - 1], eps) > 1.0, (P, k)
