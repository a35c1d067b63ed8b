"""tests/eval_reference.py proved on the CPU: it reproduces the reference's own outputs, equals the host route on finite
inputs, its two formulations agree, and every planted counting mistake of a kernel emulation falls outside the criterion the
GPU tests apply (tests/test_gpu_eval_tail.py)."""
import math
import os

import numpy as np
import pytest

from tests import eval_reference as er


@pytest.mark.parametrize("case", ["kat", "gauss", "ties", "narrow", "equal", "sep"])
def test_reproduces_reference_outputs(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "measures.npz"))
    pos, neg = g[f"{case}_pos"], g[f"{case}_neg"]
    both = np.concatenate([pos, neg])
    assert np.unique(both).size == np.unique(both.astype(np.float32)).size   # the fp32 cast keeps the order: same counts
    got = np.array(er.measures_exact(pos, neg))
    np.testing.assert_allclose(got, g[f"{case}_measures"], rtol=0, atol=1e-12)   # tests/test_metrics.py's tolerance


def _scores(n_pos, n_neg, quant, seed):
    rng = np.random.default_rng(seed)
    pos = rng.normal(0.6, 1.0, n_pos).astype(np.float32)
    neg = rng.normal(-0.4, 1.2, n_neg).astype(np.float32)
    if quant:
        pos, neg = np.round(pos * quant / 8).astype(np.float32), np.round(neg * quant / 8).astype(np.float32)
    return pos, neg


@pytest.mark.parametrize("n_pos,n_neg,quant,level", [
    (1, 1, 0, 0.95), (3, 1, 0, 0.95), (1, 7, 2, 0.95), (300, 200, 0, 0.95), (257, 511, 16, 0.9), (1237, 4099, 0, 0.5),
    (5000, 5640, 64, 0.95), (64, 64, 16, 0.0), (64, 64, 16, 1.0), (50000, 10000, 4096, 0.95),
])
def test_equals_host_route_on_finite_inputs(n_pos, n_neg, quant, level):
    from mcm_amd.metrics import get_measures

    pos, neg = _scores(n_pos, n_neg, quant, n_pos + n_neg)
    got = er.measures_exact(pos, neg, level)
    want = get_measures(pos, neg, recall_level=level)
    assert got[0] == pytest.approx(want[0], rel=0, abs=1e-12)     # sklearn's trapezoid sum rounds differently
    assert got[1] == pytest.approx(want[1], rel=0, abs=1e-12)
    assert got[2] == want[2]                                      # a ratio of exact counts on both sides


@pytest.mark.parametrize("seed", range(6))
def test_sorted_and_broadcast_formulations_agree(seed):
    rng = np.random.default_rng(seed)
    n_pos, n_neg = int(rng.integers(1, 200)), int(rng.integers(1, 200))
    pos, neg = _scores(n_pos, n_neg, (0, 16)[seed % 2], seed)
    # the special values, at random places
    for special in (-np.inf, np.inf, -0.0, 0.0, 1e-45, 2e-45, np.finfo(np.float32).max, -np.finfo(np.float32).max):
        (pos if rng.random() < 0.5 else neg)[int(rng.integers(0, min(n_pos, n_neg)))] = special
    for level in (0.0, 0.5, 0.95, 1.0, (n_pos // 2) / n_pos):
        a, b = er.measures_exact(pos, neg, level), er.measures_bruteforce(pos, neg, level)
        assert a[0] == b[0] and a[2] == b[2] and a[1] == b[1]


def test_special_values_are_ordered_values():
    inf = np.inf
    # -inf below everything, +inf above: perfectly separated both ways
    assert er.measures_exact([inf, 1.0], [-inf, 0.0]) == (1.0, 1.0, 0.0)
    a = er.measures_exact([-inf, 0.0], [inf, 1.0])
    assert a[0] == 0.0 and a[2] == 1.0
    # a -inf positive ties a -inf negative (half a win) and loses to nothing else
    assert er.measures_exact([-inf], [-inf])[0] == 0.5
    assert er.measures_exact([-inf], [-inf, -inf, 0.0])[0] == (2 * 0 + 2) / 6
    # signed zeros tie
    assert er.measures_exact([-0.0], [0.0]) == er.measures_exact([0.0], [0.0]) == (0.5, 0.5, 1.0)
    # subnormals that differ only below 2^-126 stay distinct
    t = np.float32(1e-45)
    assert t > 0 and er.measures_exact([2 * t], [t]) == (1.0, 1.0, 0.0)
    # NaN anywhere: NaN everywhere
    assert all(math.isnan(v) for v in er.measures_exact([1.0, np.nan], [0.0]))
    assert all(math.isnan(v) for v in er.measures_exact([1.0], [0.0, np.nan]))


def test_recall_tie_goes_to_the_lowest_threshold():
    # 4 positives in two tied pairs: operating points at recall 0.5 (t = 2) and 1.0 (t = 1); level 0.75 is exactly between
    # (all values exact in fp64).  The lowest threshold, t = 1, admits both negatives at 1.5 and 1.0: FPR 2/3, not 0.
    pos, neg = [2.0, 2.0, 1.0, 1.0], [1.5, 1.0, 0.0]
    assert er.measures_exact(pos, neg, 0.75)[2] == 2 / 3
    assert er.measures_exact(pos, neg, 0.75, _highest_tie=True)[2] == 0.0
    assert er.measures_bruteforce(pos, neg, 0.75)[2] == 2 / 3


# ---- planted mistakes ------------------------------------------------------------------------------------------------------
def _tie_case():
    """Quantised scores (ties between the classes), a -inf in each class, sizes ragged against the 4096 tile, and a recall
    level that ties exactly between two operating points (n_pos = 64: every recall is a dyadic rational)."""
    rng = np.random.default_rng(11)
    pos = np.round(rng.normal(0.6, 1.0, 64) * 2).astype(np.float32)
    neg = np.round(rng.normal(-0.4, 1.2, 101) * 2).astype(np.float32)
    pos[5] = -np.inf
    neg[7] = -np.inf
    ts = np.unique(pos)
    tp = np.array([(pos >= t).sum() for t in ts])
    i = len(ts) // 2
    level = (tp[i] + tp[i + 1]) / 2 / 64          # halfway between two adjacent operating points
    return pos, neg, float(level)


def test_correct_emulation_agrees():
    pos, neg, level = _tie_case()
    assert er.agrees(er.kernel_emulation(pos, neg, level), er.measures_exact(pos, neg, level), pos.size)
    for n_pos, n_neg, quant in ((1, 1, 0), (255, 257, 16), (300, 70, 0)):
        pos, neg = _scores(n_pos, n_neg, quant, 3)
        for level in (0.0, 0.95, 1.0):
            assert er.agrees(er.kernel_emulation(pos, neg, level), er.measures_exact(pos, neg, level), n_pos)


@pytest.mark.parametrize("mistake", ["strict", "ties_whole", "inf_pad", "highest"])
def test_planted_mistakes_fall_outside(mistake):
    pos, neg, level = _tie_case()
    want = er.measures_exact(pos, neg, level)
    got = er.kernel_emulation(pos, neg, level, mistake)
    assert not er.agrees(got, want, pos.size)
    # by how much: the miss is of the size of a count, orders of magnitude beyond the rounding the criterion allows
    miss = max(abs(got[0] - want[0]), abs(got[2] - want[2]), abs(got[1] - want[1]) - er.aupr_bound(pos.size))
    print(f"MISTAKE {mistake}: got {got} want {want}")
    assert miss >= 1.0 / (2 * pos.size * neg.size)     # at least half a pair / one count, >= 1e9 aupr_bound here
    assert 1.0 / (2 * pos.size * neg.size) > 1e9 * er.aupr_bound(pos.size)


def test_inf_pad_mistake_needs_a_ragged_size_and_a_minus_inf():
    """The planted -inf padding is invisible at an exact tile multiple or without a -inf score among the positives: the GPU
    cases must be ragged AND hold a -inf positive (after the sign flip) to see it."""
    rng = np.random.default_rng(2)
    pos = rng.normal(0.5, 1, 300).astype(np.float32)
    neg = rng.normal(-0.5, 1, 200).astype(np.float32)
    assert er.agrees(er.kernel_emulation(pos, neg, 0.95, "inf_pad"), er.measures_exact(pos, neg), 300)
    # among the negatives alone it stays invisible: only the counts of positives, and of examples >= min(pos), are ever read
    neg[0] = -np.inf
    assert er.agrees(er.kernel_emulation(pos, neg, 0.95, "inf_pad"), er.measures_exact(pos, neg), 300)
    pos[0] = -np.inf
    got, want = er.kernel_emulation(pos, neg, 0.95, "inf_pad"), er.measures_exact(pos, neg)
    assert not er.agrees(got, want, 300)
    # and at an exact tile multiple there is no pad
    pos, neg = np.resize(pos, er.TILE), np.resize(neg, 2 * er.TILE)
    assert er.agrees(er.kernel_emulation(pos, neg, 0.95, "inf_pad"), er.measures_exact(pos, neg), er.TILE)


def test_aupr_bound_covers_fp64_sums_in_any_order():
    rng = np.random.default_rng(0)
    for n_pos, n_neg in ((1, 1), (2, 3), (4097, 8193)):
        pos, neg = _scores(n_pos, n_neg, 16, 1)
        want = er.measures_exact(pos, neg)[1]
        ps, ns = np.sort(pos), np.sort(neg)
        tp = (n_pos - np.searchsorted(ps, pos, side="left")).astype(np.float64)
        fp = (n_neg - np.searchsorted(ns, pos, side="left")).astype(np.float64)
        terms = tp / (tp + fp)
        for order in (np.arange(n_pos), np.argsort(terms), np.argsort(-terms), rng.permutation(n_pos)):
            s = 0.0
            for v in terms[order]:
                s += float(v)
            assert abs(s / n_pos - want) <= er.aupr_bound(n_pos)
