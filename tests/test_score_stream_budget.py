"""The budget of the streamed tail of the MCM family (tests/score_stream_budget.py) is neither slack nor wrong: a numpy restatement
of the two kernels is inside it at every split count, and the same restatement with one deliberate mistake is not.  numpy only."""
import numpy as np
import pytest

from tests import score_stream_budget as sb

SPLITS = [1, 2, 3, 32]
# (B, K): the shapes of tests/test_gpu_score_stream.py that reach the walk's edges (a ragged tile, the tile edge, splits of
# several tiles) and are large enough for a mistake to show
SHAPES = [(3, 300), (65, 256), (130, 257), (65, 1000)]
P = 64


@pytest.fixture(scope="module")
def cases():
    """(name, f, bank, T, s64, E): lattice inputs (E = 0) at both temperatures, unit inputs at T = 0.01."""
    out = []
    for B, K in SHAPES:
        f, bank = sb.lattice_case(B, K, P, seed=B + K)
        s64 = sb.similarities(f, bank)
        for T in (0.01, 1.0):
            out.append((f"lattice B={B} K={K} T={T}", f, bank, T, s64, np.zeros_like(s64)))
        f, bank = sb.unit_case(B, K, P, seed=P + K)
        out.append((f"unit B={B} K={K} T=0.01", f, bank, 0.01, sb.similarities(f, bank), sb.eps_elements(f, bank)))
    return out


def _worst(got, s64, E, T, topk=0):
    ref = sb.reference_from_similarities(s64, T)
    idx, prob = sb.topk_reference(s64, T, topk) if topk else (None, None)
    bud = sb.budgets_from_similarities(s64, E, T, prob_idx=idx)
    r = sb.worst_ratio(got, ref, bud)[0]
    if topk:
        r = max(r, sb.prob_ratio(got["prob"], prob, bud["prob"]))
    return r


@pytest.mark.parametrize("splits", SPLITS)
def test_the_restatement_is_inside_the_budget(cases, splits):
    for name, f, bank, T, s64, E in cases:
        got = sb.restate_fp32(f, bank, T, splits, topk=5)
        assert _worst(got, s64, E, T, topk=5) <= 1.0, (name, splits)
        if not E.any():                                                # exact similarities: the order is the reference's
            assert np.array_equal(got["idx"], sb.topk_reference(s64, T, 5)[0]), (name, splits)
        plain = sb.restate_fp32(f, bank, T, splits)
        assert all(np.array_equal(plain[k].view(np.int32), got[k].view(np.int32)) for k in sb.KINDS), (name, splits)


@pytest.mark.parametrize("mistake", ["w_no_dz", "q_scale_a", "var_split_rows", "drop_ragged", "no_rescale"])
def test_a_mistake_in_the_sums_leaves_the_budget(cases, mistake):
    """Three splits: every shape then has a split boundary, and all but (65, 256) a ragged tile.  At T = 1 the lattice softmax is
    nearly flat: every row counts, and every rise of the maximum between tiles or splits moves W and Q, so each mistake must
    show in each of those cases.  At T = 0.01 one planted logit can dominate so far that what a mistake moves lies below the
    budget on that row (rightly: the result does not depend on it), so there the mistake must show in some case of each kind."""
    seen = {}
    for name, f, bank, T, s64, E in cases:
        if mistake == "drop_ragged" and "K=256" in name:
            continue                                                   # three splits of 86 rows are ragged, 256 is not asked
        got = sb.restate_fp32(f, bank, T, 3, **{mistake: True})
        seen[name] = _worst(got, s64, E, T) > 1.0
    assert all(v for n, v in seen.items() if n.endswith("T=1.0")), (mistake, seen)
    assert any(v for n, v in seen.items() if n.startswith("unit")), (mistake, seen)
    assert any(v for n, v in seen.items() if n.startswith("lattice") and n.endswith("T=0.01")), (mistake, seen)


def test_a_tie_given_to_the_higher_row_is_seen():
    """tests/knn_budget.py's lattice bank holds rows K // 2 and K - 1 as copies of rows 0 and 1: two ties in every query's order."""
    B, K = 65, 1000
    f, bank = sb.lattice_case(B, K, P, seed=7)
    s64 = sb.similarities(f, bank)
    want = sb.topk_reference(s64, 1.0, K)[0]
    for splits in SPLITS:
        top = sb.restate_fp32(f, bank, 1.0, splits, topk=8)["idx"]
        assert np.array_equal(top, want[:, :8]), splits
    # a query whose best row is one of the copied ones: the lower copy must come first
    fq = np.concatenate([bank[:2], f[:3]])
    s64 = sb.similarities(fq, bank)
    good = sb.restate_fp32(fq, bank, 1.0, 3, topk=8)["idx"]
    bad = sb.restate_fp32(fq, bank, 1.0, 3, topk=8, tie_high=True)["idx"]
    assert good[0, :2].tolist() == [0, K // 2] and good[1, :2].tolist() == [1, K - 1]
    assert np.array_equal(good, sb.topk_reference(s64, 1.0, 8)[0]) and not np.array_equal(bad, good)


def test_var_budget_is_absolute_where_the_softmax_is_uniform():
    """Identical bank rows: the softmax is uniform, var is 0 in exact arithmetic and the budget must still leave room for the
    rounding of Q / Z^2 — and no more than rel_Q + 2 rel_Z (about 3 K u here) of 1 / K^2 plus the smallest fp32 step."""
    B, K = 3, 300
    f, bank = sb.lattice_case(B, K, P, seed=1)
    bank[:] = bank[0]
    s64 = sb.similarities(f, bank)
    ref = sb.reference_from_similarities(s64, 1.0)
    bud = sb.budgets_from_similarities(s64, np.zeros_like(s64), 1.0)
    assert np.abs(ref["var"]).max() <= 4 * sb.U64 / K ** 2
    assert (bud["var"] > 0).all() and (bud["var"] <= (3 * K + 400) * sb.U64 / K ** 2 + 3 * float(np.finfo(np.float32).tiny)).all()
    for splits in SPLITS:
        got = sb.restate_fp32(f, bank, 1.0, splits)
        assert sb.worst_ratio(got, ref, bud)[0] <= 1.0, splits


def test_topk_past_the_bank_and_nan_rows():
    B, K = 3, 5
    f, bank = sb.lattice_case(B, K, P, seed=2)
    bank[3] = np.nan
    s32 = (f.astype(np.float64) @ np.nan_to_num(bank).astype(np.float64).T).astype(np.float32)
    s32[:, 3] = np.nan
    got = sb.restate_fp32(f, bank, 1.0, 2, topk=8, sims=s32)
    idx, prob = sb.topk_reference(s32.astype(np.float64), 1.0, 8)
    assert np.array_equal(got["idx"], idx) and (got["idx"][:, 4:] == -1).all() and not (got["idx"] == 3).any()
    assert np.isnan(got["prob"]).all() and all(np.isnan(got[k]).all() for k in sb.KINDS)
