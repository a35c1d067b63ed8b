"""The NegLabel budget of tests/neglabel_budget.py is neither vacuous nor out of reach: a numpy restatement of the two kernels
(fp32 similarities, tiles, splits, fp32 pairs) passes it on lattice and on unit inputs, and each of five deliberate mistakes
fails it on inputs where it provably must.  CPU only."""
import numpy as np
import pytest

from tests import neglabel_budget as nb

SHAPE = (65, 37, 7, 100)      # B, K, G, gs: N = 737 = two full tiles and a ragged one of 225 rows; groups cross both tile edges


def _ratios(got, f, bank, K, G, gs, T):
    S, score, _ = nb.reference(f, bank, K, G, gs, T)
    bS, bs = nb.budgets(f, bank, K, G, gs, T)
    return nb.ratio(got[1], S, bS), nb.ratio(got[0], score, bs)


@pytest.mark.parametrize("P", [64, 512])
@pytest.mark.parametrize("T", [0.01, 1.0])
def test_restatement_passes_on_lattice_inputs(P, T):
    B, K, G, gs = SHAPE
    f, bank = nb.lattice_case(B, K, G, gs, P, seed=P)
    S, score, _ = nb.reference(f, bank, K, G, gs, T)
    bS, bs = nb.budgets(f, bank, K, G, gs, T, exact=True)     # exact similarities: the arithmetic term and the ulp alone
    for splits in (1, 2, 7):
        sc, Sg = nb.restate_fp32(f, bank, K, G, gs, T, splits)
        rS, rs = nb.ratio(Sg, S, bS), nb.ratio(sc, score, bs)
        assert rS <= 1.0 and rs <= 1.0, (P, T, splits, rS, rs)


@pytest.mark.parametrize("P", [64, 512])
@pytest.mark.parametrize("T", [0.01, 1.0])
def test_restatement_passes_on_unit_inputs(P, T):
    B, K, G, gs = SHAPE
    f, bank = nb.unit_case(B, K, G, gs, P, seed=P)
    S, _, _ = nb.reference(f, bank, K, G, gs, T)
    if T == 0.01:
        assert S.min() < 1e-4 and S.max() > 0.999           # the planted queries spread S over its range
    for splits in (1, 2, 7):
        rS, rs = _ratios(nb.restate_fp32(f, bank, K, G, gs, T, splits), f, bank, K, G, gs, T)
        assert rS <= 1.0 and rs <= 1.0, (P, T, splits, rS, rs)


def test_small_and_edge_shapes_pass():
    for B, K, G, gs in [(1, 1, 1, 1), (3, 300, 1, 1), (5, 257, 100, 3), (4, 1000, 3, 301)]:
        f, bank = nb.unit_case(B, K, G, gs, 64, seed=K)
        for splits in (1, 2, 7):
            rS, rs = _ratios(nb.restate_fp32(f, bank, K, G, gs, 0.01, splits), f, bank, K, G, gs, 0.01)
            assert rS <= 1.0 and rs <= 1.0, (B, K, G, gs, splits, rS, rs)


MISTAKES = {
    # a query pulled toward bank row K (the first negative) has S[., 0] near 0; with the boundary one row later that row is ID
    "boundaries shifted by one row": dict(shift=1),
    # a query pulled toward the bank's last row (in the ragged tile of 225 rows) loses that row from its last group
    "ragged last tile dropped": dict(drop_ragged=True),
    # G = 7 > 1: the pooled negatives outweigh every single group, so the pooled mass is below the mean of the group masses
    "one softmax over all negatives": dict(pooled=True),
    # T = 0.01 against T = 1: logits a hundred times smaller
    "T ignored": dict(use_T=False),
}


@pytest.mark.parametrize("name", list(MISTAKES))
def test_each_mistake_fails_the_budget(name):
    B, K, G, gs = SHAPE
    f, bank = nb.unit_case(B, K, G, gs, 64, seed=64)
    got = nb.restate_fp32(f, bank, K, G, gs, 0.01, 2, **MISTAKES[name])
    rS, rs = _ratios(got, f, bank, K, G, gs, 0.01)
    print(f"{name}: ratio to the budget, groups {rS:.3g}, scores {rs:.3g}")
    assert rS > 1.0 and rs > 1.0, (name, rS, rs)


def test_bf16_rounded_operands_fail_the_budget_at_p64():
    B, K, G, gs = SHAPE
    f, bank = nb.unit_case(B, K, G, gs, 64, seed=64)
    sims = (nb.bf16_round(f) @ nb.bf16_round(bank).T).astype(np.float32)
    got = nb.restate_fp32(f, bank, K, G, gs, 0.01, 1, sims=sims)
    rS, rs = _ratios(got, f, bank, K, G, gs, 0.01)
    print(f"bf16 operands, P = 64, T = 0.01: ratio to the budget, groups {rS:.3g}, scores {rs:.3g}")
    assert rS > 1.0 and rs > 1.0, (rS, rs)
