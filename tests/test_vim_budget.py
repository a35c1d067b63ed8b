"""The ViM budget of tests/vim_budget.py is neither vacuous nor out of reach: a numpy restatement of the two kernels (fp32
similarities, tiles cut at row K, splits, 16-byte slots) passes it on lattice and on unit inputs at every shape the GPU test
uses, and each of six deliberate mistakes fails it on inputs where it provably must.  CPU only."""
import numpy as np
import pytest

from tests import vim_budget as vb

# (B, K, R) of tests/test_gpu_vim.py, with fewer queries where they only repeat
SHAPES = [(1, 1, 1), (3, 300, 1), (8, 255, 2), (12, 256, 256), (12, 257, 3), (8, 1, 300), (12, 1000, 256)]
SPLITS = [1, 2, 3, 32]
ALPHA = 1.75


def _worst(got, f, bank, K, off, T, exact=False):
    return vb.worst_ratio(got, vb.reference(f, bank, K, off, T, ALPHA), vb.budgets(f, bank, K, off, T, ALPHA, exact=exact))


@pytest.mark.parametrize("P", [4, 36, 64, 512])
def test_restatement_passes_on_lattice_inputs(P):
    for B, K, R in SHAPES:
        f, bank = vb.lattice_case(B, K, R, P, seed=K + R)
        for off in (None, vb.lattice_off(R, seed=R)):
            for T in (0.01, 1.0):
                for splits in SPLITS:
                    r = _worst(vb.restate_fp32(f, bank, K, off, T, ALPHA, splits), f, bank, K, off, T, exact=True)
                    assert r <= 1.0, (P, B, K, R, off is not None, T, splits, r)


@pytest.mark.parametrize("P", [64, 512])
def test_restatement_passes_on_unit_inputs(P):
    for B, K, R in SHAPES:
        f, bank = vb.unit_case(B, K, R, P, seed=P + K)
        ref = vb.reference(f, bank, K, None, 0.01, ALPHA)
        if R <= 4 and B >= 2:
            assert (ref["resid"][:2] == 0.0).all()             # the rows that lie exactly in the principal space
        off = vb.similarities(f[-1:], bank[K:])[0]             # the projections of the last query
        for o in (None, off):
            for splits in SPLITS:
                got = vb.restate_fp32(f, bank, K, o, 0.01, ALPHA, splits)
                r = _worst(got, f, bank, K, o, 0.01)
                assert r <= 1.0, (P, B, K, R, o is not None, splits, r)
                if o is None and R <= 4 and B >= 2:
                    assert (got["resid"][:2] == 0.0).all()


# Every mistake is run on the inputs where it provably shows.  B, K, R = 12, 300, 300 in two splits of 300 rows: the split
# boundary falls exactly at K, each split is a full tile and a ragged one of 44 rows; in three splits of 200 rows one boundary
# lies inside the prompts and one inside the basis.
MISTAKES = {
    # lattice inputs: the terms are multiples of 2^-44 below 2^-8 and their sum needs about 40 bits: an fp32 accumulator rounds
    # every addition to 24, and the budget there is the fp64 arithmetic term plus one fp32 ulp of the result
    "ssq accumulated in fp32": ("lattice", 2, dict(ssq_fp32=True)),
    # off = the projections of the last query: its resid is 0 with off and about 0.7 without
    "off ignored": ("unit", 2, dict(ignore_off=True)),
    # query 3 is pulled toward prompt K - 1 (cosine 0.8, T = 0.01): counted as a basis row it leaves the log-sum-exp (about 80
    # logit units above the rest) and enters the residual
    "the last prompt counted as a basis row": ("unit", 2, dict(shift=-1)),
    # query 3's prompt K - 1 lies in the ragged tile of the first split, and every query loses 44 basis rows
    "ragged last tile dropped": ("unit", 2, dict(drop_ragged=True)),
    # three splits of 200 rows: queries 2 and 3 have their dominant prompt in one split, the other split's sum is relative to a
    # maximum tens of logit units below: added as it is it is counted e^(tens) times too large
    "split pairs merged without rescaling": ("unit", 3, dict(no_rescale=True)),
    # resid is about 0.7 on unit rows (half of the energy lies outside the principal space), its square about 0.5
    "sqrt omitted": ("unit", 2, dict(no_sqrt=True)),
}


@pytest.mark.parametrize("name", list(MISTAKES))
def test_each_mistake_fails_the_budget(name):
    kind, splits, switch = MISTAKES[name]
    B, K, R, P, T = 12, 300, 300, 64, 0.01
    if kind == "lattice":
        f, bank = vb.lattice_case(B, K, R, P, seed=7)
        off = None
    else:
        f, bank = vb.unit_case(B, K, R, P, seed=7)
        off = vb.similarities(f[-1:], bank[K:])[0]
    right = _worst(vb.restate_fp32(f, bank, K, off, T, ALPHA, splits), f, bank, K, off, T, exact=kind == "lattice")
    wrong = _worst(vb.restate_fp32(f, bank, K, off, T, ALPHA, splits, **switch), f, bank, K, off, T, exact=kind == "lattice")
    print(f"{name}: ratio to the budget {wrong:.3g} (the faithful restatement: {right:.3g})")
    assert right <= 1.0 and wrong > 1.0, (name, right, wrong)


def test_bf16_rounded_operands_fail_the_budget_at_p64():
    B, K, R = 12, 300, 300
    f, bank = vb.unit_case(B, K, R, 64, seed=7)
    sims = (vb_bf16(f) @ vb_bf16(bank).T).astype(np.float32)
    r = _worst(vb.restate_fp32(f, bank, K, None, 0.01, ALPHA, 1, sims=sims), f, bank, K, None, 0.01)
    print(f"bf16 operands, P = 64, T = 0.01: ratio to the budget {r:.3g}")
    assert r > 1.0, r


def vb_bf16(x):
    from tests.knn_budget import bf16_round

    return bf16_round(x)
