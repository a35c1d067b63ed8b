"""The budget of GL-MCM's local score (tests/glmcm_budget.py) on the CPU: the numpy restatement of the two kernels stays inside
it on lattice and planted inputs, the planted cells are where they are meant to be, and every deliberate mistake leaves it."""
import numpy as np
import pytest

from tests import glmcm_budget as gb

B, R, K, P = 6, 49, 300, 64   # images straddle the 64-row query tiles (rows 49, 98, ...), K crosses the 256-row bank tile


def _ratios(got_score, got_patch, local, text, T, exact=False):
    patch, score = gb.reference(local, text, T)
    b_patch, b_score = gb.budgets(local, text, T, exact=exact)
    return gb.ratio(got_score, score, b_score), gb.ratio(got_patch, patch, b_patch)


def test_plants_cover_every_edge():
    pl = gb.plants(B, R, K)
    assert pl[0] == (0, 0) and pl[1] == (R - 1, 255)                       # first / last patch of an image
    assert (2 * R + pl[2][0]) % 64 == 63 and (3 * R + pl[3][0]) % 64 == 0  # either side of a query-tile edge
    assert pl[2][1] == 256 and pl[3][1] == K - 1
    assert pl[-1] == (R - 1, K - 1)                                        # the last image's last patch, the last prompt
    local, text, _cls, _scale = gb.unit_case(B, R, K, P, 0)
    s = gb.similarities(local, text)
    for b, (i, k) in enumerate(pl):                                        # a single cell decides S_L
        assert np.unravel_index(np.argmax(s[b]), s[b].shape) == (i, k)
        patch, _ = gb.reference(local[b:b + 1], text, 1.0)
        assert int(np.argmax(patch[0])) == i


@pytest.mark.parametrize("T", [1.0, 0.01])
def test_restatement_is_inside_the_budget(T):
    local, text = gb.lattice_case(B, R, K, P, 1)
    score, patch = gb.restate_fp32(local, text, T)
    rs, rp = _ratios(score, patch, local, text, T, exact=True)
    print(f"BUDGET glmcm restatement lattice T={T}: score {rs:.3f} patch {rp:.3f}")
    assert rs <= 1.0 and rp <= 1.0
    local, text, _cls, _scale = gb.unit_case(B, R, K, P, 2)
    score, patch = gb.restate_fp32(local, text, T)
    rs, rp = _ratios(score, patch, local, text, T)
    print(f"BUDGET glmcm restatement unit T={T}: score {rs:.3f} patch {rp:.3f}")
    assert rs <= 1.0 and rp <= 1.0
    assert np.array_equal(score, -patch.max(axis=1))


@pytest.mark.parametrize("mistake,T", [("cls", 1.0), ("mean", 1.0), ("t_after", 0.01), ("scale", 1.0), ("first_tile_only", 1.0),
                                       ("neighbour", 1.0)])
def test_deliberate_mistakes_leave_the_budget(mistake, T):
    local, text, cls, scale = gb.unit_case(B, R, K, P, 2)
    kw = {"cls": {"cls": cls}, "mean": {"mean": True}, "t_after": {"t_after": True}, "scale": {"scale": scale},
          "first_tile_only": {"first_tile_only": True}, "neighbour": {"neighbour": True}}[mistake]
    score, _patch = gb.restate_fp32(local, text, T, **kw)
    rs, _ = _ratios(score, np.zeros((B, R)), local, text, T)
    print(f"BUDGET glmcm mistake {mistake} T={T}: score ratio {rs:.3g}")
    assert rs > 1.0


def test_budget_has_no_similarity_term_on_the_lattice():
    local, text = gb.lattice_case(2, 5, 7, 64, 3)
    bp, _ = gb.budgets(local, text, 1.0, exact=True)
    patch, _ = gb.reference(local, text, 1.0)
    assert (bp < 3 * np.spacing(patch.astype(np.float32))).all()          # one ulp and a little arithmetic, nothing else
