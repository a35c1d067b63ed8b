"""CPU proof of tests/maha_fit_budget.py: a correct row-sequential emulation of the device Mahalanobis fit stays inside the
covariance budget, a list of plausible mistakes does not, and n = 1 ends in a non-finite covariance, not in a crash."""
import numpy as np
import pytest

from tests import maha_fit_budget as fb

CASES = [(P, n, off) for P in (8, 64, 100) for n in (2, 67, 1100) for off in (0.0, 20.0)]


def _shift(x, use):
    return fb.first_batch_shift(x) if use else None


@pytest.mark.parametrize("use_shift", [False, True], ids=["noshift", "shift"])
@pytest.mark.parametrize("P,n,off", CASES)
def test_emulation_within_budget(P, n, off, use_shift):
    x = fb.fit_case(n, P, off)
    shift = _shift(x, use_shift)
    r, i = fb.cov_ratio(fb.emulate_fit(x, shift), x, shift)
    print(f"BUDGET maha-fit emulation {r:.3f} P={P} n={n} offset={off} shift={use_shift}")
    assert r <= 1.0, (P, n, off, use_shift, r, i)


@pytest.mark.parametrize("P,n,off", [(8, 67, 0.0), (100, 1100, 20.0)])
def test_torch_cov_within_budget(P, n, off):
    """The host route's own covariance (torch.cov on the fp64 rows) under the same budget: the two routes are then within
    twice the budget of each other."""
    torch = pytest.importorskip("torch")
    x = fb.fit_case(n, P, off)
    got = torch.cov(torch.from_numpy(x).T.double()).numpy()
    r, _ = fb.cov_ratio(got, x, fb.first_batch_shift(x))
    print(f"BUDGET maha-fit torch.cov {r:.3f} P={P} n={n} offset={off}")
    assert r <= 1.0


@pytest.mark.parametrize("mutation", ["fp32", "sum_unshifted", "div_n"])
@pytest.mark.parametrize("P,n,off", CASES)
def test_mutations_break_the_budget(P, n, off, mutation):
    """Each mistake, on every case it applies to (dropping the shift from sum needs a shift to drop)."""
    x = fb.fit_case(n, P, off)
    for use_shift in ((True,) if mutation == "sum_unshifted" else (False, True)):
        shift = _shift(x, use_shift)
        r, _ = fb.cov_ratio(fb.emulate_fit(x, shift, mutation), x, shift)
        assert r > 1.0, (mutation, P, n, off, use_shift, r)


@pytest.mark.parametrize("use_shift", [False, True], ids=["noshift", "shift"])
@pytest.mark.parametrize("P", [8, 64, 100])
def test_one_sample_gives_a_non_finite_covariance(P, use_shift):
    for off in (0.0, 20.0):
        x = fb.fit_case(1, P, off)
        cov = fb.emulate_fit(x, _shift(x, use_shift))
        ref, _ = fb.cov_reference(x)
        assert cov.shape == (P, P) and not np.isfinite(cov).any()
        assert not np.isfinite(np.asarray(ref, np.float64)[~np.isnan(np.asarray(ref, np.float64))]).any()
        assert np.isnan(np.asarray(ref, np.float64)).all()          # 0 / 0 everywhere
        fb.cov_budget(x, _shift(x, use_shift))                      # and the budget itself does not raise


def test_shift_is_what_keeps_the_precision(capsys):
    """The reason for the shift, on the CPU: columns 20 sigma from the origin.  Without the shift the inverted covariance
    moves by orders of magnitude more than with it, and with it the precision bound stays below 1e-8 of max |precision|."""
    x = fb.fit_case(1100, 64, 20.0)
    ref, own = fb.cov_reference(x)
    moved = {}
    for use_shift in (False, True):
        shift = _shift(x, use_shift)
        cov = fb.emulate_fit(x, shift)
        prec_ref, bound = fb.precision_bound(ref, fb.cov_budget(x, shift) + own)
        got = np.linalg.inv(cov).astype(np.float32)
        moved[use_shift] = float(np.abs(np.linalg.inv(cov) - prec_ref).max() / np.abs(prec_ref).max())
        assert (np.abs(got - prec_ref) <= bound).all()
        if use_shift:
            assert np.linalg.cond(np.asarray(ref, np.float64)) <= 2e3
            assert float((bound - 0.5 * fb.ulp(prec_ref, "fp32")).max()) < 1e-8 * np.abs(prec_ref).max()
    print(f"precision moved by {moved[False]:.1e} without the shift, {moved[True]:.1e} with it (relative to max |precision|)")
    assert moved[True] < moved[False]
