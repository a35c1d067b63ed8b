"""The evaluation tail on the device against exact references: mcm_measures (metrics.hip count_kernel / measures_kernel) vs
tests/eval_reference.py, mcm_score_histogram (hist_kernel) vs numpy.histogram, and the Mahalanobis pair (score.hip
maha_prepare_kernel / maha_score_kernel) vs the fp64 direct form under tests/error_budget.py's maha_budget.

Measures: AUROC and FPR are single fp64 divisions of exact integers on both sides, so they must be BIT-EQUAL; AUPR is an fp64
sum of n_pos terms and must be within eval_reference.aupr_bound(n_pos).  -inf / +inf are ordered scores; a NaN anywhere makes
all three outputs NaN (include/mcm.h).  Each measures case prints "BUDGET aupr fp64 <|d| / bound>", each Mahalanobis case
"BUDGET maha fp64 <max |got - ref| / budget>" (run with -s to collect them)."""
import math

import numpy as np
import pytest

from tests import error_budget as eb
from tests import eval_reference as er
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gs.dev

INF = np.float32(np.inf)
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def net():
    n = gs.widened_net()
    yield n
    n.close()


def _check_measures(net, pos, neg, level=0.95, negate=False, where="", dev=None):
    """Device vs exact.  With negate the device evaluates -score: the reference gets the negated vectors."""
    pos, neg = np.asarray(pos, np.float32), np.asarray(neg, np.float32)
    dpos, dneg = dev if dev is not None else (_dev(pos), _dev(neg))
    got = net.measures(dpos, dneg, recall_level=level, negate=negate)
    want = er.measures_exact(-pos, -neg, level) if negate else er.measures_exact(pos, neg, level)
    bound = er.aupr_bound(pos.size)
    print(f"BUDGET aupr fp64 {abs(got[1] - want[1]) / bound:.3f} n_pos={pos.size} n_neg={neg.size} {where}")
    assert got[0] == want[0], ("auroc", where, got, want)
    assert got[2] == want[2], ("fpr", where, got, want)
    assert abs(got[1] - want[1]) <= bound, ("aupr", where, got, want, bound)
    return got


def _scores(n_pos, n_neg, quant, seed):
    rng = np.random.default_rng(seed)
    pos = rng.normal(0.6, 1.0, n_pos).astype(np.float32)
    neg = rng.normal(-0.4, 1.2, n_neg).astype(np.float32)
    if quant:                    # about 16 levels over the bulk of the two distributions
        pos, neg = np.round(pos * 3).astype(np.float32) / 3, np.round(neg * 3).astype(np.float32) / 3
    return pos, neg


# ---- measures: tile and block edges ------------------------------------------------------------------------------------------
EDGES = [1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193]   # CT = 256 examples per workgroup, TILE = 4096 staged values
# each edge size for n_pos and for n_neg against a ragged partner, then totals that are multiples of CT = 256 and of RT = 1024
# (255 + 1, 4095 + 1, 257 + 767, 8193 + 8191) and tile multiples on both sides
SIZES = ([(s, 300) for s in EDGES] + [(300, s) for s in EDGES]
         + [(255, 1), (1, 255), (4095, 1), (257, 767), (8193, 8191), (8192, 8192), (8193, 8193)])


@pytest.mark.parametrize("quant", [0, 1], ids=["random", "quantised"])
@pytest.mark.parametrize("n_pos,n_neg", SIZES)
def test_measures_exact_at_tile_and_block_edges(net, n_pos, n_neg, quant):
    pos, neg = _scores(n_pos, n_neg, quant, 31 * n_pos + n_neg)
    _check_measures(net, pos, neg, where=f"quant={quant}")


# ---- measures: infinities are ordered values -----------------------------------------------------------------------------------
@pytest.mark.parametrize("negate", [False, True], ids=["plain", "negate"])
@pytest.mark.parametrize("n_pos,n_neg", [(1237, 4099), (4096, 8192)], ids=["ragged", "tiles"])
@pytest.mark.parametrize("side", ["pos", "neg", "both"])
@pytest.mark.parametrize("value", [-INF, INF], ids=["minus_inf", "plus_inf"])
def test_measures_infinities_are_ordered_values(net, value, side, n_pos, n_neg, negate):
    """A -inf score (after the sign flip) used to match every -inf pad of a ragged tile: tp / fp over-counted by the pad
    length and 2 n_neg - fp - gt wrapped.  Visible when the infinity is among the positives at a ragged size."""
    pos, neg = _scores(n_pos, n_neg, 0, 5)
    if side in ("pos", "both"):
        pos[[0, n_pos // 2, n_pos - 1]] = value
    if side in ("neg", "both"):
        neg[[0, n_neg // 3, n_neg - 1]] = value
    _check_measures(net, pos, neg, negate=negate, where=f"{value} in {side} negate={negate}")


# ---- measures: NaN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negate", [False, True], ids=["plain", "negate"])
@pytest.mark.parametrize("side,index", [("pos", 0), ("pos", -1), ("pos", 4095), ("pos", 4096),
                                        ("neg", 0), ("neg", -1), ("neg", 4095), ("neg", 4096)])
def test_measures_nan_gives_nan(net, side, index, negate):
    pos, neg = _scores(4097, 4099, 0, 9)
    (pos if side == "pos" else neg)[index] = np.nan
    got = net.measures(_dev(pos), _dev(neg), negate=negate)
    assert all(math.isnan(v) for v in got), got
    assert all(math.isnan(v) for v in er.measures_exact(pos, neg))


def test_measures_nan_only_value(net):
    got = net.measures(_dev([np.nan]), _dev([0.0]))
    assert all(math.isnan(v) for v in got), got
    got = net.measures(_dev([0.0]), _dev([np.nan, np.nan]))
    assert all(math.isnan(v) for v in got), got


# ---- measures: values at the edges of the format -----------------------------------------------------------------------------------
def test_measures_signed_zeros_tie(net):
    rng = np.random.default_rng(3)
    pos = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), 700)
    neg = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), 900)
    a = _check_measures(net, pos, neg, where="signed zeros")
    b = _check_measures(net, pos + np.float32(0.0), neg + np.float32(0.0), where="zeros made positive")
    assert a == b
    assert _check_measures(net, [-0.0], [0.0])[0] == 0.5
    assert _check_measures(net, [-0.0], [0.0], negate=True)[0] == 0.5


def test_measures_subnormals_stay_distinct(net):
    """Scores that differ only below 2^-126: a build that flushes denormals would see one big tie at zero."""
    rng = np.random.default_rng(4)
    tiny = np.float32(2.0 ** -149)
    pos = (rng.integers(-40, 60, 513) * tiny).astype(np.float32)
    neg = (rng.integers(-60, 40, 700) * tiny).astype(np.float32)
    assert np.abs(pos).max() < 2.0 ** -126 and np.unique(pos).size > 50
    flushed = er.measures_exact(np.zeros_like(pos), np.zeros_like(neg))
    for negate in (False, True):
        got = _check_measures(net, pos, neg, negate=negate, where=f"subnormal negate={negate}")
        assert got[0] != flushed[0]
    assert _check_measures(net, [2 * tiny], [tiny]) == (1.0, 1.0, 0.0)


def test_measures_at_flt_max(net):
    rng = np.random.default_rng(6)
    vals = np.array([-INF, -FLT_MAX, np.nextafter(-FLT_MAX, np.float32(0)), -1.0, 0.0, 1.0,
                     np.nextafter(FLT_MAX, np.float32(0)), FLT_MAX, INF], np.float32)
    pos, neg = rng.choice(vals, 1237), rng.choice(vals, 300)
    for negate in (False, True):
        _check_measures(net, pos, neg, negate=negate, where=f"flt_max negate={negate}")


# ---- measures: recall levels, degenerate orders ------------------------------------------------------------------------------------
def test_measures_recall_levels_and_exact_ties(net):
    """n_pos = 256: every recall k / 256 and every midpoint between two of them is exact in fp64, so |recall - level| ties
    for real and the lowest threshold must win."""
    pos, neg = _scores(256, 333, 1, 8)
    dev = (_dev(pos), _dev(neg))
    ts = np.unique(pos)
    tp = sorted({int((pos >= t).sum()) for t in ts})
    levels = [0.0, 1.0] + [k / 256 for k in tp] + [(a + b) / 2 / 256 for a, b in zip(tp, tp[1:])] + [1 / 256, 255 / 256]
    fprs = set()
    for level in levels:
        fprs.add(_check_measures(net, pos, neg, level=level, where=f"level={level}", dev=dev)[2])
    assert len(fprs) > 5                                   # the levels really pick different operating points
    tied = [lv for lv in levels if er.measures_exact(pos, neg, lv)[2] != er.measures_exact(pos, neg, lv, _highest_tie=True)[2]]
    assert len(tied) > 5                                   # and the tie rule matters at them


@pytest.mark.parametrize("level", [0.0, 0.5, 0.95, 1.0])
def test_measures_all_equal_and_separated(net, level):
    same_p, same_n = np.full(1237, 0.25, np.float32), np.full(4099, 0.25, np.float32)
    assert _check_measures(net, same_p, same_n, level=level, where="all equal")[0] == 0.5
    rng = np.random.default_rng(1)
    hi, lo = rng.uniform(1, 2, 4097).astype(np.float32), rng.uniform(-2, -1, 1237).astype(np.float32)
    assert _check_measures(net, hi, lo, level=level, where="separated")[0] == 1.0
    assert _check_measures(net, lo, hi, level=level, where="separated, reversed")[0] == 0.0
    assert _check_measures(net, hi, lo, level=level, negate=True, where="separated, negated")[0] == 0.0


def test_measures_on_views_at_an_odd_offset(net):
    """pos = buf[1:]: a 4-byte offset into a larger allocation (the kernels read scalars, no 16-byte alignment needed)."""
    pos, neg = _scores(4098, 1238, 0, 12)
    bp, bn = _dev(pos), _dev(neg)
    vp, vn = bp[1:], bn[1:]
    assert vp.data_ptr() % 16 == 4 and vn.data_ptr() % 16 == 4 and vp.is_contiguous()
    _check_measures(net, pos[1:], neg[1:], where="views", dev=(vp, vn))
    _check_measures(net, pos[1:], neg, where="one view", dev=(vp, bn))


# ---- histogram ---------------------------------------------------------------------------------------------------------------------
def _edges(nb, seed=0):
    """nb + 1 strictly increasing, non-uniform fp32 edges over about [-3, 3]."""
    rng = np.random.default_rng(seed + nb)
    e = np.cumsum(rng.uniform(0.2, 1.8, nb + 1))
    e = (-3.0 + 6.0 * (e - e[0]) / max(e[-1] - e[0], 1e-9)).astype(np.float32)
    assert nb > 4096 or (np.diff(e) > 0).all()
    return np.sort(e)


def _check_hist(net, x, edges, where=""):
    x, edges = np.asarray(x, np.float32), np.asarray(edges, np.float32)
    got = net.histogram(_dev(x) if x.size else torch.empty(0, device="cuda"), edges).cpu().numpy()
    want = np.histogram(x, bins=edges)[0]
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (where, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return got


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 262144, 262145, 1000003])
def test_histogram_sizes(net, n):
    """The grid is 1024 workgroups of 256: 262 144 values fill it exactly, one more starts the grid-stride loop's second trip."""
    x = np.random.default_rng(n).normal(0, 1.5, n).astype(np.float32)
    got = _check_hist(net, x, _edges(64), f"n={n}")
    assert got.sum() <= n


@pytest.mark.parametrize("nb", [1, 2, 255, 256, 257, 8192])
def test_histogram_bin_counts(net, nb):
    x = np.random.default_rng(nb).normal(0, 1.5, 20011).astype(np.float32)
    _check_hist(net, x, _edges(nb), f"nb={nb}")


def test_histogram_refuses_more_than_8192_bins(net):
    x = _dev(np.zeros(10, np.float32))
    with pytest.raises(RuntimeError):
        net.histogram(x, np.linspace(-1, 1, 8194).astype(np.float32))
    torch.cuda.synchronize()


def test_histogram_edge_values(net):
    rng = np.random.default_rng(2)
    e = _edges(257)
    x = rng.normal(0, 1.5, 5000).astype(np.float32)
    # every edge value itself, and one fp32 ulp below and above the first and the last edge
    x = np.concatenate([x, e, e, [np.nextafter(e[0], -INF), np.nextafter(e[0], INF), np.nextafter(e[-1], -INF),
                                  np.nextafter(e[-1], INF)]]).astype(np.float32)
    _check_hist(net, rng.permutation(x), e, "edge values")


def test_histogram_repeated_edges(net):
    rng = np.random.default_rng(3)
    e = np.array([-2, -1, -1, 0, 0.5, 0.5, 0.5, 1, 2, 2], np.float32)       # zero-width bins, the last edge repeated
    x = np.concatenate([rng.choice(e, 4000), rng.normal(0, 1.5, 4000).astype(np.float32), np.full(100, 2, np.float32)])
    got = _check_hist(net, x, e, "repeated edges")
    assert got[1] == 0 and got[-1] >= 100
    e0 = np.array([-1, -1, 0, 1], np.float32)                                 # the first edge repeated
    _check_hist(net, np.concatenate([rng.choice(e0, 1000), [-1.0] * 10]), e0, "repeated first edge")


def test_histogram_nonfinite_values_are_dropped_as_numpy_drops_them(net):
    """numpy.histogram with explicit bins counts by searchsorted on the sorted data: -inf sorts before the first edge, +inf
    and NaN after the last, none is counted and nothing raises.  The device does the same."""
    rng = np.random.default_rng(4)
    x = rng.normal(0, 1.5, 3000).astype(np.float32)
    x[rng.integers(0, 3000, 300)] = rng.choice(np.array([np.nan, INF, -INF], np.float32), 300)
    e = _edges(33)
    assert np.histogram(np.array([np.nan, INF, -INF, 0.0], np.float32), bins=e)[0].sum() == 1
    got = _check_hist(net, x, e, "non-finite")
    assert got.sum() < 3000
    _check_hist(net, np.array([np.nan, INF, -INF], np.float32), e, "only non-finite")


def test_histogram_everything_in_one_bin_and_everything_outside(net):
    e = _edges(256)
    n = 1000003                                        # 10^6 LDS atomics on one address
    mid = np.float32((e[100] + e[101]) / 2)
    got = _check_hist(net, np.full(n, mid, np.float32), e, "one bin")
    assert got[100] == n
    got = _check_hist(net, np.full(n, e[-1], np.float32), e, "the closed last edge")
    assert got[-1] == n
    got = _check_hist(net, np.concatenate([np.full(5000, 4.0, np.float32), np.full(5000, -4.0, np.float32)]), e, "all outside")
    assert got.sum() == 0


def test_histogram_second_call_rezeroes_the_counts(net):
    """Through the C ABI with one caller-owned output tensor: the second call's counts replace the first's."""
    e = _edges(64)
    xs = [np.random.default_rng(s).normal(0, 1.5, 70001).astype(np.float32) for s in (1, 2)]
    out = torch.full((64,), 12345, device="cuda", dtype=torch.int64)      # dirty to begin with
    from mcm_amd.engine import _stream_ptr

    ed = _dev(e)
    for x in xs:
        xd = _dev(x)
        net._check(net._lib.mcm_score_histogram(net._h, xd.data_ptr(), xd.numel(), ed.data_ptr(), 64, out.data_ptr(),
                                                 _stream_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), np.histogram(x, bins=e)[0])


# ---- Mahalanobis under the fp64 budget ---------------------------------------------------------------------------------------------
# proj_dim must be a multiple of 4 (mcm_create); 100 is the width that is no multiple of 64 (the wave's stride over a row)
MAHA_WIDTHS = [64, 100, 512, 768]


@pytest.fixture(scope="module")
def maha_nets():
    yield from gs.net_cache()


@pytest.mark.parametrize("pkind", ["asym", "scaled"])
@pytest.mark.parametrize("P", MAHA_WIDTHS)
def test_maha_within_budget(maha_nets, P, pkind):
    """C = 1 and 15: whole waves of the 16 see no class and contribute +inf to the minimum; 17: one wave sees two.  Rows of
    the near / equal kinds start at the LAST class.  B = 33 mixes far / near / equal rows; B = 1 runs each kind alone."""
    mnet = maha_nets(P)
    assert mnet.geo.proj_dim == P
    for C in (1, 15, 16, 17, 1000):
        state = None
        for B, where in ((33, "mixed"), (1, "far"), (1, "near"), (1, "equal")):
            feats, means, prec = eb.maha_case(P, C, B, where, pkind)      # means, prec: the same for every (B, where)
            if state is None:
                state = mnet.maha_prepare(_dev(means), _dev(prec))
            got = mnet.maha_scores(_dev(feats), state).cpu().numpy()
            ref, bud = eb.maha_budget(feats, means, prec)
            if where == "equal":
                assert (ref == 0.0).all()
            r, i = eb.worst(got, ref, bud)
            print(f"BUDGET maha fp64 {r:.3f} P={P} C={C} B={B} {where} {pkind}")
            assert np.isfinite(got).all()
            assert r <= 1.0, (P, C, B, where, pkind, r, got[i], ref[i], bud[i])

