"""The top-k form of the fused scoring tail (score_kernel<true>, include/mcm.h mcm_score_features_topk / mcm_score_topk) on
a real MI355X: which concepts an image matched, in what order, with what probability — and the scores left bit for bit
what the plain tail writes.

Order is held to EXACT index equality with numpy.argsort(-(f64 @ t64.T), kind="stable").  That is decidable because the
inputs are chosen (seeds picked on the CPU, asserted on the host before the GPU is touched) so that every gap among the
top `topk + 1` fp64 similarities of every row exceeds 2 gamma_P, gamma_P = P u / (1 - P u), u = 2^-24: an fp32 dot product
of unit vectors is within gamma_P of the exact one in any summation order, so two similarities further apart than 2 gamma_P
cannot swap.
"""
import ctypes

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MCM_EINVAL = -1
PS = (64, 512, 1024)
KS = (1, 15, 16, 17, 1023, 1024, 1025, 2049)   # the 16-wave stride, the 1024-thread stride, more than two passes
TOPKS = (1, 5, 8)
BS = (1, 3)
# (P, K, B) -> seed of the case, where seed 0 leaves a gap of the top 9 similarities within 2 gamma_P (found on the CPU)
SEEDS = {(64, 1024, 3): 1, (512, 16, 3): 1, (512, 17, 1): 1, (512, 1023, 3): 1, (512, 1024, 3): 2, (512, 2049, 3): 1,
         (1024, 15, 1): 1, (1024, 16, 3): 1, (1024, 1023, 1): 1, (1024, 1024, 1): 2, (1024, 1025, 1): 2,
         (1024, 1025, 3): 1, (1024, 2049, 1): 3, (1024, 2049, 3): 1}


def _unit(rng, n, P):
    a = rng.standard_normal((n, P))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _case(P, K, B):
    rng = np.random.default_rng([SEEDS.get((P, K, B), 0), P, K, B])
    return _unit(rng, B, P), _unit(rng, K, P)


def _sim64(f, t):
    return f.astype(np.float64) @ t.astype(np.float64).T


def _assert_separated(sim, topk, P):
    """The host-side pre-check: every gap among the top topk + 1 similarities of every row exceeds 2 gamma_P."""
    gamma = P * eb.U32 / (1 - P * eb.U32)
    top = -np.sort(-sim, axis=1)[:, : topk + 1]
    if top.shape[1] > 1:
        gaps = -np.diff(top, axis=1)
        assert gaps.min() > 2 * gamma, f"inputs do not decide the order: min gap {gaps.min():.3e} <= 2 gamma_P {2 * gamma:.3e}"


def _want_idx(sim, topk):
    K = sim.shape[1]
    order = np.argsort(-sim, axis=1, kind="stable")[:, :topk].astype(np.int32)
    if topk > K:
        order = np.concatenate([order, np.full((sim.shape[0], topk - K), -1, np.int32)], axis=1)
    return order


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def nets():
    """One tiny-geometry handle per projection width (the tail's P is the handle's proj_dim)."""
    made = {P: gs.widened_net(P, precision="fp32", max_batch=4) for P in PS}
    yield made
    for n in made.values():
        n.close()


# ---- A. order against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", PS)
def test_order_matches_fp64_argsort(nets, P, K, B):
    f, t = _case(P, K, B)
    sim = _sim64(f, t)
    _assert_separated(sim, max(TOPKS), P)        # before the GPU is touched; covers topk = 1 and 5 as well
    fd, td = _dev(f), _dev(t)
    for topk in TOPKS:
        scores, idx, prob = nets[P].score_features(fd, td, 1.0, "MCM", topk=topk)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, topk) and tuple(prob.shape) == (B, topk)
        np.testing.assert_array_equal(idx.cpu().numpy(), _want_idx(sim, topk), err_msg=f"P={P} K={K} B={B} topk={topk}")


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("K", [17, 1025, 2049])
def test_planted_winner_at_the_ends(nets, K, where):
    P = 512
    f, t = _case(P, K, 1)
    w = 0 if where == "first" else K - 1
    t[w] = f[0]                                  # similarity 1 with the image: the winner, at an end of the bank
    sim = _sim64(f, t)
    _assert_separated(sim, 8, P)
    _, idx, _ = nets[P].score_features(_dev(f), _dev(t), 1.0, "MCM", topk=8)
    got = idx.cpu().numpy()
    assert got[0, 0] == w
    np.testing.assert_array_equal(got, _want_idx(sim, 8))


# ---- B. ties ------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_index(nets):
    P, K = 64, 40
    f, t = _case(P, K, 1)
    t[7] = f[0]
    t[29] = t[7]                                 # bitwise copies: bitwise equal similarities
    _, idx, prob = nets[P].score_features(_dev(f), _dev(t), 1.0, "MCM", topk=5)
    got = idx.cpu().numpy()[0]
    assert list(got[:2]) == [7, 29]
    pb = _bits(prob)[0]
    assert pb[0] == pb[1]
    _assert_separated(_sim64(f, np.delete(t, 29, axis=0)), 5, P)   # apart from the planted tie the order is decided
    np.testing.assert_array_equal(got, _want_idx(_sim64(f, t), 5)[0])
    t[35] = t[7]                                 # three copies, two slots: the cut keeps the two lowest rows
    _, idx, _ = nets[P].score_features(_dev(f), _dev(t), 1.0, "MCM", topk=2)
    assert list(idx.cpu().numpy()[0]) == [7, 29]


# ---- C. no candidate ----------------------------------------------------------------------------------------------------
def test_slots_without_a_candidate(nets):
    P = 64
    f, t = _case(P, 15, 3)
    sim = _sim64(f, t[:3])
    _assert_separated(sim, 5, P)
    _assert_separated(_sim64(f, t), 5, P)
    _, idx, prob = nets[P].score_features(_dev(f), _dev(t[:3]), 1.0, "MCM", topk=5)   # topk > K
    got, pr = idx.cpu().numpy(), prob.cpu().numpy()
    np.testing.assert_array_equal(got, _want_idx(sim, 5))
    assert (got[:, 3:] == -1).all() and np.isnan(pr[:, 3:]).all() and np.isfinite(pr[:, :3]).all()
    tn = t[:6].copy()
    tn[2] = np.nan                               # a bank row of NaNs is never selected
    _, idx, prob = nets[P].score_features(_dev(f), _dev(tn), 1.0, "MCM", topk=6)
    got = idx.cpu().numpy()
    keep = [0, 1, 3, 4, 5]
    want = np.asarray(keep, np.int32)[np.argsort(-_sim64(f, tn[keep]), axis=1, kind="stable")]
    np.testing.assert_array_equal(got[:, :5], want)
    assert (got[:, 5] == -1).all() and np.isnan(prob.cpu().numpy()[:, 5]).all()
    fn = f.copy()
    fn[1] = np.nan                               # an all-NaN feature row: nothing to select
    _, idx, prob = nets[P].score_features(_dev(fn), _dev(t), 1.0, "MCM", topk=5)
    got, pr = idx.cpu().numpy(), prob.cpu().numpy()
    assert (got[1] == -1).all() and np.isnan(pr[1]).all()
    np.testing.assert_array_equal(got[[0, 2]], _want_idx(_sim64(f, t), 5)[[0, 2]])


# ---- D. scores unchanged ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 0.01])
def test_scores_are_the_plain_tails_bits(nets, T):
    from mcm_amd.config import SCORE_KINDS

    P, K, B = 512, 1025, 3
    f, t = _case(P, K, B)
    fd, td = _dev(f), _dev(t)
    for name in SCORE_KINDS:
        plain = nets[P].score_features(fd, td, T, name)
        scores, idx, prob = nets[P].score_features(fd, td, T, name, topk=5)
        np.testing.assert_array_equal(_bits(scores), _bits(plain), err_msg=f"{name} T={T}")
        if name == "MCM":
            np.testing.assert_array_equal(_bits(prob[:, 0]), _bits(-scores), err_msg=f"prob[:,0] vs -score, T={T}")


# ---- E. probabilities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 0.01])
def test_probabilities_within_the_fp64_budget(nets, T):
    """prob[b,j] against the fp64 softmax at idx[b,j], under a RELATIVE budget derived like tests/error_budget.py's
    score_budget (same constants: C_ACC, C_EXP, u32 = 2^-24), not fitted to the output.

    The kernel computes p_j = (float)((double) e_j / z), e_k = expf(u_k), u_k = s_k / T - m / T in fp32, z = sum_k e_k in
    fp64.  Mathematically p_j does not depend on m, so only the ROUNDING of the m / T term enters, not m's own error.
      * exponent argument, absolute (= relative in e_k):
          du_k = C_ACC u32 (|f| . |t_k| + |f| . |t_m|) / T        the two fp32 dot products (s_k and the max s_m), scaled by 1 / T
               + u32 (|s_k / T| + 2 |m / T| + |u_k|)               the two fp32 divides and the subtract (score_budget's term)
      * expf: C_EXP u32 relative per term (the documented few-ulp bound error_budget.py uses for score.hip);
      * z is a sum of positive terms, so its relative error is at most the largest relative error of a term,
        max_k du_k + C_EXP u32 (the fp64 summation itself: K 2^-53, nothing);
      * the quotient is formed in fp64 and rounded once to fp32: 1/2 ulp32.
    Hence |p_j - ref_j| <= ref_j (du_j + max_k du_k + 2 C_EXP u32) 1.01 + 1/2 ulp32(ref_j) (1.01: second-order terms).
    The worst error / budget ratio is printed; it must be <= 1."""
    P, K, B, topk = 512, 1025, 3, 8
    f, t = _case(P, K, B)
    fd, td = _dev(f), _dev(t)
    sim = _sim64(f, t)
    sa = np.abs(f.astype(np.float64)) @ np.abs(t.astype(np.float64)).T
    m = sim.max(axis=1, keepdims=True)
    u = sim / T - m / T
    e = np.exp(u)
    p = e / e.sum(axis=1, keepdims=True)
    sa_m = np.take_along_axis(sa, sim.argmax(axis=1)[:, None], axis=1)
    du = eb.C_ACC * eb.U32 * (sa + sa_m) / T + eb.U32 * (np.abs(sim / T) + 2 * np.abs(m / T) + np.abs(u))
    dumax = du.max(axis=1, keepdims=True)
    worst = 0.0
    for name in ("MCM", "max-logit", "var"):     # max-logit: the softmax it otherwise skips; var: sim[] overwritten twice
        _, idx, prob = nets[P].score_features(fd, td, T, name, topk=topk)
        ix = idx.cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(ix, _want_idx(sim, topk))
        ref = np.take_along_axis(p, ix, axis=1)
        pre = ref * (np.take_along_axis(du, ix, axis=1) + dumax + 2 * eb.C_EXP * eb.U32) * 1.01
        bud = pre + 0.5 * eb.ulp(ref + pre, "fp32")
        ratio = float((np.abs(prob.cpu().numpy().astype(np.float64) - ref) / bud).max())
        print(f"top-k probabilities, {name}, T={T}: worst error / budget = {ratio:.4f}")
        worst = max(worst, ratio)
    assert worst <= 1.0


# ---- F. through the towers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["fp32", "fp16", "fp16-x2", "fp16-u8"])
def test_images_equal_features_through_the_same_arm(arm):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    prec = "fp32" if arm == "fp32" else "fp16"
    net = NativeCLIP(geo, synth_state_dict(geo, 0), precision=prec, max_batch=4, max_prompt_tokens=256,
                     x2_max_batch=3 if arm == "fp16-x2" else None)
    try:
        rng = np.random.default_rng(5)
        B, S = 10, geo.image_size                # more than two chunks of max_batch (and of the x2 batch), a ragged last one
        bank = _dev(_unit(rng, 33, geo.proj_dim))
        if arm == "fp16-u8":
            px = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).cuda()
        else:
            px = _dev(rng.standard_normal((B, 3, S, S)).astype(np.float32))
        if arm == "fp16-x2":
            got = net.score_images_x2(px, bank, 1.0, "MCM", topk=5)
            feats = net.get_image_features_x2(px, normalize=True)
            for a, b in zip(got, net.x2_scorer().score_images(px, bank, topk=5)):   # (the refiner's view of the same arm)
                np.testing.assert_array_equal(_bits(a), _bits(b))
        else:
            got = net.score_images(px, bank, 1.0, "MCM", topk=5)
            feats = net.get_image_features(px, normalize=True)
        want = net.score_features(feats, bank, 1.0, "MCM", topk=5)
        for g, w, what in zip(got, want, ("scores", "idx", "prob")):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{arm}: {what}")
        np.testing.assert_array_equal(_bits(got[0]), _bits(net.score_images_x2(px, bank) if arm == "fp16-x2"
                                                           else net.score_images(px, bank)))
        assert (got[1].cpu().numpy() >= 0).all()
    finally:
        net.close()


# ---- G. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_at_the_c_level(nets):
    net = nets[64]
    lib, h = net._lib, net._h
    P, K, B = 64, 17, 3
    f, t = _case(P, K, B)
    fd, td = _dev(f), _dev(t)
    sc = torch.empty(B, device="cuda")
    ix = torch.full((B, 8), -7, dtype=torch.int32, device="cuda")
    pr = torch.empty((B, 8), device="cuda")
    vp = ctypes.c_void_p

    def feat(topk, idx=ix, scores=sc, T=1.0):
        return lib.mcm_score_features_topk(h, vp(fd.data_ptr()), B, vp(td.data_ptr()), K, T, 0, topk,
                                           vp(scores.data_ptr()) if scores is not None else None,
                                           vp(idx.data_ptr()) if idx is not None else None, vp(pr.data_ptr()), None)

    for bad in (0, 9, -1):
        assert feat(bad) == MCM_EINVAL
    assert feat(5, idx=None) == MCM_EINVAL
    assert feat(5, scores=None) == MCM_EINVAL
    assert feat(5, T=0.0) == MCM_EINVAL
    S = net.geo.image_size
    px = torch.zeros((B, 3, S, S), device="cuda")

    def img(topk, x2=0, idx=ix):
        return lib.mcm_score_topk(h, vp(px.data_ptr()), 0, x2, B, vp(td.data_ptr()), K, 1.0, 0, topk, vp(sc.data_ptr()),
                                  vp(idx.data_ptr()) if idx is not None else None, vp(pr.data_ptr()), None)

    for bad in (0, 9, -1):
        assert img(bad) == MCM_EINVAL
    assert img(5, idx=None) == MCM_EINVAL
    assert img(5, x2=1) == MCM_EINVAL            # the split-activation arm on a handle that is not fp16
    torch.cuda.synchronize()
    assert (ix.cpu().numpy() == -7).all()        # no refused call wrote an index
    # ... and the handle still works
    assert img(5) == 0
    _, idx, _ = net.score_features(fd, td, 1.0, "MCM", topk=5)
    np.testing.assert_array_equal(idx.cpu().numpy(), _want_idx(_sim64(f, t), 5))
    with pytest.raises(ValueError):
        net.score_features(fd, td, 1.0, "MCM", topk=9)
    assert lib.mcm_abi_version() == 5
