"""GL-MCM's local score on a real MI355X: mcm_local_score_features (glmcm.hip) against the fp64 reference and the derived
budget of tests/glmcm_budget.py — the arithmetic term plus one ulp on lattice inputs (every similarity exact in fp32), the full
budget on planted unit inputs — its determinism, NaN and refusal contract.  Budget cases print "BUDGET glmcm <worst ratio> ..."
(run with -s to collect them)."""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import glmcm_budget as gb
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gs.dev
_bits = gs.bits

WIDTHS = [64, 512, 768, 1024]
# (B, R, K).  (1,1,1): one cell; (3,16,5): three images inside one query tile; (2,196,300): images across three tile edges, K
# across the bank's 256-row tile; (5,49,257): K one row past the edge, images straddling tiles; (65,3,256): more images than a
# query tile has rows, K on the edge; (1,576,1000): nine query tiles of one image, four bank tiles.
SHAPES = [(1, 1, 1), (3, 16, 5), (2, 196, 300), (5, 49, 257), (65, 3, 256), (1, 576, 1000)]
TEMPS = [1.0, 0.01]


@pytest.fixture(scope="module")
def gl_nets():
    yield from gs.net_cache()


def _run(net, local, text, T):
    s, p = net.local_scores(local, text, T=T, return_patches=True)
    return s.cpu().numpy(), p.cpu().numpy()


@pytest.mark.parametrize("P", WIDTHS)
def test_lattice_inputs_within_the_arithmetic_term(gl_nets, P):
    net = gl_nets(P)
    worst, cases = 0.0, 0
    for B, R, K in SHAPES:
        local, text = gb.lattice_case(B, R, K, P, seed=B + R + K)
        ld, td = _dev(local), _dev(text)
        for T in TEMPS:
            patch, score = gb.reference(local, text, T)
            bp, bs = gb.budgets(local, text, T, exact=True)
            s, p = _run(net, ld, td, T)
            rp, rs = gb.ratio(p, patch, bp), gb.ratio(s, score, bs)
            worst, cases = max(worst, rp, rs), cases + 1
            assert rp <= 1.0 and rs <= 1.0, (P, B, R, K, T, rp, rs)
            assert np.array_equal(_bits(s), _bits(-p.max(axis=1))), (P, B, R, K, T)
    print(f"BUDGET glmcm {worst:.3f} lattice (arithmetic term + one ulp) P={P}: {cases} cases")


@pytest.mark.parametrize("P", WIDTHS)
def test_unit_inputs_within_budget(gl_nets, P):
    net = gl_nets(P)
    for B, R, K in SHAPES:
        local, text, _cls, _scale = gb.unit_case(B, R, K, P, seed=P + B)
        ld, td = _dev(local), _dev(text)
        for T in TEMPS:
            patch, score = gb.reference(local, text, T)
            bp, bs = gb.budgets(local, text, T)
            s, p = _run(net, ld, td, T)
            rp, rs = gb.ratio(p, patch, bp), gb.ratio(s, score, bs)
            print(f"BUDGET glmcm {max(rp, rs):.3f} (patches {rp:.3f}, scores {rs:.3f}) unit P={P} B={B} R={R} K={K} T={T}; "
                  f"S_L in [{-score.max():.3e}, {-score.min():.6f}]")
            assert rp <= 1.0 and rs <= 1.0, (P, B, R, K, T, rp, rs)
            assert np.array_equal(_bits(s), _bits(-p.max(axis=1))), (P, B, R, K, T)       # local_scores == -max(patch_dev) exactly


def test_same_bits_over_runs_image_cuts_and_image_positions(gl_nets):
    net = gl_nets(512)
    B, R, K, T = 3, 49, 257, 0.01
    local, text, _cls, _scale = gb.unit_case(B, R, K, 512, seed=5)
    ld, td = _dev(local), _dev(text)
    s1, p1 = _run(net, ld, td, T)
    for _ in range(2):                                                                   # three runs in all
        s, p = _run(net, ld, td, T)
        assert np.array_equal(_bits(s), _bits(s1)) and np.array_equal(_bits(p), _bits(p1))
    parts = [_run(net, ld[a:a + n], td, T) for a, n in ((0, 1), (1, 1), (2, 1))]
    assert np.array_equal(_bits(np.concatenate([q[0] for q in parts])), _bits(s1))
    assert np.array_equal(_bits(np.concatenate([q[1] for q in parts])), _bits(p1))
    perm = np.array([2, 0, 1])
    s, p = _run(net, _dev(local[perm]), td, T)
    assert np.array_equal(_bits(s), _bits(s1[perm])) and np.array_equal(_bits(p), _bits(p1[perm]))
    s, _ = net.local_scores(ld, td, T=T), None                                           # without patch_dev: the same scores
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(s1))


def test_a_nan_similarity_gives_a_nan_score_for_that_image_only(gl_nets):
    net = gl_nets(64)
    B, R, K, T = 5, 49, 257, 0.01
    local, text, _cls, _scale = gb.unit_case(B, R, K, 64, seed=3)
    s0, p0 = _run(net, _dev(local), _dev(text), T)
    lq = local.copy()
    lq[2, 17, 7] = np.nan                                                                # row 115 of [B R, P]: not a planted row
    s, p = _run(net, _dev(lq), _dev(text), T)
    keep = [0, 1, 3, 4]
    assert np.isnan(s[2]) and np.isnan(p[2, 17])
    others = np.ones((B, R), bool)
    others[2, 17] = False
    assert np.array_equal(_bits(p[others]), _bits(p0[others]))                           # the image's other rows included
    assert np.array_equal(_bits(s[keep]), _bits(s0[keep]))
    tn = text.copy()
    tn[256, 0] = np.nan                                                                  # one NaN prompt, in the second bank tile
    s, p = _run(net, _dev(local), _dev(tn), T)
    assert np.isnan(s).all() and np.isnan(p).all()


def test_refused_calls_launch_nothing(gl_nets):
    from mcm_amd.engine import _stream_ptr

    net, P = gl_nets(64), 64
    B, R, K = 5, 49, 257
    local, text, _cls, _scale = gb.unit_case(B, R, K, P, seed=3)
    ld, td = _dev(local), _dev(text)
    work = torch.full((B * R + 4,), 7.5, device="cuda")
    out = torch.full((B,), -2.5, device="cuda")
    pat = torch.full((B, R), -3.5, device="cuda")
    call, sp = net._lib.mcm_local_score_features, _stream_ptr

    def go(h=net._h, lp=ld.data_ptr(), B=B, R=R, tp=td.data_ptr(), K=K, T=0.01, wp=work.data_ptr(), nbytes=B * R * 4,
           op=out.data_ptr(), pp=pat.data_ptr()):
        return call(h, lp, B, R, tp, K, T, wp, nbytes, op, pp, sp())

    assert go(h=None) == -1
    assert go(lp=None) == -1 and go(tp=None) == -1 and go(wp=None) == -1 and go(op=None) == -1
    assert go(B=0) == -1 and go(B=-1) == -1 and go(R=0) == -1 and go(R=-2) == -1 and go(K=0) == -1 and go(K=-3) == -1
    assert go(B=2 ** 16, R=2 ** 15) == -1 and go(B=2 ** 30, R=2) == -1                   # B R = 2^31
    assert go(T=0.0) == -1 and go(T=-0.01) == -1 and go(T=float("inf")) == -1 and go(T=float("nan")) == -1
    assert go(nbytes=B * R * 4 - 1) == -1
    assert go(lp=ld.data_ptr() + 4) == -1 and go(tp=td.data_ptr() + 8) == -1             # rows are read 16 bytes at a time
    need = ctypes.c_int64(-1)
    wbytes = net._lib.mcm_local_workspace_bytes
    assert wbytes(None, B, R, K, ctypes.byref(need)) == -1 and wbytes(net._h, B, R, K, None) == -1
    assert wbytes(net._h, 0, R, K, ctypes.byref(need)) == -1 and wbytes(net._h, B, 0, K, ctypes.byref(need)) == -1
    assert wbytes(net._h, B, R, 0, ctypes.byref(need)) == -1 and wbytes(net._h, 2 ** 16, 2 ** 15, K, ctypes.byref(need)) == -1
    assert need.value == -1
    assert wbytes(net._h, B, R, K, ctypes.byref(need)) == 0 and need.value == B * R * 4
    torch.cuda.synchronize()
    assert (work == 7.5).all() and (out == -2.5).all() and (pat == -3.5).all()
    with pytest.raises(ValueError):
        net.local_scores(ld, td, T=0.0)
    with pytest.raises(ValueError):
        net.local_scores(ld[:, :, :60], td)
    with pytest.raises(ValueError):
        net.local_scores(ld[0], td)                                                      # [R, P]: not a batch of images
    assert go(pp=None) == 0                                                              # patch_dev is optional
    torch.cuda.synchronize()
    assert (out != -2.5).all() and (pat == -3.5).all() and (work[B * R:] == 7.5).all()
    first = out.clone()
    work.fill_(float("nan"))                                                             # the workspace needs no initialisation
    assert go() == 0                                                                     # the same buffers take a good call
    torch.cuda.synchronize()
    assert torch.equal(out, first) and (pat != -3.5).all() and torch.isnan(work[B * R:]).all()


def test_a_handle_whose_width_is_not_a_multiple_of_four_is_refused_at_create():
    """proj_dim % 4 != 0 cannot reach mcm_local_score_features: mcm_create refuses such a handle (the rule the entry states
    is the walk's; it is checked there all the same)."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = dataclasses.replace(geometry("tiny"), name="tiny-P62", proj_dim=62)
    with pytest.raises(RuntimeError):
        NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=8, max_prompt_tokens=256)
