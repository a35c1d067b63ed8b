"""The referee of tests/test_gpu_geometry_envelope.py is itself held to a second implementation: the C oracle
(oracle.OracleCLIP) against transformers.CLIPModel (oracle/hf_reference.HFReference, fp32, CPU) at every geometry of
tests/geometry_envelope.py, and the helper's restatement of mcm_create's rules against its own lists.

The bounds are about 3 x the largest differences measured between the two fp32 implementations at these geometries (features
3.0e-7, MCM score 3.0e-8: fp32 round-off of two independent summation orders): 1e-6 on a unit-norm feature, 1e-7 on the score."""
import dataclasses

import numpy as np
import pytest

from oracle import hf_reference
from tests import geometry_envelope as ge

FEATURE_TOL, SCORE_TOL = 1e-6, 1e-7

needs_hf = pytest.mark.skipif(hf_reference.hf_available() is not None, reason=str(hf_reference.hf_available()))


def test_every_envelope_geometry_is_accepted_and_every_refusal_is_one_step_outside():
    for name, geo in ge.ENVELOPE.items():
        assert ge.accepted(geo) is None, (name, ge.accepted(geo))
        assert geo.v_layers <= 2 and geo.t_layers <= 2 and geo.image_size <= 128
    for geo, kw in ge.REFUSED:
        assert ge.accepted(geo, **kw) is not None, geo.name
        base = next(b for n, b in sorted(ge.ENVELOPE.items(), key=lambda nb: -len(nb[0])) if geo.name.startswith(n + "-"))
        assert ge.accepted(base) is None
        changed = [f.name for f in dataclasses.fields(geo) if f.name != "name" and getattr(geo, f.name) != getattr(base, f.name)]
        assert len(changed) + len(kw) in (1, 2), (geo.name, changed)       # (a width moves with its head count)
    # the two readings of 320 are different geometries, both inside
    a, b = ge.ENVELOPE["w320-h4x80-2tok"], ge.ENVELOPE["w320-h5x64"]
    assert a.v_width == b.v_width == 320 and a.v_width // a.v_heads == 80 and b.v_width // b.v_heads == 64


def test_the_position_limit_is_the_last_length_the_causal_fp32_attention_fits():
    L = ge.MAX_POSITIONS_LIMIT
    assert ge.attn_f32_lds_bytes(L) <= ge.ATTN_F32_LDS_CAP < ge.attn_f32_lds_bytes(L + 1)


# ---- the ping-pong GEMM's stage schedule, as a model: which shapes can show a stage parity that is not carried -------------------
def _pp_tiles_per_workgroup(M, N, grid):
    """gemm_pp_kernel's deal (gemm.hip): row tiles to the 8 XCDs by blockIdx % 8, an XCD's tiles to its grid / 8 workgroups."""
    nbm, nbn, g8 = M // 256, N // 256, grid >> 3
    out = []
    for block in range(grid):
        xcd, jx = block & 7, block >> 3
        ntl_x = ((nbm - xcd + 7) >> 3) * nbn
        out.append((ntl_x - jx + g8 - 1) // g8 if jx < ntl_x else 0)
    return out


def _pp_stale_steps(ntl, nk, carried):
    """Steps of one workgroup that read an LDS stage which does not hold their K-step.  The kernel stages step s + 1 into
    stage si = sr ^ 1 while step s computes from stage sr; sr = s & 1 over the flat step count of all its tiles (carried), or
    — the mistake — restarted at 0 with every tile (sr = ktc & 1)."""
    holds = {0: 0}                       # stage -> flat step staged into it (the prologue stages step 0 into stage 0)
    stale = 0
    for s in range(ntl * nk):
        sr = (s if carried else s % nk) & 1
        holds[sr ^ 1] = s + 1
        stale += holds.get(sr) != s
    return stale


def test_pingpong_stage_parity_shows_only_with_odd_ksteps_and_several_tiles_per_workgroup():
    """What tests/test_gpu_geometry_envelope.py's ping-pong shapes are chosen by: a stage index restarted per tile reads stale
    stages exactly when nk is odd and the workgroup walks a second tile — never with nk even (every shape of the shipped
    checkpoints) and never with one tile per workgroup (the two odd-nk shapes the suite had)."""
    for ntl in (1, 2, 3, 4):
        for nk in (1, 2, 3, 4, 5, 6, 12):
            assert _pp_stale_steps(ntl, nk, carried=True) == 0
            assert (_pp_stale_steps(ntl, nk, carried=False) > 0) == (nk % 2 == 1 and ntl >= 2), (ntl, nk)
    # the harness shapes: 4096 rows on a grid of 8 are 2 tiles per workgroup at N = 256 and 4 at N = 512
    assert set(_pp_tiles_per_workgroup(4096, 256, 8)) == {2} and set(_pp_tiles_per_workgroup(4096, 512, 8)) == {4}
    # the shipped-policy shape runs the kernel on the whole part, where no workgroup has a second tile: it holds the route
    # and the odd K-step count to the budget, not the carry
    assert max(_pp_tiles_per_workgroup(12288, 768, 256)) == 1
    # ... and (2048, 256, K = 64), the suite's earlier odd-nk ping-pong shape, is one tile per workgroup as well
    assert max(_pp_tiles_per_workgroup(2048, 256, 256)) == 1


def _both(geo):
    from mcm_amd.weights import synth_state_dict
    from oracle import oracle as orc
    from oracle.hf_reference import HFReference

    sd = synth_state_dict(geo, 0)
    return orc.OracleCLIP(geo, sd), HFReference(geo, sd, device="cpu")


@needs_hf
@pytest.mark.parametrize("name", [n for n in ge.ENVELOPE if n not in ge.TEXT_ONLY])
def test_oracle_agrees_with_hf_at_the_envelope_geometry(name):
    import torch

    from mcm_amd.synth import make_pixels, make_token_ids
    from oracle import oracle as orc

    geo = ge.ENVELOPE[name]
    o, hf = _both(geo)
    ids, mask = make_token_ids(10, seed=2)
    px, _ = make_pixels(3, geo.image_size, 10, ood=False, seed=1)
    fi, ft = o.encode_image(px), o.encode_text(ids)
    hi = hf.image_features(torch.from_numpy(px)).numpy()
    ht = hf.text_features(ids, mask).numpy()
    di, dt = float(np.abs(fi - hi).max()), float(np.abs(ft - ht).max())
    hf.set_bank(ids, mask)
    ds = float(np.abs(orc.score_features(fi, ft, 1.0, 0) - hf.score_batch(torch.from_numpy(px)).numpy()).max())
    print(f"ENVELOPE-CPU {name}: max|d image feat| {di:.2e} max|d text feat| {dt:.2e} max|d score| {ds:.2e}")
    assert di < FEATURE_TOL and dt < FEATURE_TOL and ds < SCORE_TOL, (di, dt, ds)


@needs_hf
@pytest.mark.parametrize("name", ge.TEXT_ONLY)
def test_oracle_agrees_with_hf_on_the_text_tower_at_other_lengths(name):
    geo = ge.ENVELOPE[name]
    o, hf = _both(geo)
    worst = 0.0
    for S in ge.prompt_lengths(geo.max_positions):
        ids = ge.prompts(6, S, seed=S)
        d = float(np.abs(o.encode_text(ids) - hf.text_features(ids).numpy()).max())
        print(f"ENVELOPE-CPU {name} S={S}: max|d text feat| {d:.2e}")
        worst = max(worst, d)
    assert worst < FEATURE_TOL, worst


@needs_hf
def test_hf_tells_the_two_readings_of_320_apart():
    """The referee of the GPU check that 4 heads of 80 and 5 heads of 64 are different models: with the same weights the two
    head counts give different image features in HF itself."""
    import torch

    from mcm_amd.synth import make_pixels
    from mcm_amd.weights import synth_state_dict
    from oracle.hf_reference import HFReference

    g5 = ge.ENVELOPE["w320-h5x64"]
    g4 = dataclasses.replace(g5, name="w320-h4x80", v_heads=4)
    sd = synth_state_dict(g5, 0)
    px = torch.from_numpy(make_pixels(3, g5.image_size, 10, ood=False, seed=1)[0])
    f5, f4 = (HFReference(g, sd, device="cpu").image_features(px).numpy() for g in (g5, g4))
    assert np.abs(f5 - f4).max() > 1e-3
