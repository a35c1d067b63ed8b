"""tests/text_reference.py proved on the CPU: the float64 restatement of the text tower agrees with HF's model and with the
C oracle, does not move when a prompt is padded, and pools the row HF pools.  This is what lets test_gpu_text_lengths.py hold
the HIP text tower to it at every prompt length without a second opinion on the GPU machine."""
import numpy as np
import pytest

from tests import text_reference as tr

torch = pytest.importorskip("torch")

from mcm_amd.config import geometry  # noqa: E402
from mcm_amd.weights import synth_state_dict  # noqa: E402

GEOS = ["tiny", "B16-2L"]


@pytest.fixture(scope="module", params=GEOS)
def tower(request):
    geo = geometry(request.param)
    sd = synth_state_dict(geo, 0)
    return geo, sd, tr.TextTowerFp64(geo, sd)


@pytest.fixture(scope="module")
def hf_double():
    """geometry name -> HF's CLIPModel of the seeded weights, .double() (its eager attention keeps an fp32 softmax)."""
    pytest.importorskip("transformers")
    from oracle.hf_reference import HFReference, _pooled

    models = {}

    def run(geo, sd, ids):
        if geo.name not in models:
            models[geo.name] = HFReference(geo, sd, "cpu").model.double()
        m = models[geo.name]
        t = torch.as_tensor(np.asarray(ids), dtype=torch.long)
        with torch.no_grad():
            hidden = m.text_model(input_ids=t).last_hidden_state
            pooled = _pooled(m.get_text_features(input_ids=t))
        assert hidden.dtype == torch.float64 and pooled.dtype == torch.float64
        return hidden.numpy(), pooled.numpy()

    return run


@pytest.mark.parametrize("S", [12, 77])
def test_agrees_with_hf_double(tower, hf_double, S):
    """max |difference| <= 1e-6 on hidden and pooled: HF's fp32 softmax accounts for about 1e-7, so the bound leaves a decade
    and sits two decades under the fp32 arm's tolerance (2e-4)."""
    geo, sd, ref = tower
    ids, _ = tr.length_prompts(S)
    hidden, pooled = ref(ids)
    assert hidden.dtype == np.float64 and hidden.shape == (ids.shape[0], S, geo.t_width)
    assert pooled.dtype == np.float64 and pooled.shape == (ids.shape[0], geo.proj_dim)
    h_hf, p_hf = hf_double(geo, sd, ids)
    dh, dp = float(np.abs(hidden - h_hf).max()), float(np.abs(pooled - p_hf).max())
    print(f"TEXTREF vs HF.double() {geo.name} S={S}: hidden {dh:.3g} pooled {dp:.3g} (|hidden| max {np.abs(hidden).max():.3g}, "
          f"|pooled| max {np.abs(pooled).max():.3g})")
    assert dh <= 1e-6 and dp <= 1e-6, (dh, dp)


@pytest.mark.parametrize("S", [12, 77])
def test_agrees_with_the_oracle(tower, S):
    """The fp32 C oracle's unit rows within 2e-4 (the fp32 tolerance of test_towers_vs_hf_fixture)."""
    from oracle import oracle as orc

    geo, sd, ref = tower
    ids, _ = tr.length_prompts(S)
    want = tr.unit(ref(ids)[1])
    got = orc.OracleCLIP(geo, sd).encode_text(ids)
    d = float(np.abs(got - want).max())
    print(f"TEXTREF vs oracle {geo.name} S={S}: unit rows {d:.3g}")
    assert d <= 2e-4, d


def test_pad_invariance(tower):
    """Every prompt of the sweep gives the same pooled row at its own length and at every longer S, padded with EOS or followed
    by lower ids: 1e-12 in fp64 (a causal tower cannot see them; what differs is the order of BLAS sums over other shapes)."""
    geo, sd, ref = tower
    worst = 0.0
    for p in (0, 1, 6, 15, 16, 31, 38, 75, 76):
        for row in (tr.prompt(p), tr.garbage_prompt(p)):
            own = ref(row[None, :])[1][0]
            for S in sorted(s for s in {p + 1, p + 2, 16, 17, 33, 64, 77} if p + 1 <= s <= geo.max_positions):
                both = np.stack([tr.pad_to(row, S), tr.pad_to(row, S, garbage_seed=S)])
                got = ref(both)[1]
                worst = max(worst, float(np.abs(got - own).max()))
    print(f"TEXTREF pad invariance {geo.name}: {worst:.3g}")
    assert worst <= 1e-12, worst


def test_sweep_rows_are_the_prompts_they_name(tower):
    """reference_rows (each prompt once, at its own length) equals the whole padded batch at every S it is used for."""
    geo, sd, ref = tower
    cache = {}
    for S in (1, 2, 3, 16, 17, 36, 77):
        ids, keys = tr.length_prompts(S)
        assert ids.shape == (len(keys), S) and len(keys) <= 6 and (ids == tr.EOS).any(axis=1).all()
        assert [int(r.argmax()) for r in ids] == [p for _, p in keys]
        assert np.abs(ref(ids)[1] - tr.reference_rows(ref, keys, cache)).max() <= 1e-12
    assert tr.eos_positions(77) == [0, 1, 38, 75, 76] and tr.eos_positions(1) == [0] and tr.eos_positions(2) == [0, 1]
    a, b = tr.length_prompts(20)[0], tr.length_prompts(77)[0]
    assert np.array_equal(a[0], b[0, :20]) and np.array_equal(a[1], b[1, :20])     # the same prompt at every S


def test_eos_rule(tower, hf_double):
    """The pooled row is the FIRST position of the largest id: EOS at position 0, ids after the first EOS, a repeated EOS."""
    geo, sd, ref = tower
    rng = np.random.default_rng(3)
    r = rng.integers(1, tr.BOS, size=8)
    cases = [
        (np.array([tr.EOS, r[0], r[1], r[2], r[3]]), 0),                 # EOS at position 0, lower ids behind it
        (np.array([tr.BOS, r[0], tr.EOS, r[1], r[2]]), 2),               # garbage after the first EOS
        (np.array([tr.BOS, r[0], tr.EOS, r[1], tr.EOS]), 2),             # a repeated EOS: the first wins
        (np.array([tr.BOS, tr.EOS, tr.EOS, tr.EOS, tr.EOS]), 1),         # the padded form
    ]
    ids = np.stack([c[0] for c in cases]).astype(np.int64)
    hidden, pooled = ref(ids)
    proj = np.asarray(sd["text_projection.weight"], np.float64)
    for k, (_, pos) in enumerate(cases):
        rows = hidden[k] @ proj.T                                          # every position's candidate
        assert np.array_equal(pooled[k], rows[pos])
        others = [j for j in range(ids.shape[1]) if j != pos]
        assert min(np.abs(rows[j] - pooled[k]).max() for j in others) > 1e-3   # no other row would have passed for it
        alone = ref(ids[k:k + 1, :pos + 1])[1][0]                           # ... and the rest of the row does not matter
        assert np.abs(alone - pooled[k]).max() <= 1e-12
    _, p_hf = hf_double(geo, sd, ids)
    assert np.abs(pooled - p_hf).max() <= 1e-6


def test_exact_gelu_geometry_agrees_with_hf_double(hf_double):
    """The exact-GELU branch (the OpenCLIP geometries), on tiny-gelu."""
    geo = geometry("tiny-gelu")
    sd = synth_state_dict(geo, 0)
    ids, _ = tr.length_prompts(33)
    hidden, pooled = tr.text_tower_fp64(geo, sd, ids)
    h_hf, p_hf = hf_double(geo, sd, ids)
    assert np.abs(hidden - h_hf).max() <= 1e-6 and np.abs(pooled - p_hf).max() <= 1e-6
    quick = tr.text_tower_fp64(geometry("tiny"), sd, ids)[1]
    assert np.abs(quick - pooled).max() > 1e-4     # the two activations are told apart
