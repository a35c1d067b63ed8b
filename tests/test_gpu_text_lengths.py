"""Causal attention and the whole text tower at EVERY prompt length 1 ... 77, against float64.

The text tower runs at whatever length the tokenizer pads to, so every key-tile count 1 ... 5 of attn_tr_kernel<..., CAUSAL>
and every residue of L mod 16 is a length a real prompt bank can hit.  Three layers of checks:

  a. mcm_op_attention, causal, at every L = 1 ... 77 (and one full and one ragged length of each larger instantiation the C
     ABI reaches) under the derived fp64 budget of tests/error_budget.py, which test_error_budget.py proves to be broken
     by each of three wrong masks at every length 2 ... 77;
  b. rows past a cut replaced by +-1e4 in q, k and v: the output rows up to the cut keep their bits;
  c. get_text_features against tests/text_reference.py (float64 throughout, proved on the CPU by test_text_reference.py),
     at every padded length, in several passes per call, at the tower tolerances of test_towers_vs_hf_fixture.

Prints "BUDGET text-attn ..." and "BUDGET text-length ..." lines (run with -s to collect them)."""
import numpy as np
import pytest

from tests import text_reference as tr
from tests.test_gpu_error_budget import DTYPE, _attention, _attn_check, _attn_qkv, _tiny

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PRECS = ["bf16", "fp16", "fp32"]
NSEQ, HEADS = 3, 2


@pytest.fixture(scope="module")
def op_net():
    """A handle of the shipped library for the op-level calls (the precision of an op call is its own argument)."""
    net = _tiny(False)
    yield net
    net.close()


# ---- a. every length under the derived budget --------------------------------------------------------------------------
def _sweep(net, prec, lengths, what):
    """Causal attention at every L of lengths under the fp64 budget; every failing L is collected before the assert."""
    failed, worst = [], (-1.0, 0)
    for L in lengths:
        qkv = _attn_qkv(NSEQ, L, HEADS, prec, seed=L * 7 + 1)
        out = _attention(net, prec, qkv, NSEQ, L, HEADS, True)
        try:
            r = _attn_check(what, prec, qkv, out, NSEQ, L, HEADS, True)
            worst = max(worst, (r, L))
        except pytest.fail.Exception as e:
            failed.append(f"L={L}: {e.msg}")
    print(f"BUDGET {what} {prec} worst {worst[0]:.3f} at L={worst[1]}" + (f" ({len(failed)} lengths over budget)" if failed else ""))
    assert net.kernel_faults == 0
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("prec", PRECS)
def test_causal_attention_every_text_length_within_budget(op_net, prec):
    """L = 1 ... 77: key-tile counts 1 ... 5, the diagonal tile full, ragged and the ragged LAST tile, every L mod 16."""
    _sweep(op_net, prec, range(1, 78), "text-attn")


# key-tile counts 6, 8, 10, 13, 17, 18 of launch_tr_by_tiles: a full and a ragged length each (the fp32 VALU kernel's LDS,
# (129 L + 256 + 4 L) * 4 bytes, is 154 240 bytes at L = 288, under its 160 KiB limit)
LONG_CAUSAL = [96, 81, 128, 97, 160, 129, 208, 161, 272, 209, 288, 273]


@pytest.mark.parametrize("prec", PRECS)
def test_causal_attention_larger_instantiations_within_budget(op_net, prec):
    assert (129 * max(LONG_CAUSAL) + 256 + 4 * max(LONG_CAUSAL)) * 4 <= 160 * 1024
    _sweep(op_net, prec, LONG_CAUSAL, "text-attn-long")


# ---- b. future rows cannot reach past rows -----------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("prec", PRECS)
def test_future_rows_do_not_reach_past_rows_bit_for_bit(op_net, prec):
    """Rows p + 1 ... of q, k and v replaced by +-1e4 (finite in all three formats; |q.k| <= 64 * 1e4 * |q| and 64 * 1e8 stay
    finite in fp32, so a masked score is replaced, never NaN, and 0 * v is an exact zero): output rows 0 ... p keep their bits.
    Holds by construction: a masked key gets exp2(-inf) = 0, and the fp32 kernel never reads it."""
    D = HEADS * 64
    differ = []
    for L in (17, 32, 33, 49, 64, 77):
        qkv = _attn_qkv(NSEQ, L, HEADS, prec, seed=L + 100)
        out = _attention(op_net, prec, qkv, NSEQ, L, HEADS, True).view(NSEQ, L, D)
        assert torch.isfinite(out.float()).all()
        g = torch.Generator(device="cuda").manual_seed(L)
        sign = torch.randint(0, 2, (NSEQ, L, 3 * D), device="cuda", generator=g).to(torch.float32) * 2 - 1
        for p in sorted({c for c in (0, 14, 15, 16, 17, L - 2) if 0 <= c <= L - 2}):
            bad = qkv.clone().view(NSEQ, L, 3 * D)
            bad[:, p + 1:] = (sign[:, p + 1:] * 1.0e4).to(DTYPE[prec])
            got = _attention(op_net, prec, bad.view(NSEQ * L, 3 * D), NSEQ, L, HEADS, True).view(NSEQ, L, D)
            same = _bits(got[:, :p + 1]) == _bits(out[:, :p + 1])
            if not bool(same.all()):
                rows = sorted({int(r) for r in (~same).nonzero()[:, 1].unique().cpu()})
                differ.append(f"L={L} cut={p}: rows {rows} changed")
            assert not bool(_bits(got[:, p + 1:]).eq(_bits(out[:, p + 1:])).all())   # the poison did reach the rows it may reach
    assert op_net.kernel_faults == 0
    assert not differ, "\n".join(differ)


# ---- c. the whole text tower, by length --------------------------------------------------------------------------------
TILE_CLASSES = [(1, 16), (17, 32), (33, 48), (49, 64), (65, 77)]
FP32_ATOL, COS_FLOOR = 2e-4, {"fp16": 0.99998, "bf16": 0.999}   # test_towers_vs_hf_fixture's tower tolerances
_REF = {}     # geometry name -> (state dict, TextTowerFp64, {prompt key: fp64 pooled row})


def _reference(name):
    from mcm_amd.config import geometry
    from mcm_amd.weights import synth_state_dict

    if name not in _REF:
        geo = geometry(name)
        sd = synth_state_dict(geo, 0)
        _REF[name] = (geo, sd, tr.TextTowerFp64(geo, sd), {})
    return _REF[name]


def _net(name, arm, max_prompt_tokens):
    from mcm_amd.engine import NativeCLIP

    geo, sd, _, _ = _reference(name)
    return NativeCLIP(geo, sd, precision=arm, max_batch=4, max_prompt_tokens=max_prompt_tokens)


def _cos(a, b):
    return np.sum(tr.unit(a) * tr.unit(b), axis=-1)


def _length_sweep(name, arm, lengths, max_prompt_tokens):
    """get_text_features (normalised and raw) of tr.length_prompts(S) at every S of lengths against the fp64 rows.  Returns
    nothing; fails with every (S, row) that misses the arm's tolerance: 2e-4 max abs (every arm, see below), and the cosine floor
    of a 16-bit arm."""
    _, _, tower, cache = _reference(name)
    net = _net(name, arm, max_prompt_tokens)
    missed = []
    worst = {c: np.zeros(2) for c in TILE_CLASSES}
    try:
        for S in lengths:
            ids, keys = tr.length_prompts(S)
            want = tr.reference_rows(tower, keys, cache)
            idt = torch.from_numpy(ids)
            txt = net.get_text_features(input_ids=idt, normalize=True).cpu().numpy().astype(np.float64)
            raw = net.get_text_features(input_ids=idt).cpu().numpy().astype(np.float64)
            assert np.isfinite(txt).all() and np.isfinite(raw).all(), (name, arm, S)
            cls = next(c for c in TILE_CLASSES if c[0] <= S <= c[1])
            # max |difference| on unit rows (both forms) and on the raw rows relative to max(1, max |raw|): the fp32 tolerance.
            # It is asked of EVERY arm: the text tower runs the exact-fp32 kernels whatever the handle's precision
            # (mcm_api.hip: h->txt is MCM_PREC_F32), so the 16-bit arms owe the same rows; their cosine floors hold a fortiori.
            err = np.maximum(np.abs(txt - tr.unit(want)).max(axis=1), np.abs(tr.unit(raw) - tr.unit(want)).max(axis=1))
            err = np.maximum(err, np.abs(raw - want).max(axis=1) / max(1.0, float(np.abs(want).max())))
            one_minus_cos = 1.0 - np.minimum(_cos(txt, want), _cos(raw, want))
            bad = err > FP32_ATOL
            if arm != "fp32":
                bad |= ~(1.0 - one_minus_cos > COS_FLOOR[arm])
            if np.abs(txt - tr.unit(raw)).max() > 1e-6:    # the fused normalise is the raw form's rows over their norms
                missed.append(f"S={S}: normalised and raw forms differ by {np.abs(txt - tr.unit(raw)).max():.3g}")
            worst[cls] = np.maximum(worst[cls], [err.max(), one_minus_cos.max()])
            for i in np.nonzero(bad)[0]:
                missed.append(f"S={S} row {keys[i]}: max abs {err[i]:.3g}, 1 - cos {one_minus_cos[i]:.3g}")
        sat, faults = net.saturation_count(), net.kernel_faults
    finally:
        net.close()
    for (lo, hi), w in worst.items():
        if any(lo <= S <= hi for S in lengths):
            print(f"BUDGET text-length {name} {arm} S={lo}..{hi} mpt={max_prompt_tokens} worst max-abs {w[0]:.3g} 1-cos {w[1]:.3g}")
    assert sat == 0 and faults == 0, (sat, faults)
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("arm", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "B16-2L"])
def test_text_tower_every_length_against_fp64(name, arm):
    """Every S = 1 ... 77 on a handle of max_prompt_tokens = 154: one pass up to S = 25, a ragged last pass at S = 31 ... 38,
    two prompts per pass from S = 52 on."""
    _length_sweep(name, arm, range(1, 78), 154)


def test_text_tower_h14_lengths_against_fp64():
    """The 16-head, 1024-wide, exact-GELU text tower of H/14 (fp16), at a length of each key-tile class."""
    _length_sweep("H14-2L", "fp16", [16, 17, 32, 49, 77], 154)


@pytest.mark.parametrize("arm", ["fp32", "fp16", "bf16"])
def test_text_tower_one_prompt_per_pass_at_77(arm):
    """max_prompt_tokens = 77 at S = 77: every prompt a pass of its own."""
    _length_sweep("tiny", arm, [77], 77)
