"""tests/attention_hd_budget.py on the CPU: at hd = 64 its helpers are the existing ones; the numpy emulation of the
head_dim-80 kernels' order stays inside the budget at L = 17, 257, 577 and 1025 in every mode; and three mistakes a
head_dim-80 kernel can make fall outside it — scale 0.125 instead of 80^-0.5, the logits summed over the first 64 dims only,
and the split-image column map of a head that does not straddle applied to head 1.  The discrimination factors are printed
(run with -s)."""
import numpy as np
import pytest

from tests import attention_hd_budget as hb
from tests import error_budget as eb
from tests import online_softmax_budget as ob

MODES = ["bf16", "fp16", "fp32", "split"]


def _operands(L, hd, heads, seed, mode):
    """qkv [L, 3 heads hd] as the mode's operand values; split: the split image [L, 6 heads hd] (float16)."""
    rng = np.random.default_rng(seed)
    D = heads * hd
    qkv = rng.standard_normal((L, 3 * D)).astype(np.float32)
    qkv[:, :2 * D] *= 1.5
    if mode == "split":
        return eb.split_image(qkv)
    return eb.round_to(qkv, mode).astype(np.float32)


def _ratio(got, ref, bud):
    return float(eb.worst(got, ref, bud)[0])


def test_hd64_helpers_equal_the_existing_modules():
    L, heads, hd = 97, 3, 64
    qkv = _operands(L, hd, heads, 1, "fp16")
    for h in range(heads):
        q, k, v = hb.head_qkv(qkv, L, heads, hd, 0, h)
        D = heads * 64
        np.testing.assert_array_equal(q, qkv[:, h * 64:(h + 1) * 64])
        np.testing.assert_array_equal(k, qkv[:, D + h * 64:D + (h + 1) * 64])
        for out in ("bf16", "fp16", "fp32"):
            r0, b0 = ob.online_attention_budget(q, k, v, out)
            r1, b1 = hb.attention_budget(q, k, v, out)
            np.testing.assert_allclose(r1, r0, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(b1, b0, rtol=1e-12, atol=1e-15)
            r2, b2 = eb.attention_budget(q, k, v, False, out)
            r3, b3 = hb.attention_budget(q, k, v, out, online=False)
            np.testing.assert_allclose(r3, r2, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(b3, b2, rtol=1e-12, atol=1e-15)
    img = _operands(L, hd, heads, 2, "split")
    for h in range(heads):
        new = hb.split_head_parts(img, L, heads, hd, 0, h)
        old = eb.head_parts(img, L, heads, 0, h)
        for a, b in zip(new, old):
            np.testing.assert_array_equal(a, b)
        # at 64 no head straddles: the contiguous map is the same map
        for a, b in zip(hb.split_head_parts_contiguous(img, L, heads, hd, 0, h), old):
            np.testing.assert_array_equal(a, b)
        r0, b0 = ob.online_attention_split_budget(*old)
        r1, b1 = hb.attention_split_budget(*new)
        np.testing.assert_allclose(r1, r0, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(b1, b0, rtol=1e-12, atol=1e-15)


def test_split_col_is_the_kernels_map():
    c = np.arange(1280)
    off = hb.split_col(c)
    assert off[0] == 0 and off[63] == 63 and off[64] == 128 and off[80] == 144 and off[127] == 191 and off[128] == 256
    # an 8-column chunk never crosses a block: its 8 offsets are consecutive
    ch = off.reshape(-1, 8)
    assert (np.diff(ch, axis=1) == 1).all()
    # hi and lo offsets together tile the 2560-element row exactly once
    assert sorted(np.concatenate([off, off + 64]).tolist()) == list(range(2560))
    # heads of 80 columns: 1280 = 16 heads = 20 blocks; head 1 (columns 80 .. 159) straddles blocks 1 and 2
    assert set((np.arange(80, 160) // 64).tolist()) == {1, 2}


def _emulated(L, mode, heads, h, seed, **mistake):
    hd = 80
    x = _operands(L, hd, heads, seed, mode)
    if mode == "split":
        wrong_map = mistake.pop("contiguous_map", False)
        parts = hb.split_head_parts(x, L, heads, hd, 0, h)
        ref, bud = hb.attention_split_budget(*parts)
        use = hb.split_head_parts_contiguous(x, L, heads, hd, 0, h) if wrong_map else parts
        qh, ql, kh, kl, vh, vl = use
        got = hb.emulate(qh, kh, vh, "split", ql=ql, kl=kl, vl=vl, **mistake)
    else:
        q, k, v = hb.head_qkv(x, L, heads, hd, 0, h)
        ref, bud = hb.attention_budget(q, k, v, mode)
        got = hb.emulate(q, k, v, mode, **mistake)
    return _ratio(got, ref, bud)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [17, 257, 577, 1025])
def test_the_kernels_order_stays_inside_the_budget(L, mode):
    r = max(_emulated(L, mode, heads=4, h=h, seed=L + h) for h in (0, 1))
    print(f"BUDGET emulation-hd80 {mode} L={L}: {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [17, 257, 1025])
def test_wrong_scale_falls_outside(L, mode):
    r = _emulated(L, mode, heads=4, h=1, seed=L, scale=0.125)
    print(f"DISCRIMINATION hd80 scale-0.125 {mode} L={L}: {r:.1f} x budget")
    assert r > 1.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [17, 257, 1025])
def test_first_64_dims_only_falls_outside(L, mode):
    r = _emulated(L, mode, heads=4, h=1, seed=L, dims=64)
    print(f"DISCRIMINATION hd80 64-of-80-dims {mode} L={L}: {r:.1f} x budget")
    assert r > 1.0


@pytest.mark.parametrize("L", [17, 257, 1025])
def test_non_straddling_column_map_on_head_1_falls_outside(L):
    r = _emulated(L, "split", heads=4, h=1, seed=L, contiguous_map=True)
    print(f"DISCRIMINATION hd80 contiguous-split-map head 1 L={L}: {r:.1f} x budget")
    assert r > 1.0
    # head 0 starts a block but is 80 wide: its last 16 columns are wrong too
    assert _emulated(L, "split", heads=4, h=0, seed=L, contiguous_map=True) > 1.0
