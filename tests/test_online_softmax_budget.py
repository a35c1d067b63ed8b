"""The online-softmax attention budget (tests/online_softmax_budget.py) proved on the CPU, the way tests/test_error_budget.py
proves the others: a numpy emulation of the streaming kernels' tile order (attention.hip attn_long_kernel and
attn_long_f32_kernel) stays inside it in every mode at L = 289, 577 and 1025, on random logits and on logits whose max jumps
at a chosen tile; and the two classic rescale mistakes (guide rule T13) break it: O not rescaled when the max grows, and the
row sum scaled by a stale factor."""
import numpy as np
import pytest

from tests import error_budget as eb
from tests import online_softmax_budget as ob

torch = pytest.importorskip("torch")

F32 = np.float32
SC16 = F32(0.125 * 1.4426950408889634)


def _f32(a):
    return np.asarray(a, dtype=F32)


def _mm(a, b):
    return (torch.from_numpy(_f32(a)) @ torch.from_numpy(_f32(b))).numpy()


def _online_emulate(q, k, v, out, mutation=None, kt=ob.KT):
    """One (sequence, head) as the streaming kernels compute it: per tile of kt keys S = Q K^T (fp32), the tile max, m' =
    max(m, tile max), a = exp2((m - m') SC) (16-bit modes; exact: exp(m - m') on the 0.125-scaled logits), O *= a, l *= a,
    P = exp2(S SC - m' SC) rounded to the operand format (exact: exp(s - m') in fp32), l += rowsum(P) in fp32, O += P V
    (fp32 accumulation); at the end O / l rounded to the output format.
    mutation "no_rescale_o": O is not multiplied by a; "stale_l": l is multiplied by the previous tile's factor."""
    L = q.shape[0]
    o = np.zeros((L, 64), F32)
    lsum = np.zeros((L, 1), F32)
    m = np.full((L, 1), -np.inf, F32)
    a_prev = np.ones((L, 1), F32)
    for k0 in range(0, L, kt):
        s = _mm(q, k[k0:k0 + kt].T)                     # [q, keys of the tile], fp32
        if out == "fp32":
            s = _f32(s * F32(0.125))
        mt = s.max(axis=1, keepdims=True)
        mn = np.maximum(m, mt)
        with np.errstate(invalid="ignore"):
            if out == "fp32":
                a = _f32(np.exp((m - mn).astype(np.float64)))
                e = _f32(np.exp(_f32(s - mn).astype(np.float64)))
                p = e
            else:
                a = _f32(np.exp2(_f32(_f32(m - mn) * SC16).astype(np.float64)))
                arg = _f32(s.astype(np.float64) * SC16 - _f32(mn * SC16))
                e = _f32(np.exp2(arg.astype(np.float64)))
                p = eb.round_to(e, out)
        a = np.where(np.isfinite(m), a, F32(0)).astype(F32)
        m = mn
        if mutation != "no_rescale_o":
            o = _f32(o * a)
        lsum = _f32(lsum * (a_prev if mutation == "stale_l" else a))
        a_prev = a
        lsum = _f32(lsum + p.sum(axis=1, keepdims=True, dtype=F32))
        o = _f32(o + _mm(p, v[k0:k0 + kt]))
    res = _f32(o * _f32(F32(1) / lsum))
    return res if out == "fp32" else eb.round_to(res, out)


def _case(L, out, seed, spike=None):
    """q, k, v [L, 64] in the operand format.  spike = key index: that key dominates the logits of (nearly) every query
    (every query gets a positive dim 0, the spiked K row a large one), so the running max jumps at the tile holding it."""
    rng = np.random.default_rng(seed)
    qkv = rng.standard_normal((L, 192)).astype(F32)
    qkv[:, :128] *= 1.5
    if spike is not None:
        qkv[:, 0] = np.abs(qkv[:, 0]) + 2.0
        qkv[spike, 64:128] *= 0.1
        qkv[spike, 64] = 48.0
    if out != "fp32":
        qkv = eb.round_to(qkv, out)
    return qkv[:, :64], qkv[:, 64:128], qkv[:, 128:]


LS = [289, 577, 1025]


def test_block_terms_equal_the_whole_row_budget():
    """online=False reproduces error_budget.attention_budget (row blocks, no [L, L, 64] temporary)."""
    for out in ("bf16", "fp16", "fp32"):
        q, k, v = _case(289, out, 3)
        ref0, bud0 = eb.attention_budget(q, k, v, False, out)
        ref1, bud1 = ob.online_attention_budget(q, k, v, out, online=False)
        np.testing.assert_allclose(ref1, ref0, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bud1, bud0, rtol=1e-9, atol=0)


@pytest.mark.parametrize("out", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("L", LS)
def test_online_emulation_within_budget(L, out):
    worst = 0.0
    for spike in (None, 0, L - 1, L // 2):
        q, k, v = _case(L, out, L + (spike or 0), spike)
        ref, bud = ob.online_attention_budget(q, k, v, out)
        r, _ = eb.worst(_online_emulate(q, k, v, out), ref, bud)
        worst = max(worst, r)
        assert r <= 1.0, (L, out, spike, r)
    print(f"online attention {out} L={L}: worst budget ratio {worst:.3g}")


@pytest.mark.parametrize("mutation", ["no_rescale_o", "stale_l"])
@pytest.mark.parametrize("out", ["bf16", "fp16", "fp32"])
def test_rescale_mistakes_break_the_budget(mutation, out):
    for L in LS:
        q, k, v = _case(L, out, L + 1, spike=L - 1)   # the max jumps at the last tile
        ref, bud = ob.online_attention_budget(q, k, v, out)
        r, _ = eb.worst(_online_emulate(q, k, v, out, mutation=mutation), ref, bud)
        print(f"online attention {mutation} {out} L={L}: worst budget ratio {r:.3g}")
        assert r > 1.0, (mutation, out, L, r)


def test_spike_moves_the_running_max_at_its_tile():
    """The spiked cases do exercise the rescale: for nearly every query the max of the spiked key's tile is far above every
    earlier tile's max."""
    for L in LS:
        q, k, v = _case(L, "fp32", L + 1, spike=L - 1)
        s = q.astype(np.float64) @ k.astype(np.float64).T
        last = (L - 1) // ob.KT * ob.KT
        assert (s[:, last:].max(axis=1) > s[:, :last].max(axis=1) + 16.0).mean() > 0.9
