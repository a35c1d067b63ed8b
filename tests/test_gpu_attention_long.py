"""The streaming attention kernels (attention.hip attn_long_kernel / attn_long_f32_kernel: bidirectional, L = 289 ... 1025)
against fp64 references: under the online-softmax budget of tests/online_softmax_budget.py (proved on the CPU by
tests/test_online_softmax_budget.py) over every (sequence, head) pair, with logits whose running max jumps at a chosen tile
(guide rule 26: random data never takes the rescale branch), the CLS-only last layer (qrows = 1), the split-activation form,
and the ceiling (L = 1026 is refused without a launch).

Each budget check prints "BUDGET <what> <precision> <worst max|got - ref| / budget>" (run with -s to collect them)."""

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gpu_scaffold as gs
from tests import online_softmax_budget as ob

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREC = {"bf16": 0, "fp32": 1, "fp16": 2}
DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}


def _tiny(harness):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    return NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=64, max_prompt_tokens=4096,
                      harness=harness)


@pytest.fixture(scope="module")
def tiny_net():
    """A handle of the SHIPPED library (libmcm_hip.so): its own kernel choice, no switches."""
    net = _tiny(False)
    yield net
    net.close()


@pytest.fixture(scope="module")
def harness_net():
    """A handle of libmcm_hip_harness.so (same sources, -DMCM_HARNESS): mcm_debug_op_attention's qrows."""
    net = _tiny(True)
    yield net
    net.close()


_ptr = gs.ptr


_check = gs.check_budget


def _qkv(nseq, L, heads, seed, spike=None, spread=1.5):
    """[nseq * L, 3 D] fp32 on the host.  spike = key index: in every (sequence, head) that key dominates the logits of
    (nearly) every query (the queries' dim 0 made positive, the spiked K row's dim 0 = 48), so the running max jumps at the
    tile holding it."""
    rng = np.random.default_rng(seed)
    D = heads * 64
    qkv = rng.standard_normal((nseq * L, 3 * D)).astype(np.float32)
    qkv[:, :2 * D] *= spread
    if spike is not None:
        for n in range(nseq):
            for h in range(heads):
                rows = slice(n * L, (n + 1) * L)
                qkv[rows, h * 64] = np.abs(qkv[rows, h * 64]) + 2.0
                kr = n * L + spike
                qkv[kr, D + h * 64:D + (h + 1) * 64] *= 0.1
                qkv[kr, D + h * 64] = 48.0
    return qkv


def _attention(net, prec, qkv_dev, nseq, L, heads):
    out = torch.zeros((nseq * L, heads * 64), device="cuda", dtype=DTYPE[prec])
    rc = net._lib.mcm_op_attention(net._h, PREC[prec], _ptr(qkv_dev), _ptr(out), nseq, L, heads, 0, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    return out


def _budget_check(what, prec, qkv_dev, out, nseq, L, heads, rows=None):
    """Every (sequence, head) pair against the fp64 reference under the online-softmax budget (query rows `rows` of each
    sequence: all by default)."""
    qkv_h = qkv_dev.float().cpu().numpy()
    out_h = out.float().cpu().numpy()
    D = heads * 64
    got_all, ref_all, bud_all = [], [], []
    for n in range(nseq):
        seq = qkv_h[n * L:(n + 1) * L]
        sel = slice(None) if rows is None else rows
        for h in range(heads):
            ref, bud = ob.online_attention_budget(seq[sel, h * 64:(h + 1) * 64], seq[:, D + h * 64:D + (h + 1) * 64],
                                                  seq[:, 2 * D + h * 64:2 * D + (h + 1) * 64], prec)
            got_all.append(out_h[n * L:(n + 1) * L][sel, h * 64:(h + 1) * 64])
            ref_all.append(ref)
            bud_all.append(bud)
    return _check(what, prec, np.stack(got_all), np.stack(ref_all), np.stack(bud_all),
                  f"nseq={nseq} L={L} heads={heads}")


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("L,nseq", [(289, 3), (401, 3), (577, 2), (1025, 2)])
def test_long_attention_within_budget(tiny_net, L, nseq, prec):
    heads = 2
    qkv = torch.from_numpy(_qkv(nseq, L, heads, seed=L * 7 + nseq)).cuda().to(DTYPE[prec])
    out = _attention(tiny_net, prec, qkv, nseq, L, heads)
    _budget_check("attention-long", prec, qkv, out, nseq, L, heads)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("spike", [576, 0, 300], ids=["last-tile", "first-tile", "mid-tile"])
def test_long_attention_spiked_max_within_budget(tiny_net, spike, prec):
    """A dominant key at index 576 (the last 64-key tile of 577 keys, one valid key in it), at 0 (the first tile: no later
    rescale) and at 300: the running max of nearly every query jumps there."""
    nseq, L, heads = 2, 577, 2
    qkv = torch.from_numpy(_qkv(nseq, L, heads, seed=spike + 1, spike=spike)).cuda().to(DTYPE[prec])
    out = _attention(tiny_net, prec, qkv, nseq, L, heads)
    assert torch.isfinite(out.float()).all()
    _budget_check("attention-long-spiked", prec, qkv, out, nseq, L, heads)
    # the spike does decide the output: the dominant key's V row carries most of the weight
    got = out[0:L, 0:64].float().cpu().numpy()
    vrow = qkv[spike, 2 * heads * 64:2 * heads * 64 + 64].float().cpu().numpy()
    assert np.median(np.abs(got - vrow).max(axis=1)) < 0.5


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_long_attention_cls_only_rows(harness_net, prec):
    """qrows = 1 (the CLS-only last vision layer): one query chunk per (sequence, head); row 0 equals the full launch's row 0
    bit for bit, in both walk directions."""
    lib = harness_net._lib
    nseq, L, heads = 3, 577, 2
    qkv = torch.from_numpy(_qkv(nseq, L, heads, seed=9)).cuda().to(DTYPE[prec])
    full = _attention(harness_net, prec, qkv, nseq, L, heads)
    for rev in (0, 1):
        out = torch.zeros((nseq * L, heads * 64), device="cuda", dtype=DTYPE[prec])
        rc = lib.mcm_debug_op_attention(harness_net._h, PREC[prec], _ptr(qkv), _ptr(out), nseq, L, heads, 0, 1, rev, None)
        assert rc == 0, lib.mcm_last_error(harness_net._h)
        torch.cuda.synchronize()
        cls = torch.arange(nseq, device="cuda") * L
        assert torch.equal(out[cls], full[cls])
    _budget_check("attention-long-cls", prec, qkv, full, nseq, L, heads, rows=slice(0, 1))


_split_image = eb.split_image
_merge_image = eb.merge_image


def _attention_f64(qkv, nseq, L, heads):
    D = heads * 64
    out = np.empty((nseq * L, D))
    for n in range(nseq):
        seq = qkv[n * L:(n + 1) * L]
        for h in range(heads):
            s = 0.125 * (seq[:, h * 64:(h + 1) * 64] @ seq[:, D + h * 64:D + (h + 1) * 64].T)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            out[n * L:(n + 1) * L, h * 64:(h + 1) * 64] = p @ seq[:, 2 * D + h * 64:2 * D + (h + 1) * 64]
    return out


@pytest.mark.parametrize("L,spike", [(577, None), (577, 576), (1025, None)])
def test_long_attention_split(tiny_net, L, spike):
    """mcm_op_attention_split (three fp16 MFMAs per product on hi / lo pairs) against fp64, to the tolerance of the
    whole-K/V kernel at 197 tokens (tests/test_gpu_x2.py)."""
    nseq, heads = 2, 2
    qs = _split_image(_qkv(nseq, L, heads, seed=L + 3, spike=spike))
    want = _attention_f64(_merge_image(qs), nseq, L, heads)
    out = torch.zeros((nseq * L, 2 * heads * 64), device="cuda", dtype=torch.float16)
    qd = torch.from_numpy(qs).cuda()
    rc = tiny_net._lib.mcm_op_attention_split(tiny_net._h, _ptr(qd), _ptr(out), nseq, L, heads, None)
    assert rc == 0, tiny_net._lib.mcm_last_error(tiny_net._h)
    torch.cuda.synchronize()
    got = _merge_image(out.cpu().numpy())
    err = float(np.abs(got - want).max())
    print(f"attention-long-split L={L} spike={spike}: max|d| {err:.2e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=8e-6)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32", "split"])
def test_past_the_ceiling_is_refused_without_a_launch(tiny_net, prec):
    """L = 1026 (one past 32^2 + 1): a non-zero return and an untouched output."""
    nseq, L, heads = 1, 1026, 2
    D = heads * 64
    lib = tiny_net._lib
    if prec == "split":
        qkv = torch.zeros((nseq * L, 6 * D), device="cuda", dtype=torch.float16)
        out = torch.full((nseq * L, 2 * D), 7.0, device="cuda", dtype=torch.float16)
        rc = lib.mcm_op_attention_split(tiny_net._h, _ptr(qkv), _ptr(out), nseq, L, heads, None)
    else:
        qkv = torch.zeros((nseq * L, 3 * D), device="cuda", dtype=DTYPE[prec])
        out = torch.full((nseq * L, D), 7.0, device="cuda", dtype=DTYPE[prec])
        rc = lib.mcm_op_attention(tiny_net._h, PREC[prec], _ptr(qkv), _ptr(out), nseq, L, heads, 0, None)
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((out.float() == 7.0).all())
    # the handle stays usable
    q2 = torch.zeros((289, 3 * D), device="cuda", dtype=torch.float16)
    assert lib.mcm_op_attention(tiny_net._h, PREC["fp16"], _ptr(q2), _ptr(torch.empty((289, D), device="cuda",
                                                                                        dtype=torch.float16)),
                                1, 289, heads, 0, None) == 0
