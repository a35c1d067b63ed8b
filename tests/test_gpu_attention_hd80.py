"""The head_dim-80 attention family (attention.hip attn_hd80_kernel / attn_hd80_f32_kernel; ViT-H/14's vision tower) through
the harness library's mcm_debug_op_attention_hd / mcm_debug_op_attention_split_hd, against the fp64 reference under the budget
of tests/attention_hd_budget.py (proved on the CPU by tests/test_attention_hd_budget.py): bf16 / fp16 / fp32 / split, every
length class of the streaming loop (L = 1, 16, 17, 64, 65, 257, 289, 577, 1025), 1, 3 and 16 heads, the CLS-only last layer
(qrows = 1) and both walk directions, logits whose running max jumps at the first, a middle and the last tile, and the
coherent-small-P input of the split form.  Every (sequence, head) pair is checked.

A split row is whole 64-column blocks, so the split form exists for heads x 80 a multiple of 64 only: it runs 4 and 16 heads
here, and 1 and 3 heads are refused without a launch (as are head_dim 96, L = 1026 and causal attention at 80).

Each budget check prints "BUDGET attn-hd80-<mode> <worst max|got - ref| / budget>" (run with -s to collect them)."""

import numpy as np
import pytest

from tests import attention_hd_budget as hb
from tests import error_budget as eb
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HD = 80
PREC = {"bf16": 0, "fp32": 1, "fp16": 2}
DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
LENGTHS = [1, 16, 17, 64, 65, 257, 289, 577, 1025]
WORST = {}


@pytest.fixture(scope="module")
def harness_net():
    """A handle of libmcm_hip_harness.so: the operator-level entry points with a head_dim argument live there."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    net = NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=64, max_prompt_tokens=4096, harness=True)
    yield net
    assert net.kernel_faults == 0
    assert net.saturation_count() == 0
    net.close()
    for mode in sorted(WORST):
        print(f"BUDGET attn-hd80-{mode} worst {WORST[mode]:.3f}")


_ptr = gs.ptr


def _qkv(nseq, L, heads, seed, spike=None, spread=1.5):
    """tests/test_gpu_attention_long.py's input at 80-wide heads: [nseq L, 3 D] fp32; spike = key index whose K row
    dominates the logits of (nearly) every query of every (sequence, head), so the running max jumps at its tile."""
    rng = np.random.default_rng(seed)
    D = heads * HD
    qkv = rng.standard_normal((nseq * L, 3 * D)).astype(np.float32)
    qkv[:, :2 * D] *= spread
    if spike is not None:
        for n in range(nseq):
            for h in range(heads):
                rows = slice(n * L, (n + 1) * L)
                qkv[rows, h * HD] = np.abs(qkv[rows, h * HD]) + 2.0
                kr = n * L + spike
                qkv[kr, D + h * HD:D + (h + 1) * HD] *= 0.1
                qkv[kr, D + h * HD] = 48.0
    return qkv


def _run(net, mode, qkv_dev, nseq, L, heads, qrows=0, rev=0, head_dim=HD, causal=0, fill=0.0):
    lib = net._lib
    D = heads * head_dim
    if mode == "split":
        out = torch.full((nseq * L, 2 * D), fill, device="cuda", dtype=torch.float16)
        rc = lib.mcm_debug_op_attention_split_hd(net._h, _ptr(qkv_dev), _ptr(out), nseq, L, heads, head_dim, qrows, rev, None)
    else:
        out = torch.full((nseq * L, D), fill, device="cuda", dtype=DTYPE[mode])
        rc = lib.mcm_debug_op_attention_hd(net._h, PREC[mode], _ptr(qkv_dev), _ptr(out), nseq, L, heads, head_dim, causal, qrows,
                                           rev, None)
    torch.cuda.synchronize()
    return rc, out


def _device_operands(mode, qkv32):
    if mode == "split":
        return torch.from_numpy(eb.split_image(qkv32)).cuda()
    return torch.from_numpy(qkv32).cuda().to(DTYPE[mode])


def _budget_check(what, mode, qkv_dev, out, nseq, L, heads, rows=None):
    """Every (sequence, head) pair, query rows `rows` of each sequence (all by default)."""
    sel = slice(None) if rows is None else rows
    out_h = out.float().cpu().numpy()
    x = qkv_dev.cpu().numpy() if mode == "split" else qkv_dev.float().cpu().numpy()
    got_all, ref_all, bud_all = [], [], []
    for n in range(nseq):
        for h in range(heads):
            if mode == "split":
                qh, ql, kh, kl, vh, vl = hb.split_head_parts(x, L, heads, HD, n, h)
                ref, bud = hb.attention_split_budget(qh[sel], ql[sel], kh, kl, vh, vl)
                got = hb.split_head_out(out_h, L, heads, HD, n, h)[sel]
            else:
                q, k, v = hb.head_qkv(x, L, heads, HD, n, h)
                ref, bud = hb.attention_budget(q[sel], k, v, mode)
                got = hb.head_out(out_h, L, heads, HD, n, h)[sel]
            got_all.append(got)
            ref_all.append(ref)
            bud_all.append(bud)
    got, ref, bud = np.stack(got_all), np.stack(ref_all), np.stack(bud_all)
    r, i = eb.worst(got, ref, bud)
    print(f"BUDGET attn-hd80-{mode} {what} nseq={nseq} L={L} heads={heads}: {r:.3f}")
    WORST[mode] = max(WORST.get(mode, 0.0), float(r))
    if not r <= 1.0:
        idx = np.unravel_index(i, ref.shape)
        pytest.fail(f"attn-hd80-{mode} {what} L={L} heads={heads}: max|got - ref| / budget = {r:.3g} at (pair, row, dim) {idx}: "
                    f"got {got.flat[i]!r} ref {ref.flat[i]!r} budget {bud.flat[i]:.3g}")
    return r


def _heads_for(mode, heads):
    return {1: 4, 3: 4}.get(heads, heads) if mode == "split" else heads


def _full_and_variants(net, what, mode, qkv32, nseq, L, heads):
    """The full launch under the budget; the reverse walk bit-identical to it; qrows = 1 bit-identical in row 0, in both
    directions, and row 0 under the budget on its own."""
    qd = _device_operands(mode, qkv32)
    rc, full = _run(net, mode, qd, nseq, L, heads)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    assert torch.isfinite(full.float()).all()
    _budget_check(what, mode, qd, full, nseq, L, heads)
    rc, rev = _run(net, mode, qd, nseq, L, heads, rev=1)
    assert rc == 0 and torch.equal(rev, full)
    cls = torch.arange(nseq, device="cuda") * L
    for r in (0, 1):
        rc, one = _run(net, mode, qd, nseq, L, heads, qrows=1, rev=r)
        assert rc == 0 and torch.equal(one[cls], full[cls])
        if L > 16:   # rows past the first 16-query block are not computed
            rest = torch.ones(nseq * L, dtype=torch.bool, device="cuda")
            for n in range(nseq):
                rest[n * L:n * L + 16] = False
            assert bool((one[rest].float() == 0).all())
    _budget_check(what + "-cls", mode, qd, full, nseq, L, heads, rows=slice(0, 1))


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "split"])
@pytest.mark.parametrize("L", LENGTHS)
def test_every_length_three_heads(harness_net, L, mode):
    """3 heads (split: 4 — see the module docstring), 2 sequences: head 1 starts inside a 64-column block, head 2 crosses one."""
    heads = _heads_for(mode, 3)
    _full_and_variants(harness_net, "lengths", mode, _qkv(2, L, heads, seed=L * 7 + 2), 2, L, heads)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "split"])
@pytest.mark.parametrize("heads", [1, 16])
@pytest.mark.parametrize("L", [17, 257, 1025])
def test_one_and_sixteen_heads(harness_net, L, heads, mode):
    heads = _heads_for(mode, heads)
    nseq = 2 if L < 1025 or heads < 16 else 1
    _full_and_variants(harness_net, "heads", mode, _qkv(nseq, L, heads, seed=L + heads), nseq, L, heads)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "split"])
@pytest.mark.parametrize("spike", [576, 0, 300], ids=["last-tile", "first-tile", "mid-tile"])
def test_spiked_running_max(harness_net, spike, mode):
    """A dominant key at index 576 (the last 64-key tile of 577 keys: one valid key in it), at 0 and at 300: the running
    max of nearly every query jumps there."""
    nseq, L, heads = 2, 577, 4
    qkv32 = _qkv(nseq, L, heads, seed=spike + 1, spike=spike)
    qd = _device_operands(mode, qkv32)
    rc, out = _run(harness_net, mode, qd, nseq, L, heads)
    assert rc == 0, harness_net._lib.mcm_last_error(harness_net._h)
    assert torch.isfinite(out.float()).all()
    _budget_check("spiked", mode, qd, out, nseq, L, heads)
    # the spike does decide the output: the dominant key's V row carries most of the weight
    out_h = out.float().cpu().numpy()
    got = hb.split_head_out(out_h, L, heads, HD, 0, 1) if mode == "split" else hb.head_out(out_h, L, heads, HD, 0, 1)
    vrow = qkv32[spike, 2 * heads * HD + HD:2 * heads * HD + 2 * HD]
    assert np.median(np.abs(got - vrow).max(axis=1)) < 0.5


@pytest.mark.parametrize("L", [65, 257, 577])
def test_split_coherent_small_p(harness_net, L):
    """Every P but one equal and tiny: without the 2^12 scale before P is split their lo halves all miss by nearly 2^-25 in
    the same direction (tests/attention_hd_budget.py coherent_small_p_qkv)."""
    nseq, heads = 2, 4
    qd = _device_operands("split", hb.coherent_small_p_qkv(L, heads, HD, nseq))
    rc, out = _run(harness_net, "split", qd, nseq, L, heads)
    assert rc == 0, harness_net._lib.mcm_last_error(harness_net._h)
    _budget_check("coherent-small-p", "split", qd, out, nseq, L, heads)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "split"])
def test_wrong_arguments_are_refused_without_a_launch(harness_net, mode):
    """head_dim 96, L = 1026, causal attention at 80 (and, split, heads x 80 that is not whole blocks): a non-zero return
    and an untouched output; head_dim 64 through the same entry point still runs; the handle stays usable."""
    heads = 4
    cases = [dict(L=257, head_dim=96), dict(L=1026, head_dim=HD)]
    if mode != "split":
        cases.append(dict(L=257, head_dim=HD, causal=1))
    for c in cases:
        L, hd = c["L"], c["head_dim"]
        qkv = torch.zeros((L, (6 if mode == "split" else 3) * heads * hd), device="cuda",
                          dtype=torch.float16 if mode == "split" else DTYPE[mode])
        rc, out = _run(harness_net, mode, qkv, 1, L, heads, head_dim=hd, causal=c.get("causal", 0), fill=7.0)
        assert rc != 0, c
        assert bool((out.float() == 7.0).all()), c
    if mode == "split":
        for h in (1, 3):
            qkv = torch.zeros((64, 6 * h * HD), device="cuda", dtype=torch.float16)
            rc, out = _run(harness_net, mode, qkv, 1, 64, h, fill=7.0)
            assert rc != 0 and bool((out.float() == 7.0).all())
    # head_dim 64 takes the routes it always took: the same bits as the entry point without the argument
    L = 197
    q64 = _device_operands(mode, np.random.default_rng(5).standard_normal((L, 3 * heads * 64)).astype(np.float32))
    rc, a = _run(harness_net, mode, q64, 1, L, heads, head_dim=64)
    assert rc == 0
    lib = harness_net._lib
    b = torch.zeros_like(a)
    if mode == "split":
        rc = lib.mcm_debug_op_attention_split(harness_net._h, _ptr(q64), _ptr(b), 1, L, heads, 0, 0, None)
    else:
        rc = lib.mcm_debug_op_attention(harness_net._h, PREC[mode], _ptr(q64), _ptr(b), 1, L, heads, 0, 0, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(a, b)
    rc, out = _run(harness_net, mode, _device_operands(mode, _qkv(1, 65, heads, 3)), 1, 65, heads)
    assert rc == 0 and torch.isfinite(out.float()).all()
