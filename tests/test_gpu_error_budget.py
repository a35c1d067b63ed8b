"""The hot-path kernels against fp64 references under the derived error budgets of tests/error_budget.py (proved to
discriminate on the CPU by tests/test_error_budget.py): the GEMM at the edge shapes of its tiles and at the full-size
shapes the size policy actually routes (on sampled rows), the LayerNorm on hostile rows, attention from 1 to 288 keys and
the shipped persistent form, and all five score kinds up to the largest bank launch_score accepts.

Each check prints "BUDGET <kernel> <precision> <worst max|got - ref| / budget>" (run with -s to collect them)."""

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREC = {"bf16": 0, "fp32": 1, "fp16": 2}
DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}


def _tiny(harness):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    return NativeCLIP(geo, synth_state_dict(geo, 0), precision="bf16", max_batch=64, max_prompt_tokens=4096,
                      harness=harness)


@pytest.fixture(scope="module")
def tiny_net():
    """A handle of the SHIPPED library (libmcm_hip.so): its own kernel choice, no switches."""
    net = _tiny(False)
    yield net
    net.close()


@pytest.fixture(scope="module")
def harness_net():
    """A handle of libmcm_hip_harness.so (same sources, -DMCM_HARNESS): the forced kernel variants."""
    net = _tiny(True)
    yield net
    net.close()


_ptr = gs.ptr


_check = gs.check_budget


# ---- GEMM --------------------------------------------------------------------------------------------------------------
def _linear(net, prec, x, w, bias, resid0, epi):
    M, K = x.shape
    N = w.shape[0]
    y = torch.zeros((M, N), device="cuda", dtype=DTYPE[prec])
    rd = resid0.clone() if epi == 2 else None
    rc = net._lib.mcm_op_linear(net._h, PREC[prec], _ptr(x), _ptr(w), _ptr(bias), _ptr(y), _ptr(rd), M, N, K, epi, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    return rd if epi == 2 else y


def _gemm_operands(M, N, K, prec, seed, with_resid):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((M, K), generator=g, device="cuda").to(DTYPE[prec])
    w = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(DTYPE[prec])
    bias = 0.1 * torch.randn(N, generator=g, device="cuda")
    resid0 = torch.randn((M, N), generator=g, device="cuda") if with_resid else None
    return x, w, bias, resid0


def _gemm_check(net, M, N, K, prec, epi, seed, rows=None, what="gemm"):
    x, w, bias, resid0 = _gemm_operands(M, N, K, prec, seed, epi == 2)
    out = _linear(net, prec, x, w, bias, resid0, epi)
    if rows is None:
        rows = np.arange(M)
    ri = torch.from_numpy(rows).cuda()
    got = out[ri].float().cpu().numpy()
    lin, s = eb.gemm_reference(x[ri].float().cpu().numpy(), w.float().cpu().numpy(), bias.cpu().numpy())
    r0 = resid0[ri].cpu().numpy() if epi == 2 else None
    ref, bud = eb.gemm_budget(lin, s, prec, epi, r0)
    return _check(what, prec, got, ref, bud, f"M={M} N={N} K={K} epi={epi}")


EDGE_N = [16, 48, 80, 144, 208, 240, 272]      # multiples of 16 that are no multiple of 64 / 128 / 256
EDGE_M = [1, 2, 15, 17, 63, 65, 127, 129, 255, 257]
EDGE_K = {"bf16": (64, 192), "fp16": (64, 192), "fp32": (32, 96)}   # one K-step, an odd number of K-steps


@pytest.fixture(params=[-1, 0, 3, 4, 5, 9, 11], ids=["shipped-policy", "tile128", "persist256", "persist256x256",
                                                     "pingpong256x256", "pingpong-arms", "tile64"])
def gemm_net(request, tiny_net, harness_net):
    if request.param < 0:
        yield tiny_net
        return
    assert harness_net._lib.mcm_debug_gemm_variant(request.param) == 0
    yield harness_net
    harness_net._lib.mcm_debug_gemm_variant(-1)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_edge_shapes_within_budget(gemm_net, prec, epi):
    """Every N of EDGE_N at a ragged M (65), every M of EDGE_M at a ragged N (208); K alternates between one K-step and an
    odd number of K-steps."""
    shapes = [(65, n) for n in EDGE_N] + [(m, 208) for m in EDGE_M]
    for i, (M, N) in enumerate(shapes):
        K = EDGE_K[prec][i % 2]
        _gemm_check(gemm_net, M, N, K, prec, epi, seed=1000 * i + 7 * epi + K, what="gemm-edge")


# (tag, M, [(N, K, epi)], extra rows): the shipped policy's full-size problems
FULL = [
    ("B16-b512", 512 * 197, [(2304, 768, 0), (3072, 768, 1), (768, 3072, 2), (768, 768, 2)], ()),
    ("L14-b256", 256 * 257, [(3072, 1024, 0), (4096, 1024, 1), (1024, 4096, 2), (1024, 1024, 2)], ()),
    # the sliver split of launch_gemm cuts the N = 768 problems of ViT-B/32 at batch 512 (out-proj, fc2) at row 80 * 256: ping-pong
    # above, the 64x128 tile kernel below; QKV and fc1 go to the ping-pong kernel whole (tests/test_launch_routes_cpu.py)
    ("B32-b512", 512 * 50, [(2304, 768, 0), (3072, 768, 1), (768, 3072, 2), (768, 768, 2)], (20479, 20480, 20481)),
    # the text tower at K = 1000 prompts: 301 row tiles, the last one ragged -> the ragged persistent kernel
    ("text-K1000", 1000 * 77, [(1536, 512, 0), (512, 512, 2), (2048, 512, 1), (512, 2048, 2)], ()),
]


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("tag,M,shapes,extra", FULL, ids=[f[0] for f in FULL])
def test_gemm_full_size_shipped_within_budget(tiny_net, tag, M, shapes, extra, prec):
    rows = eb.sample_rows(M, extra)
    for j, (N, K, epi) in enumerate(shapes):
        _gemm_check(tiny_net, M, N, K, prec, epi, seed=M + 31 * j, rows=rows, what=f"gemm-{tag}")


def test_gemm_full_size_fp32_within_budget(tiny_net):
    """The exact-fp32 arm at a full-size shape of each routed kernel: whole 256-row tiles and the ragged text tower."""
    for M, N, K, epi in ((25600, 768, 768, 2), (25600, 3072, 768, 1), (77000, 1536, 512, 0)):
        _gemm_check(tiny_net, M, N, K, "fp32", epi, seed=N + K, rows=eb.sample_rows(M), what="gemm-full")


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------
def _layernorm(net, prec, x, g, b):
    M, D = x.shape
    y = torch.empty((M, D), device="cuda", dtype=DTYPE[prec])
    xd, gd, bd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, g, b))
    rc = net._lib.mcm_op_layernorm(net._h, PREC[prec], _ptr(xd), _ptr(gd), _ptr(bd), _ptr(y), M, D, 1e-5, 0, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    return y.float().cpu().numpy()


@pytest.mark.parametrize("D", [128, 768, 1024])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_layernorm_within_budget(tiny_net, D, prec):
    """Benign rows, constant rows (variance 0), rows of mean 1e3 and std 1e-2, rows with one 100-sigma channel; M = 203."""
    rng = np.random.default_rng(D + PREC[prec])
    M = 203
    x = (rng.standard_normal((M, D)) * 2 + 0.5).astype(np.float32)
    x[1], x[2], x[3] = 0.1, -3.75, 0.0
    x[10:30] = (1e3 + 1e-2 * rng.standard_normal((20, D))).astype(np.float32)
    x[40:60] = rng.standard_normal((20, D)).astype(np.float32)
    x[40:60, 5] = 100.0
    x[-1, -1] = -100.0
    g = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    got = _layernorm(tiny_net, prec, x, g, b)
    ref, bud = eb.layernorm_budget(x, g, b, prec)
    _check("layernorm", prec, got, ref, bud, f"D={D}")


def test_layernorm_fp16_saturation_edge_within_budget(tiny_net):
    """Outputs spread around the fp16 limit: the budget holds on every unsaturated element, and every element beyond
    the limit is stored as +-65504."""
    rng = np.random.default_rng(3)
    M, D = 61, 768
    x = rng.standard_normal((M, D)).astype(np.float32)
    g = np.full(D, 3.0e4, np.float32) * (1 + 0.05 * rng.standard_normal(D)).astype(np.float32)
    b = (100 * rng.standard_normal(D)).astype(np.float32)
    got = _layernorm(tiny_net, "fp16", x, g, b)
    ref, bud = eb.layernorm_budget(x, g, b, "fp16")
    sat = ~np.isfinite(bud)
    assert sat.any() and (~sat).any()
    assert np.isfinite(got).all()
    big = np.abs(ref) >= eb.FP16_MAX + 16 + 1.0      # beyond rounding distance of the limit: must saturate
    assert np.array_equal(got[big], np.sign(ref[big]) * eb.FP16_MAX)
    _check("layernorm-sat", "fp16", got, ref, bud, f"D={D}")


# ---- attention ---------------------------------------------------------------------------------------------------------
def _attn_check(what, prec, qkv, out, nseq, L, heads, causal, pairs=None):
    """qkv, out on the device; the fp64 reference on the (sequence, head) pairs given (all by default)."""
    D = heads * 64
    if pairs is None:
        pairs = [(n, h) for n in range(nseq) for h in range(heads)]
    qkv_h = {}
    got_all, ref_all, bud_all = [], [], []
    for n, h in pairs:
        if n not in qkv_h:
            qkv_h[n] = qkv[n * L:(n + 1) * L].float().cpu().numpy()
        rows = qkv_h[n]
        ref, bud = eb.attention_budget(rows[:, h * 64:(h + 1) * 64], rows[:, D + h * 64:D + (h + 1) * 64],
                                       rows[:, 2 * D + h * 64:2 * D + (h + 1) * 64], causal, prec)
        got_all.append(out[n * L:(n + 1) * L, h * 64:(h + 1) * 64].float().cpu().numpy())
        ref_all.append(ref)
        bud_all.append(bud)
    return _check(what, prec, np.stack(got_all), np.stack(ref_all), np.stack(bud_all),
                  f"nseq={nseq} L={L} heads={heads} causal={causal}")


def _attn_qkv(nseq, L, heads, prec, seed, spread=1.5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = heads * 64
    qkv = torch.randn((nseq * L, 3 * D), device="cuda", generator=g)
    qkv[:, :2 * D] *= spread                 # O(1)-spread logits after the 0.125 scale: a non-uniform softmax
    return qkv.to(DTYPE[prec])


def _attention(net, prec, qkv, nseq, L, heads, causal):
    out = torch.zeros((nseq * L, heads * 64), device="cuda", dtype=DTYPE[prec])
    rc = net._lib.mcm_op_attention(net._h, PREC[prec], _ptr(qkv), _ptr(out), nseq, L, heads, int(causal), None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    return out


ATTN_L = [(1, False), (2, False), (15, False), (16, False), (17, False), (50, False), (77, True), (197, False),
          (257, False), (288, False)]


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("L,causal", ATTN_L)
def test_attention_within_budget(tiny_net, L, causal, prec):
    nseq, heads = 3, 2
    qkv = _attn_qkv(nseq, L, heads, prec, seed=L * 7 + causal)
    out = _attention(tiny_net, prec, qkv, nseq, L, heads, causal)
    _attn_check("attention", prec, qkv, out, nseq, L, heads, causal)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_attention_spiked_logits_within_budget(tiny_net, prec):
    """One key dominating the rows of one query (softmax ~ one-hot) and large negative logits elsewhere."""
    nseq, L, heads = 1, 197, 2
    D = heads * 64
    qkv = _attn_qkv(nseq, L, heads, "fp32", seed=5, spread=1.0)
    qkv[7, :D] *= 20.0
    qkv[100, D:2 * D] *= 10.0
    qkv = qkv.to(DTYPE[prec])
    out = _attention(tiny_net, prec, qkv, nseq, L, heads, False)
    assert torch.isfinite(out.float()).all()
    _attn_check("attention-spiked", prec, qkv, out, nseq, L, heads, False)


def test_attention_shipped_persistent_within_budget(tiny_net):
    """The shipped library at B/16 batch 512 (the persistent form, attn_ps_kernel), fp16: ~40 sampled (sequence, head)
    pairs including the first and the last sequence."""
    nseq, L, heads = 512, 197, 12
    qkv = _attn_qkv(nseq, L, heads, "fp16", seed=11, spread=1.3)
    out = _attention(tiny_net, "fp16", qkv, nseq, L, heads, False)
    rng = np.random.default_rng(0)
    pairs = [(0, 0), (0, 11), (511, 0), (511, 11)] + [(int(n), int(h)) for n, h in
                                                      zip(rng.integers(1, 511, 36), rng.integers(0, 12, 36))]
    _attn_check("attention-ps-shipped", "fp16", qkv, out, nseq, L, heads, False, pairs)
    assert tiny_net.kernel_faults == 0


PS_CASES = [(1, 197, 12), (7, 197, 12), (43, 197, 12), (30, 193, 12), (25, 208, 3), (9, 200, 16), (400, 197, 12)]


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("nseq,L,heads", PS_CASES)
def test_attention_forced_persistent_within_budget(harness_net, nseq, L, heads, prec):
    """The persistent form forced at every size (harness variant 21), both walk directions."""
    lib = harness_net._lib
    qkv = _attn_qkv(nseq, L, heads, prec, seed=L * 1000 + nseq, spread=1.4)
    rng = np.random.default_rng(nseq)
    pairs = None
    if nseq * heads > 48:
        pairs = sorted({(0, 0), (nseq - 1, heads - 1)} | {(int(n), int(h)) for n, h in
                                                           zip(rng.integers(0, nseq, 30), rng.integers(0, heads, 30))})
    try:
        assert lib.mcm_debug_attention_variant(21) == 0
        for rev in (0, 1):
            out = torch.zeros((nseq * L, heads * 64), device="cuda", dtype=DTYPE[prec])
            rc = lib.mcm_debug_op_attention(harness_net._h, PREC[prec], _ptr(qkv), _ptr(out), nseq, L, heads, 0, 0, rev,
                                            None)
            assert rc == 0, lib.mcm_last_error(harness_net._h)
            torch.cuda.synchronize()
            _attn_check("attention-ps-forced", prec, qkv, out, nseq, L, heads, False, pairs)
    finally:
        lib.mcm_debug_attention_variant(1)
    assert lib.mcm_kernel_faults(harness_net._h) == 0


# ---- scores ------------------------------------------------------------------------------------------------------------
def _kmax(P):
    """The largest bank launch_score accepts (score.hip: (P + K) * 4 bytes of LDS <= 150 KiB)."""
    return 150 * 1024 // 4 - P


@pytest.mark.parametrize("P", [512, 768])
def test_scores_within_budget(P):
    from mcm_amd.config import SCORE_KINDS

    net = gs.widened_net(P)
    try:
        B = 17
        for K in (1, 2, 1000, 21841, _kmax(P)):
            g = torch.Generator(device="cuda").manual_seed(K + P)
            img = torch.randn((B, P), generator=g, device="cuda")
            img = img / img.norm(dim=1, keepdim=True)
            txt = torch.randn((K, P), generator=g, device="cuda")
            txt = txt / txt.norm(dim=1, keepdim=True)
            img_h, txt_h = img.cpu().numpy(), txt.cpu().numpy()
            for T in (1.0, 0.01):
                for name, kind in SCORE_KINDS.items():
                    got = net.score_features(img, txt, T, name).cpu().numpy()
                    ref, bud = eb.score_budget(img_h, txt_h, T, kind)
                    _check(f"score-{name}", "fp32", got, ref, bud, f"P={P} K={K} T={T}")
        # one past the LDS limit: refused with an error, nothing launched
        K = _kmax(P) + 1
        txt = torch.randn((K, P), device="cuda")
        with pytest.raises(RuntimeError):
            net.score_features(img, txt, 1.0, "MCM")
        torch.cuda.synchronize()
    finally:
        net.close()
