"""The split forms (one value carried as an fp16 pair, hi = round(v), lo = round(v - hi)) against fp64
references under the budgets of tests/error_budget.py (proved to discriminate on the CPU by tests/test_error_budget.py):
  * the split GEMMs of mcm_op_linear_ex (SPLIT_X, SPLIT_X | SPLIT_OUT, SPLIT_W | SPLIT_X with and without SPLIT_OUT, SPLIT_W
    alone in fp16 and bf16) at ragged M and N, K = 64 ... 4096, rows of magnitude 2^-12 ... 2^8, against the merged operands
    and, with split activations, against the unsplit fp32 operands; and at the full-size problems the split arm runs, on
    sampled rows (the sliver cut of ViT-B/32 at batch 512 included);
  * mcm_op_layernorm_split on hostile rows and on small-gamma channels (outputs with a subnormal lo);
  * mcm_op_attention_split at every tile-count boundary of launch_tr_x2 and in the streaming form, with spiked logits and
    the coherent small-P input of error_budget.coherent_small_p_qkv (what the 2^12 scale of P is for);
  * qrows = 1 and the reverse walk (mcm_debug_op_attention_split, harness library): bit-identical rows;
  * the canonical form of every split pair a kernel writes, exactly: lo finite, |lo| at most half the spacing of the format
    at hi on lo's side;
  * the range edge: what the pair holds from 65504 to 2e5, and what mcm_saturation_count counts.

Each budget check prints "BUDGET <what> split <worst max|got - ref| / budget>" (run with -s to collect them)."""
import ctypes

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gpu_scaffold as gs
from tests import online_softmax_budget as ob

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREC = {"bf16": 0, "fp16": 2}
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
SPLIT_W, SPLIT_X, SPLIT_OUT = 1, 2, 4


def _tiny(harness):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    return NativeCLIP(geo, synth_state_dict(geo, 0, "fp16-exact"), precision="fp16", max_batch=64, max_prompt_tokens=4096,
                      harness=harness)


@pytest.fixture(scope="module")
def net():
    """An fp16 handle of the SHIPPED library (the split forms run the shipped kernels only: they refuse forced variants)."""
    n = _tiny(False)
    yield n
    n.close()


@pytest.fixture(scope="module")
def harness_net():
    """A handle of libmcm_hip_harness.so: mcm_debug_op_attention_split's qrows and walk direction."""
    n = _tiny(True)
    yield n
    n.close()


_ptr = gs.ptr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(what, got, ref, bud, where=""):
    return gs.check_budget(what, "split", got, ref, bud, where)


def _decode(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(dtype).double().numpy()


def _canonical(what, img, dtype=torch.float16):
    """Exact check of a split image [M, 2N] a kernel wrote: every lo finite, and |lo| <= half the spacing of the format at
    hi on lo's side (equality allowed: what round-to-nearest-even of v and of v - hi gives), for every pair below the
    range edge (|hi| < the format's max)."""
    b = img.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF
    M, N2 = b.shape
    b = b.reshape(M, N2 // 128, 2, 64)
    hb, lb = b[:, :, 0, :].ravel(), b[:, :, 1, :].ravel()
    hi, lo = _decode(hb, dtype), _decode(lb, dtype)
    assert np.isfinite(lo).all() and np.isfinite(hi).all(), f"{what}: a non-finite half"
    mag, sgn = hb & 0x7FFF, hb & 0x8000
    away = (lo > 0) == (hi > 0)                       # lo's side of hi is away from zero
    nb = np.where(mag == 0, np.where(lo < 0, 0x8001, 0x0001), sgn | np.where(away, mag + 1, np.maximum(mag - 1, 0)))
    gap = np.abs(_decode(nb, dtype) - hi)
    bad = (np.abs(hi) < float(torch.finfo(dtype).max)) & (lo != 0) & (np.abs(lo) > 0.5 * gap)
    assert not bad.any(), f"{what}: {int(bad.sum())} non-canonical pairs, e.g. hi {hi[bad][:4]} lo {lo[bad][:4]}"


# ---- GEMM, op level ----------------------------------------------------------------------------------------------------
def _linear(net, prec, flags, x, w, bias, resid0, M, N, K, epi):
    """mcm_op_linear_ex; returns the output: the split image [M, 2N], the 16-bit [M, N], or the fp32 residual."""
    if epi == 2:
        out, y = resid0.clone(), None
    elif flags & SPLIT_OUT:
        out = y = torch.zeros((M, 2 * N), device="cuda", dtype=torch.float16)
    else:
        out = y = torch.zeros((M, N), device="cuda", dtype=DTYPE[prec])
    rc = net._lib.mcm_op_linear_ex(net._h, PREC[prec], _ptr(x), _ptr(w), _ptr(bias), _ptr(y),
                                   _ptr(out) if epi == 2 else None, M, N, K, epi, flags, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    return out


def _split_weight(net, prec, w32):
    """mcm_op_split_weight of the fp32 device weight [N, K]: the image (checked canonical) and its merged value (fp64)."""
    N, K = w32.shape
    img = torch.empty((N, 2 * K), device="cuda", dtype=DTYPE[prec])
    assert net._lib.mcm_op_split_weight(net._h, PREC[prec], _ptr(w32), N, K, _ptr(img), None) == 0
    torch.cuda.synchronize()
    _canonical("split-weight", img, DTYPE[prec])
    return img, eb.merge_image(img.double().cpu().numpy())


def _gemm_check(what, prec, flags, epi, got, x32, xm, w32, wm, bias, resid0, where):
    """got: the device output rows; x32 / w32: the unsplit fp32 operands, xm / wm: the merged (or plain) ones (host)."""
    lin, s = eb.gemm_reference(xm, wm, bias)
    out_split = bool(flags & SPLIT_OUT)
    if out_split:
        _canonical(what, got)
        g = eb.merge_image(got.cpu().numpy())
        ref, bud = eb.gemm_split_budget(lin, s, epi, True)
    elif epi == 2:
        g = got.cpu().numpy()
        ref, bud = eb.gemm_split_budget(lin, s, 2, False, resid0)
    else:
        g = got.float().cpu().numpy()
        ref, bud = eb.gemm_budget(lin, s, prec, epi)
    _check(what, g, ref, bud, where)
    if flags & SPLIT_X:   # the arm's own claim: fp32 round-off of the unsplit operands, plus their split's representation
        ref, bud = eb.gemm_unsplit_budget(x32, w32, bias, epi, out_split, resid0, True, bool(flags & SPLIT_W))
        _check(what + "-unsplit", g, ref, bud, where)


FORMS = [  # (id, prec, flags, epilogues)
    ("X", "fp16", SPLIT_X, (0, 1, 2)),
    ("X-OUT", "fp16", SPLIT_X | SPLIT_OUT, (0, 1)),
    ("W-X", "fp16", SPLIT_W | SPLIT_X, (0, 1, 2)),
    ("W-X-OUT", "fp16", SPLIT_W | SPLIT_X | SPLIT_OUT, (0, 1)),
    ("W-fp16", "fp16", SPLIT_W, (0, 1, 2)),
    ("W-bf16", "bf16", SPLIT_W, (0, 1, 2)),
]
OP_M = [1, 63, 64, 65, 255, 257, 1000]
OP_K = [64, 192, 640, 3072, 4096]        # one logical K-step, an odd number of them, L/14's padded patch K, B/16 / L/14 fc2
N_OUT = [64, 128, 192, 256, 320]         # split outputs: whole 64-column blocks
N_PLAIN = [16, 48, 80, 144, 208, 272]    # ragged multiples of 16


def _row_sweep(M):
    """Per-row magnitudes 2^-12 ... 2^8 in turn."""
    return 2.0 ** (-12 + (np.arange(M) % 21))


@pytest.mark.parametrize("form,prec,flags,epis", FORMS, ids=[f[0] for f in FORMS])
def test_split_gemm_op_level_within_budget(net, form, prec, flags, epis):
    Ns = N_OUT if flags & SPLIT_OUT else N_PLAIN
    for epi in epis:
        for i, M in enumerate(OP_M):
            K, N = OP_K[i % len(OP_K)], Ns[i % len(Ns)]
            rng = np.random.default_rng(1000 * i + 10 * epi + flags)
            x32 = (rng.standard_normal((M, K)) * _row_sweep(M)[:, None]).astype(np.float32)
            w32 = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
            bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
            resid0 = rng.standard_normal((M, N)).astype(np.float32)
            if flags & SPLIT_X:
                ximg = eb.split_image(x32)
                x, xm = _dev(ximg), eb.merge_image(ximg)
            else:
                x = _dev(x32).to(DTYPE[prec])
                xm = x.double().cpu().numpy()
            if flags & SPLIT_W:
                wd32 = _dev(w32)
                w, wm = _split_weight(net, prec, wd32)
            else:
                w = _dev(w32).to(DTYPE[prec])
                wm = w.double().cpu().numpy()
                w32 = wm.astype(np.float32)
            bd, rd = _dev(bias), _dev(resid0)
            got = _linear(net, prec, flags, x, w, bd, rd, M, N, K, epi)
            _gemm_check(f"gemm-{form}", prec, flags, epi, got, x32, xm, w32, wm, bias, resid0,
                        f"M={M} N={N} K={K} epi={epi}")


# ---- GEMM, full size ---------------------------------------------------------------------------------------------------
# (tag, width D, tokens, images, padded patch K, patches per image, extra rows): the problems the split arm runs when it
# refines (half the batch) or scores a whole run (--dtype fp16x2: the full batch)
FULL = [
    ("B16-b256", 768, 197, 256, 768, 196, ()),
    ("B16-b512", 768, 197, 512, 768, 196, ()),
    ("B32-b512", 768, 50, 512, 3072, 49, (20479, 20480, 20481)),   # the sliver cut of launch_gemm at row 80 * 256
    ("L14-b256", 1024, 257, 256, 640, 256, ()),
    ("L14-336-b128", 1024, 577, 128, 640, 576, ()),
]


def _dev_split(x):
    """fp32 device [M, K] -> its split image [M, 2K] (split2's bits for values inside the fp16 range)."""
    M, K = x.shape
    hi = x.half()
    lo = (x - hi.float()).half()
    return torch.stack((hi.view(M, K // 64, 64), lo.view(M, K // 64, 64)), dim=2).reshape(M, 2 * K)


@pytest.mark.parametrize("tag,D,L,B,kpad,npatch,extra", FULL, ids=[f[0] for f in FULL])
def test_split_gemm_full_size_within_budget(net, tag, D, L, B, kpad, npatch, extra):
    """QKV (split in, split out), out-proj (residual), fc1 (EPI_GELU_X2), fc2 (residual) and the patch GEMM at K = kpad,
    operands made on the device, rows of magnitude 2^-12 ... 2^8, the fp64 reference on eb.sample_rows; at B/16 batch 256
    also the split-weight regime (fp32-valued weights: four passes per logical K-step)."""
    M = B * L
    shapes = [("qkv", M, 3 * D, D, 0, SPLIT_X | SPLIT_OUT), ("out-proj", M, D, D, 2, SPLIT_X),
              ("fc1", M, 4 * D, D, 1, SPLIT_X | SPLIT_OUT), ("fc2", M, D, 4 * D, 2, SPLIT_X),
              ("patch", B * npatch, D, kpad, 2, SPLIT_X)]
    if tag == "B16-b256":
        shapes += [("qkv-wsplit", M, 3 * D, D, 0, SPLIT_W | SPLIT_X | SPLIT_OUT), ("fc2-wsplit", M, D, 4 * D, 2, SPLIT_W | SPLIT_X)]
    for j, (name, m, N, K, epi, flags) in enumerate(shapes):
        rows = eb.sample_rows(m, extra)
        ri = torch.from_numpy(rows).cuda()
        g = torch.Generator(device="cuda").manual_seed(m + 31 * j)
        sweep = torch.from_numpy(_row_sweep(m).astype(np.float32)).cuda()
        x = torch.randn((m, K), generator=g, device="cuda") * sweep[:, None]
        w32 = torch.randn((N, K), generator=g, device="cuda") * K ** -0.5
        bias = 0.1 * torch.randn(N, generator=g, device="cuda")
        resid0 = torch.randn((m, N), generator=g, device="cuda") if epi == 2 else None
        ximg = _dev_split(x)
        if flags & SPLIT_W:
            w, wm = _split_weight(net, "fp16", w32)
        else:
            w = w32.half()
            wm = w.double().cpu().numpy()
            w32 = w.float()
        out = _linear(net, "fp16", flags, ximg, w, bias, resid0, m, N, K, epi)
        _gemm_check(f"gemm-{tag}-{name}", "fp16", flags, epi, out[ri], x[ri].cpu().numpy(),
                    eb.merge_image(ximg[ri].cpu().numpy()), w32.cpu().numpy(), wm, bias.cpu().numpy(),
                    resid0[ri].cpu().numpy() if epi == 2 else None, f"M={m} N={N} K={K} epi={epi}")
        del x, ximg, out, resid0
    assert net.kernel_faults == 0


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 768, 1024])
def test_layernorm_split_within_budget(net, D):
    """The hostile rows of test_gpu_error_budget.py (constant, mean 1e3 / std 1e-2, a 100-sigma channel) and every 5th
    channel with gamma ~ 2^-8, whose outputs have a subnormal lo."""
    rng = np.random.default_rng(D + 5)
    M = 203
    x = (rng.standard_normal((M, D)) * 2 + 0.5).astype(np.float32)
    x[1], x[2], x[3] = 0.1, -3.75, 0.0
    x[10:30] = (1e3 + 1e-2 * rng.standard_normal((20, D))).astype(np.float32)
    x[40:60] = rng.standard_normal((20, D)).astype(np.float32)
    x[40:60, 5] = 100.0
    x[-1, -1] = -100.0
    g = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    g[::5] *= np.float32(2.0 ** -8)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    y = torch.zeros((M, 2 * D), device="cuda", dtype=torch.float16)
    xd, gd, bd = _dev(x), _dev(g), _dev(b)
    rc = net._lib.mcm_op_layernorm_split(net._h, _ptr(xd), _ptr(gd), _ptr(bd), _ptr(y), M, D, 1e-5, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    _canonical("layernorm", y)
    ref, bud = eb.layernorm_split_budget(x, g, b)
    _check("layernorm", eb.merge_image(y.cpu().numpy()), ref, bud, f"D={D}")


# ---- attention ---------------------------------------------------------------------------------------------------------
SHORT_L = [1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 197, 208, 209, 256, 257, 272, 273, 288]
LONG_L = [289, 320, 577, 1024, 1025]
HEADS = [1, 12, 16]


def _attn_img(nseq, L, heads, seed, spiked=False):
    rng = np.random.default_rng(seed)
    D = heads * 64
    qkv = rng.standard_normal((nseq * L, 3 * D)).astype(np.float32)
    qkv[:, :2 * D] *= 1.5
    if spiked:   # one query (sequence 0) and one key row scaled up: near one-hot softmax rows, large negative logits
        qkv[min(7, L - 1), :D] *= 20.0
        qkv[L // 2, D:2 * D] *= 10.0
    return eb.split_image(qkv)


def _attention_split(net, img, nseq, L, heads):
    out = torch.zeros((nseq * L, 2 * heads * 64), device="cuda", dtype=torch.float16)
    rc = net._lib.mcm_op_attention_split(net._h, _ptr(img), _ptr(out), nseq, L, heads, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    return out


def _attn_check(what, img, out, nseq, L, heads, pairs=None):
    """The fp64 reference on the (sequence, head) pairs given (all by default), under the whole-row split budget up to 288
    keys and the streaming one past it."""
    if pairs is None:
        pairs = [(n, h) for n in range(nseq) for h in range(heads)]
    _canonical(what, out)
    out_h = out.cpu().numpy()
    got_all, ref_all, bud_all = [], [], []
    for n, h in pairs:
        parts = eb.head_parts(img, L, heads, n, h)
        ref, bud = (eb.attention_split_budget if L <= 288 else ob.online_attention_split_budget)(*parts)
        got_all.append(eb.merge_image(out_h[n * L:(n + 1) * L])[:, h * 64:(h + 1) * 64])
        ref_all.append(ref)
        bud_all.append(bud)
    return _check(what, np.stack(got_all), np.stack(ref_all), np.stack(bud_all), f"nseq={nseq} L={L} heads={heads}")


def _pairs(nseq, heads, seed):
    if nseq * heads <= 6:
        return None
    rng = np.random.default_rng(seed)
    return sorted({(0, 0), (nseq - 1, heads - 1)} | {(int(n), int(h)) for n, h in
                                                     zip(rng.integers(0, nseq, 4), rng.integers(0, heads, 4))})


@pytest.mark.parametrize("L", SHORT_L + LONG_L)
def test_attention_split_within_budget(net, L):
    """Every tile-count boundary of launch_tr_x2 (NT = 2, 4, 8, 13 with its NFULL = 12 form, 17, 18) and the streaming form;
    heads 1, 12, 16 in turn, two sequences."""
    nseq, heads = 2, HEADS[(SHORT_L + LONG_L).index(L) % 3]
    img = _attn_img(nseq, L, heads, seed=L)
    out = _attention_split(net, _dev(img), nseq, L, heads)
    _attn_check("attention", img, out, nseq, L, heads, _pairs(nseq, heads, L))


@pytest.mark.parametrize("L", [197, 577])
def test_attention_split_spiked_logits_within_budget(net, L):
    nseq, heads = 2, 2
    img = _attn_img(nseq, L, heads, seed=L + 1, spiked=True)
    out = _attention_split(net, _dev(img), nseq, L, heads)
    _attn_check("attention-spiked", img, out, nseq, L, heads)


@pytest.mark.parametrize("L", [197, 288, 577, 1024])
def test_attention_split_coherent_small_p_within_budget(net, L):
    """Many keys at one equal logit far below the max, V of one sign: P's lo halves would all miss the same way on fp16's
    subnormal grid without the 2^12 pre-scale (tests/test_error_budget.py: that mistake breaks this budget by 80x - 150x)."""
    nseq, heads = 2, 2
    img = eb.split_image(eb.coherent_small_p_qkv(L, heads, nseq))
    out = _attention_split(net, _dev(img), nseq, L, heads)
    _attn_check("attention-coherent-p", img, out, nseq, L, heads)


@pytest.mark.parametrize("L", [17, 50, 197, 257, 288, 577])
def test_attention_split_cls_rows_and_walk_direction_bitwise(net, harness_net, L):
    """qrows = 1 (the CLS-only last layer) and the reverse walk, through mcm_debug_op_attention_split: every row of the
    reverse walk and row 0 of every sequence under qrows = 1 equal the shipped call bit for bit."""
    nseq, heads = 3, 2
    img = _dev(_attn_img(nseq, L, heads, seed=L + 2))
    full = _attention_split(net, img, nseq, L, heads)
    lib = harness_net._lib
    cls = torch.arange(nseq, device="cuda") * L
    for qrows, rev in ((0, 0), (0, 1), (1, 0), (1, 1)):
        out = torch.zeros_like(full)
        rc = lib.mcm_debug_op_attention_split(harness_net._h, _ptr(img), _ptr(out), nseq, L, heads, qrows, rev, None)
        assert rc == 0, lib.mcm_last_error(harness_net._h)
        torch.cuda.synchronize()
        if qrows == 0:
            assert torch.equal(out, full), (qrows, rev)
        else:
            assert torch.equal(out[cls], full[cls]), (qrows, rev)


# ---- the range edge ----------------------------------------------------------------------------------------------------
EDGE = [65504.0, 65519.0, 65520.0, 1e5, 131008.0, 2e5]


def _sat_count(net):
    n = ctypes.c_uint64(0)
    assert net._lib.mcm_saturation_count(net._h, 1, ctypes.byref(n), None) == 0
    return int(n.value)


def _expect_pair(what, hi, lo, v):
    """The pair the kernel stored for the fp32 value v: split2's bits, i.e. below 65520 the RNE pair; from there hi = 65504
    (FP16_OVFL) and lo = round(v - 65504), itself saturated past 131008 + 16."""
    want_hi, want_lo = eb.split2_f16(np.float32(v))
    assert (hi == torch.tensor(float(want_hi), dtype=torch.float16)).all(), (what, v, hi[:2], want_hi)
    assert (lo == torch.tensor(float(want_lo), dtype=torch.float16)).all(), (what, v, lo[:2], want_lo)
    if abs(v) >= eb.FP16_SAT:
        assert abs(float(want_hi)) == eb.FP16_MAX and float(want_lo) == float(eb.f16_sat(np.float32(v - np.sign(v) * 65504.0)))
    if abs(v) <= 131008.0:
        assert float(want_hi) + float(want_lo) == v


def test_split_pairs_at_the_fp16_range_edge(net):
    """A GEMM X2 epilogue (x = 0, w = 0, bias = v: the fp32 value is exactly v; EPI_GELU_X2 too for v > 0, where QuickGELU is
    the identity in fp32) and the LayerNorm split (gamma = 0, beta = v) store the values 65504, 65519, 65520, 1e5, 131008,
    2e5 (both signs): the pair is split2's, and mcm_saturation_count counts exactly the calls with |v| >= 65520."""
    assert net._lib.mcm_saturation_check(net._h, 1) == 0
    _sat_count(net)
    M, N, K, D = 64, 64, 64, 128
    x = torch.zeros((M, 2 * K), device="cuda", dtype=torch.float16)
    w = torch.zeros((N, K), device="cuda", dtype=torch.float16)
    xl = torch.randn((4, D), device="cuda")
    gl = torch.zeros(D, device="cuda")
    for v in [s * e for e in EDGE for s in (1.0, -1.0)]:
        counted = abs(v) >= eb.FP16_SAT
        for epi in ((0, 1) if v > 0 else (0,)):
            bias = torch.full((N,), 0.5, device="cuda")
            bias[3] = v
            y = _linear(net, "fp16", SPLIT_X | SPLIT_OUT, x, w, bias, None, M, N, K, epi)
            _expect_pair(f"gemm epi{epi}", y[:, 3], y[:, 64 + 3], v)
            assert (_sat_count(net) > 0) == counted, (epi, v)
        bl = torch.full((D,), 0.25, device="cuda")
        bl[70] = v
        y = torch.zeros((4, 2 * D), device="cuda", dtype=torch.float16)
        assert net._lib.mcm_op_layernorm_split(net._h, _ptr(xl), _ptr(gl), _ptr(bl), _ptr(y), 4, D, 1e-5, None) == 0
        torch.cuda.synchronize()
        _expect_pair("layernorm", y[:, 128 + 6], y[:, 128 + 64 + 6], v)   # column 70: block 1, offset 6
        assert (_sat_count(net) > 0) == counted, ("layernorm", v)
