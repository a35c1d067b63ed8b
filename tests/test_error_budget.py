"""The error budgets of tests/error_budget.py, proved on the CPU: correct emulations of each kernel's arithmetic stay
inside them, and each of a list of plausible kernel mistakes breaks them on at least one case.  This is what makes the
GPU budget tests (test_gpu_error_budget.py) trustworthy without a GPU number; any later loosening of a constant in
error_budget.py has to keep this file green."""
import numpy as np
import pytest

from tests import error_budget as eb

torch = pytest.importorskip("torch")

F32 = np.float32


def _f32(a):
    return np.asarray(a, dtype=F32)


def _round_mant(a, bits):
    """Round-to-nearest-even to `bits` significand bits, fp32 exponent range (tf32: 11, bf16: 8)."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    drop = 24 - bits
    half = (1 << (drop - 1)) - 1
    u = (u + half + ((u >> drop) & 1)) >> drop << drop
    return u.astype(np.uint32).view(F32)


def _trunc16(v, out):
    """fp32 -> 16-bit by truncation (round toward zero) instead of RNE."""
    v = _f32(v)
    if out == "bf16":
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    h = v.astype(np.float16)
    over = np.abs(h.astype(F32)) > np.abs(v)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(F32)


# ---- GEMM emulations ---------------------------------------------------------------------------------------------------
def _dot_seq(x, w, kstep, acc16_step=None, out=None, drop_step=None):
    """fp32 accumulation in the kernel's order: K-steps one after another, each K-step's products summed into the fp32
    accumulator sequentially.  acc16_step: that K-step's partial sum is accumulated in the 16-bit format `out` instead;
    drop_step: that K-step is skipped."""
    M, K = x.shape
    acc = np.zeros((M, w.shape[0]), F32)
    for k0 in range(0, K, kstep):
        st = k0 // kstep
        if st == drop_step:
            continue
        if st == acc16_step:
            part = np.zeros_like(acc)
            for k in range(k0, k0 + kstep):
                part = eb.round_to(part + _f32(x[:, k:k + 1] * w[None, :, k]), out)
            acc = acc + part
            continue
        for k in range(k0, k0 + kstep):
            acc = acc + _f32(x[:, k:k + 1].astype(np.float64) * w[None, :, k])   # MFMA products are exact in 16-bit modes
    return acc


def _quick_gelu_fast(v):
    """common.hpp quick_gelu_fast in fp32: x * rcp(1 + exp2(-1.702 log2(e) x))."""
    arg = _f32(_f32(-1.702 * 1.4426950408889634) * v)
    return _f32(v * _f32(1.0 / _f32(1.0 + _f32(np.exp2(arg.astype(np.float64))))))


def _tanh_gelu(v):
    v64 = v.astype(np.float64)
    return _f32(0.5 * v64 * (1 + np.tanh(np.sqrt(2 / np.pi) * (v64 + 0.044715 * v64 ** 3))))


def _gemm_case(M, N, K, mode, epi, seed, scale_step=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(F32)
    w = (rng.standard_normal((N, K)) * K ** -0.5).astype(F32)
    if scale_step is not None:                      # a K-step of small operands (what a lost K tail would carry)
        ks = 64 if mode != "fp32" else 32
        x[:, scale_step * ks:(scale_step + 1) * ks] *= 2.0 ** -5
    bias = (0.1 * rng.standard_normal(N)).astype(F32)
    resid0 = rng.standard_normal((M, N)).astype(F32)
    if mode != "fp32":
        x, w = eb.round_to(x, mode), eb.round_to(w, mode)
    return x, w, bias, resid0


def _gemm_emulate(x, w, bias, resid0, mode, epi, mutation=None):
    kstep = 64 if mode != "fp32" else 32
    xo, wo, bo = x, w, bias
    if mutation == "tf32":
        xo, wo = _round_mant(x, 11), _round_mant(w, 11)
    if mutation == "bias16":
        bo = eb.round_to(bias, mode)
    if mutation == "bf16x3":
        xh, wh = _round_mant(x, 8), _round_mant(w, 8)
        xl, wl = _round_mant(x - xh, 8), _round_mant(w - wh, 8)
        acc = _dot_seq(xh, wh, kstep) + _dot_seq(xh, wl, kstep) + _dot_seq(xl, wh, kstep)
    else:
        acc = _dot_seq(xo, wo, kstep, acc16_step=0 if mutation == "acc16" else None, out=mode,
                       drop_step=1 if mutation == "drop_step" else None)
    v = _f32(acc + bo[None, :])
    if epi == 2:
        return _f32(resid0 + v)
    if epi == 1:
        if mutation == "tanh_gelu":
            v = _tanh_gelu(v)
        elif mode == "fp32":
            v = _f32(v / (1.0 + np.exp(-1.702 * v.astype(np.float64))))
        else:
            v = _quick_gelu_fast(v)
    if mode == "fp32":
        return v
    return _trunc16(v, mode) if mutation == "trunc" else eb.round_to(v, mode)


def _gemm_ratio(M, N, K, mode, epi, mutation=None, seed=0, scale_step=None):
    x, w, bias, resid0 = _gemm_case(M, N, K, mode, epi, seed, scale_step)
    got = _gemm_emulate(x, w, bias, resid0, mode, epi, mutation)
    lin, s = eb.gemm_reference(x, w, bias)
    ref, bud = eb.gemm_budget(lin, s, mode, epi, resid0)
    return eb.worst(got, ref, bud)[0]


GEMM_CASES = [(65, 208, 192), (129, 144, 64), (17, 272, 256), (300, 256, 128)]


@pytest.mark.parametrize("K", [64, 96, 192, 768, 1024, 3072, 4096])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_c_acc_covers_cpu_dot_products(K, mode):
    """C_ACC is chosen here, not on GPU output: a sequential fp32 dot product and torch's CPU fp32 matmul stay within
    C_ACC / 2 of u32 * sum |x w| at every K (2x margin)."""
    rng = np.random.default_rng(K + 7)
    x = rng.standard_normal((256, K)).astype(F32)
    w = (rng.standard_normal((256, K)) * K ** -0.5).astype(F32)
    if mode == "bf16":
        x, w = eb.round_to(x, "bf16"), eb.round_to(w, "bf16")
    ref, s = eb.gemm_reference(x, w, np.zeros(256, F32))
    acc = np.zeros((256, 256), F32)
    for k in range(K):
        acc = acc + x[:, k:k + 1] * w[None, :, k]
    for name, got in (("sequential", acc), ("torch", (torch.from_numpy(x) @ torch.from_numpy(w).T).numpy())):
        r = float((np.abs(got - ref) / (eb.U32 * s)).max())
        assert r <= eb.C_ACC / 2, (name, K, mode, r)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_correct_emulation_within_budget(mode, epi):
    for M, N, K in GEMM_CASES:
        if mode == "fp32":
            K = K // 2   # the same K-step count
        r = _gemm_ratio(M, N, K, mode, epi, seed=M + N + K)
        assert r <= 1.0, (M, N, K, r)


@pytest.mark.parametrize("mutation,modes,epis", [
    ("trunc", ["bf16", "fp16"], [0, 1]),
    ("bias16", ["bf16", "fp16"], [0, 2]),
    ("tanh_gelu", ["bf16", "fp16", "fp32"], [1]),
    ("drop_step", ["bf16", "fp16", "fp32"], [0, 2]),
    ("acc16", ["bf16", "fp16"], [0, 2]),
    ("tf32", ["fp32"], [0, 2]),
    ("bf16x3", ["fp32"], [0, 2]),
])
def test_gemm_mutations_break_the_budget(mutation, modes, epis):
    """Each deliberate mistake exceeds the budget in every mode and epilogue it applies to (checked on the first of the
    GPU tests' shapes that shows it; the assertion is that at least one does)."""
    for mode in modes:
        for epi in epis:
            worst = 0.0
            for M, N, K in GEMM_CASES:
                if mode == "fp32":
                    K = K // 2
                r = _gemm_ratio(M, N, K, mode, epi, mutation, seed=M + N + K,
                                scale_step=1 if mutation == "drop_step" else None)
                worst = max(worst, r)
                if worst > 1.0:
                    break
            print(f"{mutation} {mode} epi{epi}: worst budget ratio {worst:.3g}")
            assert worst > 1.0, (mutation, mode, epi, worst)


def test_dropped_small_k_step_is_within_budget_when_kept():
    """The operand scaling of the drop_step case alone (nothing dropped) stays within budget."""
    for mode in ("bf16", "fp32"):
        for epi in (0, 2):
            assert _gemm_ratio(65, 208, 192 if mode != "fp32" else 96, mode, epi, seed=7, scale_step=1) <= 1.0


# ---- LayerNorm emulation -----------------------------------------------------------------------------------------------
def _ln_rows(D, seed):
    """The GPU test's rows: benign, constant, mean 1e3 / std 1e-2, one 100-sigma outlier channel."""
    rng = np.random.default_rng(seed)
    M = 23
    x = (rng.standard_normal((M, D)) * 2 + 0.5).astype(F32)
    x[1] = 0.1
    x[2] = -3.75
    x[3:6] = (1e3 + 1e-2 * rng.standard_normal((3, D))).astype(F32)
    x[6:8] = rng.standard_normal((2, D)).astype(F32)
    x[6:8, 5] = 100.0
    g = (1 + 0.1 * rng.standard_normal(D)).astype(F32)
    b = (0.1 * rng.standard_normal(D)).astype(F32)
    return x, g, b


def _ln_emulate(x, g, b, out, single_pass=False, eps=1e-5):
    """ln_row.hpp in fp32: lane partial sums of the row (columns (i * 64 + lane) * 4 + 0..3), the wave butterfly, mean,
    centred sum of squares the same way, rstd = 1 / sqrtf(var / D + eps), fma(c * rstd, g, b)."""
    M, D = x.shape
    eps = F32(eps)

    def wave_total(vals):  # vals [M, D] fp32 -> the kernel's sum order
        nv = (D + 255) // 256
        lane = np.zeros((M, 64), F32)
        for i in range(nv):
            for ln in range(64):
                d = (i * 64 + ln) * 4
                if d < D:
                    v = vals[:, d:d + 4]
                    lane[:, ln] = lane[:, ln] + _f32((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]))
        for o in (32, 16, 8, 4, 2, 1):
            lane = _f32(lane + lane[:, np.arange(64) ^ o])
        return lane[:, :1]

    xs = _f32(x)
    mean = _f32(wave_total(xs) / F32(D))
    if single_pass:
        msq = _f32(wave_total(_f32(xs * xs)) / F32(D))
        var = _f32(msq - _f32(mean * mean))
        c = _f32(xs - mean)
    else:
        c = _f32(xs - mean)
        var = _f32(wave_total(_f32(c * c)) / F32(D))
    rstd = _f32(F32(1) / np.sqrt(_f32(var + eps)))
    y = _f32(_f32(c * rstd).astype(np.float64) * g + b)
    return y if out == "fp32" else eb.round_to(y, out)


@pytest.mark.parametrize("D", [128, 768, 1024])
@pytest.mark.parametrize("out", ["bf16", "fp16", "fp32"])
def test_layernorm_emulation_within_budget_and_single_pass_breaks_it(D, out):
    x, g, b = _ln_rows(D, D)
    ref, bud = eb.layernorm_budget(x, g, b, out)
    r, _ = eb.worst(_ln_emulate(x, g, b, out), ref, bud)
    assert r <= 1.0, r
    with np.errstate(invalid="ignore"):
        r_bad, i = eb.worst(_ln_emulate(x, g, b, out, single_pass=True), ref, bud)
    print(f"layernorm D={D} {out}: correct {r:.3g}, single-pass {r_bad:.3g} (row {i // D})")
    assert r_bad > 1.0


# ---- attention emulation -----------------------------------------------------------------------------------------------
def _attn_emulate(q, k, v, causal, out, rowsum="fp32", p_bits=None):
    """One (sequence, head) as the kernels do it: S = K Q^T with fp32 accumulation, m = row max, e = exp2(s*SC - m*SC)
    (fp32 argument), P = e rounded to the operand format, O = P V (fp32 accumulation) / rowsum.  rowsum "fp32": over the
    fp32 e (attn_bf16_kernel); "P": over the rounded P (attn_tr_kernel's all-ones MFMA); "16bit": a mistake, the row sum
    accumulated in the 16-bit format.  p_bits: P rounded to that many significand bits instead (a mistake)."""
    L = q.shape[0]
    SC = F32(0.125 * 1.4426950408889634)
    s = (torch.from_numpy(_f32(k)) @ torch.from_numpy(_f32(q)).T).numpy().T    # [q, key], fp32
    if causal:
        s = np.where(np.tril(np.ones((L, L), bool)), s, -np.inf).astype(F32)
    m = s.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        arg = _f32(s.astype(np.float64) * SC - _f32(m * SC))
    e = _f32(np.exp2(arg.astype(np.float64)))
    e = np.where(np.isfinite(e), e, 0).astype(F32)
    if out == "fp32":
        p = e
    elif p_bits is not None:
        p = _round_mant(e, p_bits)
    else:
        p = eb.round_to(e, out)
    if rowsum in ("fp32", "P"):   # attn_bf16_kernel's order: lane g of a query adds (e0 + e1) + (e2 + e3) of keys
        src = e if rowsum == "fp32" else p   # t * 16 + g * 4 + 0..3 per 16-key tile t, then two cross-lane adds
        nt = (L + 15) // 16
        pad = np.zeros((L, nt * 16), F32)
        pad[:, :L] = src
        lane = np.zeros((L, 4), F32)
        for t in range(nt):
            blk = pad[:, t * 16:(t + 1) * 16].reshape(L, 4, 4)
            lane = _f32(lane + _f32(_f32(blk[:, :, 0] + blk[:, :, 1]) + _f32(blk[:, :, 2] + blk[:, :, 3])))
        ls = _f32(_f32(lane[:, :2] + lane[:, 2:]).sum(axis=1, keepdims=True, dtype=F32))
    else:
        ls = np.zeros((L, 1), F32)
        for j in range(L):
            ls = eb.round_to(ls + p[:, j:j + 1], out)
    o = (torch.from_numpy(p) @ torch.from_numpy(_f32(v))).numpy()
    o = _f32(o * _f32(F32(1) / ls))
    return o if out == "fp32" else eb.round_to(o, out)


def _attn_case(L, out, seed, spiked=False):
    rng = np.random.default_rng(seed)
    qkv = rng.standard_normal((L, 192)).astype(F32)
    qkv[:, :128] *= 1.5
    if spiked:
        qkv[min(7, L - 1), :64] *= 20.0
        qkv[L // 2, 64:128] *= 10.0
    if out != "fp32":
        qkv = eb.round_to(qkv, out)
    return qkv[:, :64], qkv[:, 64:128], qkv[:, 128:]


ATTN_L = [(1, False), (2, False), (17, False), (50, False), (77, True), (197, False), (197, "spiked")]


@pytest.mark.parametrize("out", ["bf16", "fp16", "fp32"])
def test_attention_emulation_within_budget(out):
    for L, kind in ATTN_L:
        q, k, v = _attn_case(L, out, L, spiked=kind == "spiked")
        causal = kind is True
        ref, bud = eb.attention_budget(q, k, v, causal, out)
        for rowsum in (("fp32", "P") if out != "fp32" else ("fp32",)):
            r, _ = eb.worst(_attn_emulate(q, k, v, causal, out, rowsum=rowsum), ref, bud)
            assert r <= 1.0, (L, kind, rowsum, r)


@pytest.mark.parametrize("mutation,out", [("p8bits", "fp16"), ("rowsum16", "bf16"), ("rowsum16", "fp16")])
def test_attention_mutations_break_the_budget(mutation, out):
    worst = 0.0
    for L, kind in ATTN_L:
        q, k, v = _attn_case(L, out, L, spiked=kind == "spiked")
        causal = kind is True
        ref, bud = eb.attention_budget(q, k, v, causal, out)
        got = _attn_emulate(q, k, v, causal, out, rowsum="16bit" if mutation == "rowsum16" else "fp32",
                            p_bits=8 if mutation == "p8bits" else None)
        worst = max(worst, eb.worst(got, ref, bud)[0])
    print(f"attention {mutation} {out}: worst budget ratio {worst:.3g}")
    assert worst > 1.0


# ---- scores ------------------------------------------------------------------------------------------------------------
def _score_emulate(img, txt, T, kind):
    """score.hip in fp32 / fp64 as the kernel does it (dot products: torch's fp32 matmul)."""
    sim = (torch.from_numpy(_f32(img)) @ torch.from_numpy(_f32(txt)).T).numpy()
    m = sim.max(axis=1, keepdims=True)
    if kind == 1:
        return -m[:, 0]
    T = F32(T)
    mt = _f32(m / T)
    u = _f32(_f32(sim / T) - mt)
    e = _f32(np.exp(u.astype(np.float64)))
    z = e.astype(np.float64).sum(axis=1)
    if kind == 0:
        return _f32(-(1.0 / z))
    if kind == 2:
        return _f32(-(T * _f32(mt[:, 0] + _f32(np.log(z)))))
    if kind == 3:
        ez = (e.astype(np.float64) * u).sum(axis=1)
        return _f32(np.log(z) - ez / z)
    p = _f32(e * _f32(1.0 / z)[:, None])
    mean = p.astype(np.float64).sum(axis=1, keepdims=True) / p.shape[1]
    return _f32(-(((p - mean) ** 2).sum(axis=1) / p.shape[1]))


@pytest.mark.parametrize("K", [1, 2, 1000])
@pytest.mark.parametrize("T", [1.0, 0.01])
def test_score_emulation_within_budget(K, T):
    rng = np.random.default_rng(K)
    img = rng.standard_normal((9, 512)).astype(F32)
    img /= np.linalg.norm(img, axis=1, keepdims=True)
    txt = rng.standard_normal((K, 512)).astype(F32)
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    for kind in range(5):
        ref, bud = eb.score_budget(img, txt, T, kind)
        r, _ = eb.worst(_score_emulate(img, txt, T, kind), ref, bud)
        assert r <= 1.0, (kind, r)


def test_ulp():
    assert eb.ulp(1.0, "bf16") == 2.0 ** -7 and eb.ulp(1.0, "fp16") == 2.0 ** -10 and eb.ulp(1.0, "fp32") == 2.0 ** -23
    assert eb.ulp(0.75, "fp16") == 2.0 ** -11 and eb.ulp(-3.0, "bf16") == 2.0 ** -6
    assert eb.ulp(1e-6, "fp16") == 2.0 ** -24 and eb.ulp(0.0, "fp16") == 2.0 ** -24   # fp16 subnormal spacing
    assert eb.ulp(65504.0, "fp16") == 32.0
    for v in (3.1, 1e-3, 7e4):
        assert eb.ulp(v, "fp32") == float(np.spacing(np.float32(v)))


def test_sample_rows():
    r = eb.sample_rows(77000)
    assert r[0] == 0 and r[-1] == 76999 and 255 in r and 76744 in r
    assert all(b in r and b - 1 in r for b in range(64, 77000, 64))
    assert len(np.unique(r)) == len(r)
