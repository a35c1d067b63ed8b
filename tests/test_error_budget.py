"""The error budgets of tests/error_budget.py, proved on the CPU: correct emulations of each kernel's arithmetic stay
inside them, and each of a list of plausible kernel mistakes breaks them on at least one case.  This is what makes the
GPU budget tests (test_gpu_error_budget.py) trustworthy without a GPU number; any later loosening of a constant in
error_budget.py has to keep this file green.

The split forms (test_gpu_split_budget.py) are proved the same way: emulations of the split GEMMs in every flag combination
(the kernel's pass order per logical K-step), of the LayerNorm split and of both split attention forms stay inside their
budgets, rows of magnitude 2^-12 ... 2^-4 included; each planted mistake breaks them: a lo pass dropped for the first or
last K-step, X_lo paired with the next K-step's W, a subnormal lo flushed on the operand or the output side, the output's
lo dropped, K_hi Q_lo or V_hi P_lo dropped, P split without its 2^12 scale (on error_budget.coherent_small_p_qkv), W_lo
dropped.  EPI_GELU_X2 computed with quick_gelu_fast is the one listed mistake no input within the op's contract shows: it
is pinned as undetectable (test_gelu_fast_in_the_split_epilogue_stays_inside_the_budget).

The causal mask (test_gpu_text_lengths.py sweeps every prompt length 1 ... 77 under attention_budget): the correct emulation
stays inside the budget on both sides of every key-tile boundary, and each of three wrong masks (one future key visible, the
diagonal tile taken as full, the diagonal excluded) breaks it at EVERY length 2 ... 77."""
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


def _ln_emulate(x, g, b, out, single_pass=False, eps=1e-5, no_column_test=False):
    """ln_row.hpp in fp32: lane partial sums of the row (columns (i * 64 + lane) * 4 + 0..3), the wave butterfly, mean,
    centred sum of squares the same way, rstd = 1 / sqrtf(var / D + eps), fma(c * rstd, g, b).
    no_column_test: ln_has without its "column < D" test: the lanes of the last, partial vector slot whose columns lie past
    the row add what is there — the start of the next row (zeros after the last one) — into the row's sums."""
    M, D = x.shape
    eps = F32(eps)
    xs = _f32(x)
    W = D                   # columns a lane's "do I hold this vector" test lets through
    if no_column_test:      # every slot whole: each row followed by what lies behind it in memory
        W = (D + 255) // 256 * 256
        flat = np.concatenate([xs.ravel(), np.zeros(W, F32)])
        xs = np.stack([flat[r * D:r * D + W] for r in range(M)])

    def wave_total(vals):  # vals [M, W] fp32 -> the kernel's sum order
        nv = (D + 255) // 256
        lane = np.zeros((M, 64), F32)
        for i in range(nv):
            for ln in range(64):
                d = (i * 64 + ln) * 4
                if d < W:
                    v = vals[:, d:d + 4]
                    lane[:, ln] = lane[:, ln] + _f32((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]))
        for o in (32, 16, 8, 4, 2, 1):
            lane = _f32(lane + lane[:, np.arange(64) ^ o])
        return lane[:, :1]

    mean = _f32(wave_total(xs) / F32(D))
    if single_pass:
        msq = _f32(wave_total(_f32(xs * xs)) / F32(D))
        var = _f32(msq - _f32(mean * mean))
        c = _f32(xs - mean)
    else:
        c = _f32(xs - mean)
        var = _f32(wave_total(_f32(c * c)) / F32(D))
    c = c[:, :D]
    rstd = _f32(F32(1) / np.sqrt(_f32(var + eps)))
    y = _f32(_f32(c * rstd).astype(np.float64) * g + b)
    return y if out == "fp32" else eb.round_to(y, out)


# 192 ... 1216: widths inside mcm_create's envelope with a partial 256-column vector slot, alone (192) or behind whole ones
# (320, 832; 1088 and 1216: the five-vector kernels of layernorm.hip with a partial fifth vector)
@pytest.mark.parametrize("D", [128, 768, 1024, 192, 320, 832, 1088, 1216])
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


@pytest.mark.parametrize("D", [192, 320, 832, 1088, 1216])
@pytest.mark.parametrize("out", ["bf16", "fp16", "fp32"])
def test_layernorm_partial_vector_without_its_column_test_breaks_the_budget(D, out):
    """A partial last vector slot whose lanes skip the "column < D" test (ln_row.hpp ln_has) takes the next row's first
    columns into the mean and the variance: far outside the budget at every such width, on the GPU test's own rows."""
    x, g, b = _ln_rows(D, D)
    ref, bud = eb.layernorm_budget(x, g, b, out)
    with np.errstate(invalid="ignore"):
        r_bad, _ = eb.worst(_ln_emulate(x, g, b, out, no_column_test=True), ref, bud)
    print(f"layernorm D={D} {out}: no column test {r_bad:.3g}")
    assert r_bad > 1.0


# ---- attention emulation -----------------------------------------------------------------------------------------------
CAUSAL_MASK_MISTAKES = ("future_key", "diag_tile_full", "no_diagonal")


def _causal_mask(L, mask=None):
    """[q, key] visibility of the causal kernels, `key < L && key <= q` (attention.hip mask_tile; jmax = q + 1 in the fp32
    kernel), or one of CAUSAL_MASK_MISTAKES: "future_key" (key <= q + 1: one future key visible), "diag_tile_full" (the
    16-key tile that holds the diagonal taken as a full tile: key < (q // 16 + 1) * 16), "no_diagonal" (key < q: row 0 is
    left with no key at all)."""
    q, key = np.arange(L)[:, None], np.arange(L)[None, :]
    if mask is None:
        return key <= q
    return {"future_key": key <= q + 1, "diag_tile_full": key < (q // 16 + 1) * 16, "no_diagonal": key < q}[mask]


def _attn_emulate(q, k, v, causal, out, rowsum="fp32", p_bits=None, mask=None):
    """One (sequence, head) as the kernels do it: S = K Q^T with fp32 accumulation, m = row max, e = exp2(s*SC - m*SC)
    (fp32 argument), P = e rounded to the operand format, O = P V (fp32 accumulation) / rowsum.  rowsum "fp32": over the
    fp32 e (attn_bf16_kernel); "P": over the rounded P (attn_tr_kernel's all-ones MFMA); "16bit": a mistake, the row sum
    accumulated in the 16-bit format.  p_bits: P rounded to that many significand bits instead (a mistake).  mask: one of
    CAUSAL_MASK_MISTAKES in place of the causal mask (a mistake; a row left without keys comes out NaN)."""
    L = q.shape[0]
    SC = F32(0.125 * 1.4426950408889634)
    s = (torch.from_numpy(_f32(k)) @ torch.from_numpy(_f32(q)).T).numpy().T    # [q, key], fp32
    if causal:
        s = np.where(_causal_mask(L, mask), s, -np.inf).astype(F32)
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
    with np.errstate(divide="ignore", invalid="ignore"):
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
# causal lengths on both sides of every key-tile boundary the text tower's 1 ... 77 tokens cross (NT = 1 ... 5)
ATTN_L += [(L, True) for L in (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 76)]


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


@pytest.mark.parametrize("out", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("mutation", CAUSAL_MASK_MISTAKES)
def test_causal_mask_mutations_break_the_budget(mutation, out):
    """Each wrong causal mask, with the kernels' own rounding emulated, misses the budget at EVERY length 2 ... 77 and in
    both row-sum forms, not only at the worst of a list: a mask that is wrong at one untested length only cannot hide (at
    L = 1 none of the three can show: one query, one key).  "no_diagonal" leaves row 0 without a key (NaN, an infinite
    ratio); its ratio is taken over rows 1 ... so that the figure says what the visible rows show."""
    low = (np.inf, None)
    for L in range(2, 78):
        q, k, v = _attn_case(L, out, L)
        ref, bud = eb.attention_budget(q, k, v, True, out)
        rows = slice(1, None) if mutation == "no_diagonal" else slice(None)
        for rowsum in (("fp32", "P") if out != "fp32" else ("fp32",)):
            assert eb.worst(_attn_emulate(q, k, v, True, out, rowsum=rowsum), ref, bud)[0] <= 1.0, (L, rowsum)
            got = _attn_emulate(q, k, v, True, out, rowsum=rowsum, mask=mutation)
            r = eb.worst(got[rows], ref[rows], bud[rows])[0]
            assert r > 1.0, (mutation, out, L, rowsum, r)
            low = min(low, (r, L))
    print(f"MUTATION causal-mask {mutation} {out}: smallest budget ratio over L = 2 ... 77: {low[0]:.3g} at L={low[1]}")


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


# ---- Mahalanobis -------------------------------------------------------------------------------------------------------
def _maha_emulate(feats, means, prec, mutation=None):
    """maha_prepare_kernel + maha_score_kernel (score.hip): the expanded form d_c = q - W_c . f + k_c accumulated in fp64 from
    the fp32 inputs, min over the classes, 0.5 * and one rounding to fp32.  mutation:
      "fp32"       the expanded form accumulated in fp32
      "symmetric"  W_c = 2 P mu_c (a symmetrised P) for P mu_c + P^T mu_c
      "drop_last"  the last class never looked at
      "max"        max over the classes for min"""
    t = np.float32 if mutation == "fp32" else np.float64
    f, mu, p = (np.asarray(a, t) for a in (feats, means, prec))
    if mutation == "drop_last":
        mu = mu[:-1]
    pm = mu @ p.T                                              # rows (P mu_c)^T
    w = 2 * pm if mutation == "symmetric" else pm + mu @ p     # + (P^T mu_c)^T
    k = np.einsum("cp,cp->c", mu, pm)
    q = np.einsum("bp,bp->b", f @ p.T, f)
    d = q[:, None] - f @ w.T + k[None, :]
    m = d.max(axis=1) if mutation == "max" else d.min(axis=1)
    return _f32(0.5 * m.astype(np.float64))


@pytest.mark.parametrize("pkind", ["asym", "scaled"])
@pytest.mark.parametrize("P,C", [(64, 1), (64, 17), (100, 15), (512, 16), (768, 1000)])
def test_maha_emulation_within_budget(P, C, pkind):
    for where in ("far", "near", "equal", "mixed"):
        feats, means, prec = eb.maha_case(P, C, 9, where, pkind)
        ref, bud = eb.maha_budget(feats, means, prec)
        if where == "equal":
            assert (ref == 0.0).all()
        r, _ = eb.worst(_maha_emulate(feats, means, prec), ref, bud)
        assert r <= 1.0, (where, r)


@pytest.mark.parametrize("mutation,factor", [("fp32", 1e3), ("symmetric", 1e3), ("drop_last", 1e6), ("max", 1e6)])
def test_maha_mutations_break_the_budget(mutation, factor):
    """Features within 1e-2 of a class mean (row 0 at the LAST of 17 classes, a count that is no multiple of the kernel's 16
    waves), P with an asymmetric perturbation: each mistake misses the budget by at least `factor`."""
    feats, means, prec = eb.maha_case(64, 17, 9, "near", "asym")
    ref, bud = eb.maha_budget(feats, means, prec)
    assert eb.worst(_maha_emulate(feats, means, prec), ref, bud)[0] <= 1.0
    r, _ = eb.worst(_maha_emulate(feats, means, prec, mutation), ref, bud)
    print(f"MUTATION maha {mutation}: ratio {r:.3g}")
    assert r > factor, (mutation, r)


# ---- split forms -------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """a @ b.T in torch's fp32 (an MFMA pass: exact products, fp32 accumulation)."""
    return (torch.from_numpy(np.ascontiguousarray(a, F32)) @ torch.from_numpy(np.ascontiguousarray(b, F32)).T).numpy()


def _chain(parts_x, parts_w, order):
    """The kernels' fp32 accumulator chain over split operands: per logical K-step of 64 columns the passes `order`
    ((x part, w part) pairs), each pass's 64 exact products added one after another."""
    M, K = parts_x[0].shape
    acc = np.zeros((M, parts_w[0].shape[0]), F32)
    for t in range(K // 64):
        for xi, wi in order:
            xa, wa = parts_x[xi], parts_w[wi]
            for k in range(t * 64, t * 64 + 64):
                acc = acc + _f32(xa[:, k:k + 1].astype(np.float64) * wa[None, :, k])
    return acc


@pytest.mark.parametrize("K,passes", [(4096, 2), (3072, 4)])
def test_c_acc_covers_split_chains(K, passes):
    """C_ACC on the chains the split forms run: 2 x 4096 products (L/14 fc2, split activations) and 4 x 3072 (B/16 fc2,
    split weights and split activations), N(0, 1) activations split into fp16 pairs: the kernel-order chain and torch's CPU
    matmul of the concatenated passes stay within C_ACC / 2 of u32 * sum |x||w| over the merged operands."""
    rng = np.random.default_rng(K + passes)
    x = rng.standard_normal((96, K)).astype(F32)
    w = (rng.standard_normal((96, K)) * K ** -0.5).astype(F32)
    xh, xl = (a.astype(F32) for a in eb.split2_f16(x))
    if passes == 4:
        wp = tuple(a.astype(F32) for a in eb.split2_f16(w))
        order = [(0, 0), (1, 0), (0, 1), (1, 1)]
    else:
        wp = (w.astype(np.float16).astype(F32),)
        order = [(0, 0), (1, 0)]
    xm = xh.astype(np.float64) + xl
    wm = sum(a.astype(np.float64) for a in wp)
    ref, s = eb.gemm_reference(xm, wm, np.zeros(96))
    seq = _chain((xh, xl), wp, order)
    cat_x = np.concatenate([(xh, xl)[i] for i, _ in order], axis=1)
    cat_w = np.concatenate([wp[j] for _, j in order], axis=1)
    for name, got in (("kernel order", seq), ("torch", _mm(cat_x, cat_w))):
        r = float((np.abs(got - ref) / (eb.U32 * s)).max())
        print(f"C_ACC split chain {passes} x {K} ({name}): {r:.3g} of u32 sum|x||w|")
        assert r <= eb.C_ACC / 2, (name, K, passes, r)


SMALL_EXP = list(range(-12, -3))   # row magnitudes 2^-12 ... 2^-4: lo on fp16's subnormal grid, its floor dominates


def _split_case(M, N, K, flags, mode, seed):
    """Operands of one split GEMM: (x32, xp, w32, wp, bias, resid0).  x32: fp32 rows, even rows of magnitude 1, odd rows
    2^-12 ... 2^-4 in turn.  xp: (X_hi, X_lo) under "X" (split2), else (x,) in the mode's format.  wp: (W_hi, W_lo) of an
    fp32-valued weight under "W" (cvt_weight_split: RNE in the mode's format), else (w,) an exact fp16 weight."""
    rng = np.random.default_rng(seed)
    sc = np.ones(M)
    sc[1::2] = [2.0 ** SMALL_EXP[i % len(SMALL_EXP)] for i in range(len(sc[1::2]))]
    x32 = _f32(rng.standard_normal((M, K)) * sc[:, None])
    w32 = _f32(rng.standard_normal((N, K)) * K ** -0.5)
    if "X" in flags:
        xp = tuple(a.astype(F32) for a in eb.split2_f16(x32))
    else:
        x32 = eb.round_to(x32, mode)
        xp = (x32,)
    if "W" in flags:
        hi = eb.round_to(w32, mode)
        wp = (hi, eb.round_to(_f32(w32 - hi), mode))
    else:
        w32 = eb.round_to(w32, mode)
        wp = (w32,)
    return x32, xp, w32, wp, _f32(0.1 * rng.standard_normal(N)), _f32(rng.standard_normal((M, N)))


def _split_gemm_emulate(xp, wp, bias, resid0, epi, out, mutation=None):
    """The split GEMM as the kernels run it: per logical K-step t the passes kt = 0 .. 2^(xsplit + ksplit) - 1, X part
    kt & xsplit, W part (kt >> xsplit) & ksplit (gemm.hip kstep_off), in one fp32 chain; then the epilogue.  out: "fp16" /
    "bf16" (a plain 16-bit store; EPI_GELU: quick_gelu_fast), "split" (EPI_*_X2: the exact QuickGELU, then split2), "fp32"
    (the residual).  Mutations: "drop_lo_first" / "drop_lo_last" (the lo pass of the first / last logical K-step skipped:
    X_lo, or W_lo without split activations), "kstep_off" (X_lo of step t meets W of step t + 1), "flush_operand" (the MFMA
    flushes fp16-subnormal inputs to zero), "drop_w_lo" (no W_lo pass), "flush_output" (split2 under an f16 denormal flush:
    a subnormal lo stored as 0), "drop_out_lo" (hi only), "gelu_fast" (EPI_GELU_X2 with quick_gelu_fast)."""
    xs, ks = len(xp) - 1, len(wp) - 1
    if mutation == "flush_operand":
        xp = tuple(np.where(np.abs(a) < 2.0 ** -14, 0, a).astype(F32) for a in xp)
        wp = tuple(np.where(np.abs(a) < 2.0 ** -14, 0, a).astype(F32) for a in wp)
    M, K = xp[0].shape
    T = K // 64
    acc = np.zeros((M, wp[0].shape[0]), F32)
    for t in range(T):
        for kt in range(1 << (xs + ks)):
            xi, wi = kt & xs, (kt >> xs) & ks
            lo_pass = xi == 1 if xs else wi == 1
            if lo_pass and ((mutation == "drop_lo_first" and t == 0) or (mutation == "drop_lo_last" and t == T - 1)):
                continue
            if mutation == "drop_w_lo" and wi == 1:
                continue
            tw = (t + 1) % T if (mutation == "kstep_off" and xi == 1) else t
            xa, wa = xp[xi], wp[wi]
            for j in range(64):
                acc = acc + _f32(xa[:, t * 64 + j:t * 64 + j + 1].astype(np.float64) * wa[None, :, tw * 64 + j])
    v = _f32(acc + bias[None, :])
    if epi == 2:
        return _f32(resid0 + v)
    if epi == 1:
        if out == "split" and mutation != "gelu_fast":
            v = _f32(v / (1.0 + np.exp(-1.702 * v.astype(np.float64))))
        else:
            v = _quick_gelu_fast(v)
    if out != "split":
        return eb.round_to(v, out)
    hi, lo = eb.split2_f16(v)
    lo = lo.astype(np.float64)
    if mutation == "drop_out_lo":
        lo = np.zeros_like(lo)
    if mutation == "flush_output":
        lo = np.where(np.abs(lo) < 2.0 ** -14, 0.0, lo)
    return hi.astype(np.float64) + lo


def _split_out(flags, mode, epi):
    return "fp32" if epi == 2 else "split" if "O" in flags else mode


def _split_ref_budget(xp, wp, bias, resid0, epi, out):
    xm = sum(a.astype(np.float64) for a in xp)
    wm = sum(a.astype(np.float64) for a in wp)
    lin, s = eb.gemm_reference(xm, wm, bias)
    if out in ("split", "fp32"):
        return eb.gemm_split_budget(lin, s, epi, out == "split", resid0)
    return eb.gemm_budget(lin, s, out, epi)


SPLIT_SHAPES = [(34, 48, 64), (18, 32, 192), (12, 16, 640), (6, 16, 3072)]
# (flags, mode, epilogues): X = split activations, O = split output, W = split weights (mcm_op_linear_ex flags)
SPLIT_FORMS = [("X", "fp16", (0, 1, 2)), ("XO", "fp16", (0, 1)), ("WX", "fp16", (0, 1, 2)), ("WXO", "fp16", (0, 1)),
               ("W", "fp16", (0, 1, 2)), ("W", "bf16", (0, 1, 2))]


def _split_ratio(flags, mode, epi, mutation=None, shapes=SPLIT_SHAPES, unsplit=False):
    worst = 0.0
    for M, N, K in shapes:
        x32, xp, w32, wp, bias, resid0 = _split_case(M, N, K, flags, mode, seed=M * N + K + epi)
        out = _split_out(flags, mode, epi)
        got = _split_gemm_emulate(xp, wp, bias, resid0, epi, out, mutation)
        if unsplit:
            ref, bud = eb.gemm_unsplit_budget(x32, w32, bias, epi, out == "split", resid0, True, "W" in flags)
        else:
            ref, bud = _split_ref_budget(xp, wp, bias, resid0, epi, out)
        worst = max(worst, eb.worst(got, ref, bud)[0])
    return worst


@pytest.mark.parametrize("flags,mode,epis", SPLIT_FORMS, ids=[f"{f}-{m}" for f, m, _ in SPLIT_FORMS])
def test_split_gemm_emulation_within_budget(flags, mode, epis):
    """Every flag combination and epilogue in the kernel's pass order, at one K-step up to 3072 (a chain of 4 x 3072 under
    WX), rows of magnitude 2^-12 ... 2^-4 included; with split activations also against the unsplit fp32 operands."""
    for epi in epis:
        r = _split_ratio(flags, mode, epi)
        ru = _split_ratio(flags, mode, epi, unsplit=True) if "X" in flags else 0.0
        print(f"split gemm {flags} {mode} epi{epi}: correct {r:.3g} (unsplit operands {ru:.3g})")
        assert r <= 1.0 and ru <= 1.0, (flags, mode, epi, r, ru)


@pytest.mark.parametrize("mutation,cases", [
    ("drop_lo_first", [("X", "fp16", 2), ("XO", "fp16", 0), ("WX", "fp16", 2), ("W", "fp16", 2), ("W", "bf16", 2)]),
    ("drop_lo_last", [("X", "fp16", 2), ("XO", "fp16", 0), ("WX", "fp16", 2), ("W", "fp16", 2), ("W", "bf16", 2)]),
    ("kstep_off", [("X", "fp16", 2), ("XO", "fp16", 0), ("WXO", "fp16", 1)]),
    ("flush_operand", [("X", "fp16", 2), ("XO", "fp16", 0)]),
    ("flush_output", [("XO", "fp16", 0), ("XO", "fp16", 1), ("WXO", "fp16", 0)]),
    ("drop_out_lo", [("XO", "fp16", 0), ("XO", "fp16", 1), ("WXO", "fp16", 0)]),
    ("drop_w_lo", [("W", "fp16", 2), ("W", "bf16", 2), ("WX", "fp16", 2)]),
])
def test_split_gemm_mutations_break_the_budget(mutation, cases):
    for flags, mode, epi in cases:
        r = _split_ratio(flags, mode, epi, mutation)
        print(f"split gemm {mutation} {flags} {mode} epi{epi}: worst budget ratio {r:.3g}")
        assert r > 1.0, (mutation, flags, mode, epi, r)


def test_gelu_fast_in_the_split_epilogue_stays_inside_the_budget():
    """EPI_GELU_X2 computed with quick_gelu_fast instead of the exact form is the one listed mistake the split budget
    cannot see: the two forms differ by a couple of fp32 ulps of the result, while every GEMM output carries the
    accumulation term C_ACC u32 sum|x||w| >= 16 u32 |lin| (and gemm_budget's C_GELU ulps), for every input within the
    op's contract.  Pinned here so that the claim stays true; the GPU tests cannot tell the two forms apart either."""
    for flags in ("XO", "WXO"):
        r = _split_ratio(flags, "fp16", 1, "gelu_fast")
        print(f"split gemm gelu_fast {flags}: worst budget ratio {r:.3g} (not detectable)")
        assert r <= 1.0


@pytest.mark.parametrize("D", [128, 768, 1024])
def test_layernorm_split_emulation_within_budget_and_lo_mistakes_break_it(D):
    """ln_row_store<X2>: the fp32 LayerNorm value split (split2).  The hostile rows of the 16-bit test, and every 7th channel
    with gamma ~ 2^-8 (outputs with a subnormal lo).  A dropped lo and a flushed subnormal lo break the budget."""
    x, g, b = _ln_rows(D, D)
    g = g.copy()
    g[::7] *= F32(2.0 ** -8)
    ref, bud = eb.layernorm_split_budget(x, g, b)
    v = _ln_emulate(x, g, b, "fp32")
    hi, lo = (a.astype(np.float64) for a in eb.split2_f16(v))
    r, _ = eb.worst(hi + lo, ref, bud)
    r_drop, _ = eb.worst(hi, ref, bud)
    r_flush, _ = eb.worst(hi + np.where(np.abs(lo) < 2.0 ** -14, 0.0, lo), ref, bud)
    print(f"layernorm split D={D}: correct {r:.3g}, lo dropped {r_drop:.3g}, subnormal lo flushed {r_flush:.3g}")
    assert r <= 1.0 < min(r_drop, r_flush)


def _attn_split_emulate(parts, mutation=None, stream=False):
    """attn_tr_kernel<X2> (stream=False) or attn_long_kernel<X2> (stream: 64-key tiles, running max, O and the row sum
    rescaled) on one (sequence, head), parts = (qh, ql, kh, kl, vh, vl): S = K_lo Q_hi + K_hi Q_lo + K_hi Q_hi (fp32),
    P = exp2(s SC - m SC + 12) split (split2), per 32-key step the row sum over P_lo then P_hi and O += V_lo P_hi + V_hi P_lo +
    V_hi P_hi, then O / rowsum split.  Mutations: "drop_kq_lo" (no K_hi Q_lo), "drop_vp_lo" (no V_hi P_lo), "p_unscaled"
    (P split without the 2^12 scale), "drop_out_lo", "flush_output"."""
    qh, ql, kh, kl, vh, vl = (_f32(a) for a in parts)
    L = qh.shape[0]
    SC = F32(0.125 * 1.4426950408889634)
    off = F32(0.0 if mutation == "p_unscaled" else 12.0)
    s = _mm(qh, kl)
    if mutation != "drop_kq_lo":
        s = _f32(s + _mm(ql, kh))
    s = _f32(s + _mm(qh, kh))
    kt = 64 if stream else L
    o = np.zeros((L, 64), F32)
    lsum = np.zeros((L, 1), F32)
    m = np.full((L, 1), -np.inf, F32)
    for k0 in range(0, L, kt):
        st = s[:, k0:k0 + kt]
        mn = np.maximum(m, st.max(axis=1, keepdims=True))
        with np.errstate(invalid="ignore"):
            a = _f32(np.exp2(_f32(_f32(m - mn) * SC).astype(np.float64)))
        a = np.where(np.isfinite(m), a, F32(0)).astype(F32)
        o, lsum, m = _f32(o * a), _f32(lsum * a), mn
        msc = _f32(_f32(mn * SC) - off)
        e = _f32(np.exp2(_f32(st.astype(np.float64) * SC - msc).astype(np.float64)))
        ph, pl = (x.astype(F32) for x in eb.split2_f16(e))
        for u in range(0, st.shape[1], 32):
            ks = slice(u, u + 32)
            vs = slice(k0 + u, k0 + u + 32)
            lsum = _f32(lsum + pl[:, ks].sum(axis=1, keepdims=True, dtype=F32))
            lsum = _f32(lsum + ph[:, ks].sum(axis=1, keepdims=True, dtype=F32))
            o = _f32(o + _mm(ph[:, ks], vl[vs].T))
            if mutation != "drop_vp_lo":
                o = _f32(o + _mm(pl[:, ks], vh[vs].T))
            o = _f32(o + _mm(ph[:, ks], vh[vs].T))
    res = _f32(o * _f32(F32(1) / lsum))
    hi, lo = (x.astype(np.float64) for x in eb.split2_f16(res))
    if mutation == "drop_out_lo":
        lo = np.zeros_like(lo)
    if mutation == "flush_output":
        lo = np.where(np.abs(lo) < 2.0 ** -14, 0.0, lo)
    return hi + lo


def _attn_split_case(L, seed, kind=None):
    """One head's (qh, ql, kh, kl, vh, vl) from a split image: N(0, 1) q / k (x 1.5) / v; "spiked": one query and one key
    scaled up (a near one-hot softmax); "small_v": V scaled by 2^-8 (outputs with a subnormal lo); "coherent": the input of
    error_budget.coherent_small_p_qkv."""
    if kind == "coherent":
        return eb.head_parts(eb.split_image(eb.coherent_small_p_qkv(L, 1)), L, 1, 0, 0)
    rng = np.random.default_rng(seed)
    qkv = rng.standard_normal((L, 192)).astype(F32)
    qkv[:, :128] *= 1.5
    if kind == "spiked":
        qkv[min(7, L - 1), :64] *= 20.0
        qkv[L // 2, 64:128] *= 10.0
    if kind == "small_v":
        qkv[:, 128:] *= F32(2.0 ** -8)
    return eb.head_parts(eb.split_image(qkv), L, 1, 0, 0)


def _attn_split_ratio(L, kind, mutation=None):
    from tests import online_softmax_budget as ob

    parts = _attn_split_case(L, L + 11, kind)
    stream = L > 288
    ref, bud = (ob.online_attention_split_budget if stream else eb.attention_split_budget)(*parts)
    return eb.worst(_attn_split_emulate(parts, mutation, stream), ref, bud)[0]


ATTN_SPLIT_CASES = [(1, None), (17, None), (50, None), (197, None), (197, "spiked"), (288, "small_v"), (288, "coherent"),
                    (289, None), (577, "spiked"), (577, "small_v"), (1024, "coherent")]


def test_attention_split_emulation_within_budget():
    """Both split attention forms (L <= 288: whole row; L > 288: streamed) within their budgets, the coherent small-P input
    included (there the 2^12 scale keeps the subnormal floor of P's lo at 2^-37)."""
    for L, kind in ATTN_SPLIT_CASES:
        r = _attn_split_ratio(L, kind)
        print(f"attention split L={L} {kind}: correct {r:.3g}")
        assert r <= 1.0, (L, kind, r)


@pytest.mark.parametrize("mutation,cases", [
    ("drop_kq_lo", [(197, None), (577, None)]),
    ("drop_vp_lo", [(197, None), (577, None)]),
    ("drop_out_lo", [(197, None), (577, None)]),
    ("flush_output", [(288, "small_v"), (577, "small_v")]),
    ("p_unscaled", [(288, "coherent"), (1024, "coherent")]),
])
def test_attention_split_mutations_break_the_budget(mutation, cases):
    """K_hi Q_lo or V_hi P_lo dropped, the output's lo dropped or flushed, and P split without the 2^12 scale (on the
    coherent small-P input: many equal P whose lo halves all miss by nearly 2^-25), in the whole-row and the streamed form."""
    for L, kind in cases:
        r = _attn_split_ratio(L, kind, mutation)
        print(f"attention split {mutation} L={L} {kind}: worst budget ratio {r:.3g}")
        assert r > 1.0, (mutation, L, kind, r)


def test_split_helpers():
    """split2_f16 is RNE with fp16 subnormals and FP16_OVFL saturation; the image helpers round-trip; split_repr bounds the
    pair at every magnitude it claims to, the subnormal floor and the range edge included."""
    assert eb.f16_sat(np.float32(1e5)) == np.float16(65504) and eb.f16_sat(np.float32(-7e4)) == np.float16(-65504)
    assert eb.f16_sat(np.float32(65519)) == np.float16(65504) and eb.f16_sat(np.float32(3.0 * 2 ** -26)) == np.float16(2 ** -24)
    hi, lo = eb.split2_f16(np.float32([1e5, 131008.0, 2e5, 65519.0]))
    assert list(hi) == [65504] * 4 and list(lo.astype(np.float64)) == [34496.0, 65504.0, 65504.0, 15.0]
    rng = np.random.default_rng(1)
    v = (rng.standard_normal((64, 128)) * 2.0 ** rng.integers(-20, 17, (64, 1))).astype(F32)
    back = eb.merge_image(eb.split_image(v))
    assert (np.abs(back - v) <= eb.split_repr(np.abs(v))).all()
    inside = np.abs(v) < eb.FP16_MAX
    assert (np.abs(back - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25))[inside].all()
    assert np.isinf(eb.split_repr(2e5)) and eb.split_repr(131008.0) == 16.0 and eb.split_repr(2.0 ** -10) == 2.0 ** -25


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


# ---- the two ends of the towers (test_gpu_tower_ends_budget.py) ----------------------------------------------------------
# Emulations of the EPI_PATCH GEMM behind each operand gather, of layernorm_pre_kernel, pool_project_kernel and
# bank_reduce_kernel in fp32 and in kernel order, on the GPU tests' own input generators: inside their budgets; each planted
# mistake outside.
from tests import test_gpu_tower_ends_budget as ends  # noqa: E402  (its generators; nothing in it touches a GPU on import)


def _butterfly(v):
    """wave_sum over the last axis (64 lanes): v += shfl_xor(v, 32), 16, ... 1; every lane ends with the total."""
    for o in (32, 16, 8, 4, 2, 1):
        v = _f32(v + v[..., np.arange(64) ^ o])
    return v


def _seq_sum(parts):
    """tot = 0; for i: tot += parts[..., i] in fp32."""
    tot = np.zeros(parts.shape[:-1], F32)
    for i in range(parts.shape[-1]):
        tot = _f32(tot + parts[..., i])
    return tot


def _smooth_pos(ntok, D, seed):
    """A position table whose neighbouring rows differ by about 1e-3 relative."""
    base = (0.1 * np.random.default_rng(seed).standard_normal(D)).astype(F32)
    base = np.where(np.abs(base) < 0.02, F32(0.05), base)
    return _f32(base[None, :] * (1 + 1e-3 * np.arange(ntok))[:, None])


def _patch_case(mode, x2, split, seed, u8=False):
    """Two images of 2 x 2 patches of 14 pixels: L/14's K = 588 padded to 640 (16-bit modes) / 608 (fp32)."""
    rng = np.random.default_rng(seed)
    B, S, P, D = 2, 28, 14, 48
    kreal = 3 * P * P
    kalign = 32 if mode == "fp32" else 64
    kpad = (kreal + kalign - 1) // kalign * kalign
    if u8:
        px = eb.u8_normalise(ends._u8(B, S, seed))
    else:
        px = ends._pixels(B, S, seed, device="cpu").numpy()
    w = np.zeros((D, kpad), F32)
    w[:, :kreal] = rng.standard_normal((D, kreal)) * kreal ** -0.5
    if not split:
        w = _f32(eb.weight_values(w, mode, False))
    return px, w, _smooth_pos(5, D, seed), P, kpad


def _patch_emulate(px, w, pos, P, kpad, mode, x2, split, mutation=None):
    """patchify (operand rounding, zero pad) then the fp32 MFMA chain K-step after K-step (a split operand: one more stretch
    of the same chain per half) and the epilogue's float32(acc + pos[1 + p])."""
    pm = eb.patchify_reference(px, P, kpad)
    n_patches = (px.shape[2] // P) ** 2
    if mutation == "pad":       # the pad columns left as a poisoned workspace holds them
        pm[:, 3 * P * P:] = np.nan
    kstep = 32 if mode == "fp32" else 64
    if x2:
        hi, lo = eb.split2_f16(pm)
        xs = [hi.astype(F32), lo.astype(F32)]
    elif mode == "fp32":
        xs = [pm]
    elif mutation == "trunc":
        xs = [_trunc16(pm, mode)]
    else:
        xs = [_f32(eb.operand_values(pm, mode))]
    if split:
        if mode == "fp16":
            wh, wl = (a.astype(F32) for a in eb.split2_f16(w))
        else:
            wh = eb.round_to(w, mode)
            wl = eb.round_to(w - wh, mode)
        ws = [wh, wl]
    else:
        ws = [w]
    xcat = np.concatenate([x for _ in ws for x in xs], axis=1)
    wcat = np.concatenate([wv for wv in ws for _ in xs], axis=1)
    with np.errstate(invalid="ignore"):
        acc = _dot_seq(xcat, wcat, kstep)
        rows = np.arange(pm.shape[0])
        prow = rows % n_patches + (0 if mutation == "pos" else 1)
        return _f32(acc + pos[prow])


PATCH_FORMS = [("bf16", False, False), ("bf16", False, True), ("fp16", False, False), ("fp16", False, True),
               ("fp16", True, False), ("fp16", True, True), ("fp32", False, False)]


def _patch_ratio(mode, x2, split, mutation=None, u8=False, seed=3):
    px, w, pos, P, kpad = _patch_case(mode, x2, split, seed, u8)
    got = _patch_emulate(px, w, pos, P, kpad, mode, x2, split, mutation)
    pm = eb.patchify_reference(px, P, kpad)
    ref, bud = eb.patch_embed_budget(eb.operand_values(pm, mode, x2), eb.weight_values(w, mode, split), pos, 4)
    assert np.isfinite(bud).all()
    return eb.worst(got, ref, bud)[0]


@pytest.mark.parametrize("mode,x2,split", PATCH_FORMS)
def test_patch_embedding_emulation_within_budget(mode, x2, split):
    for u8 in (False, True):
        r = _patch_ratio(mode, x2, split, u8=u8)
        assert r <= 1.0, (mode, x2, split, u8, r)


@pytest.mark.parametrize("mutation", ["pos", "trunc", "pad"])
def test_patch_embedding_mutations_break_the_budget(mutation):
    """The position row p instead of 1 + p on a smooth table; pixels truncated instead of rounded to nearest even (the
    16-bit single-operand modes: fp32 and the split gather have no rounding to get wrong); pad columns left as the poisoned
    workspace holds them (NaN x 0).  A FINITE value in a pad column changes no output (the weight's pad columns are zero): that
    is not a mistake an output can show, which is what the poison flag of mcm_debug_vision_front is for."""
    forms = [f for f in PATCH_FORMS if mutation != "trunc" or (f[0] != "fp32" and not f[1])]
    for mode, x2, split in forms:
        r = _patch_ratio(mode, x2, split, mutation)
        print(f"patch {mutation} {mode} x2={x2} wsplit={split}: budget ratio {r:.3g}")
        assert r > 1.0, (mutation, mode, x2, split, r)


def test_uint8_normalise_written_as_one_multiply_is_not_bit_equal():
    """u8 * (1 / (255 std)) - mean / std in fp32 instead of ((u8 / 255) - mean) / std: an fp32 ulp or two away on most of the
    768 (value, channel) pairs.  No budget of the patch GEMM can show an operand that is off by an fp32 ulp (its accumulation
    term is 16 of them); the GPU test's bit-equality with eb.u8_normalise does."""
    u8 = np.arange(256, dtype=np.uint8)[None, :, None, None] * np.ones((1, 1, 1, 3), np.uint8)
    want = eb.u8_normalise(u8)
    scale, shift = _f32(F32(1) / _f32(F32(255) * eb.CLIP_STD)), _f32(eb.CLIP_MEAN / eb.CLIP_STD)
    got = _f32(_f32(u8.astype(F32) * scale) - shift).transpose(0, 3, 1, 2)
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"uint8 normalise as one multiply: {differ} of 768 pairs differ")
    assert differ > 100
    fused = _f32(u8.astype(np.float64) * scale - shift).transpose(0, 3, 1, 2)    # ... or contracted to one fma
    assert int((fused.view(np.uint32) != want.view(np.uint32)).sum()) > 100


@pytest.mark.parametrize("mode,x2", [("bf16", False), ("fp16", False), ("fp16", True), ("fp32", False)])
def test_fused_pre_layernorm_emulation_within_budget_and_wrong_cls_row_breaks_it(mode, x2):
    """layernorm_pre_kernel: the CLS row float32(cls + pos[0]), ln_row_apply twice.  Planted: the CLS row built from pos[1]
    (smooth table), and layer_norm1 applied to the kernel's INPUT instead of to the rows it wrote back."""
    D, B, ntok = 128, 3, 5
    rng = np.random.default_rng(D)
    pos = _smooth_pos(ntok, D, 1)
    cls = (0.5 * rng.standard_normal(D)).astype(F32)
    g0, b0 = (1 + 0.1 * rng.standard_normal(D)).astype(F32), (0.05 * rng.standard_normal(D)).astype(F32)
    g1, b1 = (1 + 0.1 * rng.standard_normal(D)).astype(F32), (0.05 * rng.standard_normal(D)).astype(F32)
    x = (rng.standard_normal((B * ntok, D)) * 0.8).astype(F32)
    x[::ntok] = np.nan                                   # what the CLS slots hold does not matter

    def run(cls_pos_row=0, ln1_of_input=False):
        x0 = x.copy()
        x0[::ntok] = _f32(cls + pos[cls_pos_row])
        x1 = _ln_emulate(x0, g0, b0, "fp32")
        y = _ln_emulate(x0 if ln1_of_input else x1, g1, b1, "fp32")
        if x2:
            return x1, eb.merge_image(eb.split_image(y))
        return x1, y if mode == "fp32" else _f32(eb.operand_values(y, mode))

    x0 = x.copy()
    x0[::ntok] = eb.cls_row(cls, pos)
    x1, y = run()
    (r0, bud0), (r1, bud1) = eb.pre_ln_budgets(x0, x1, g0, b0, g1, b1, mode, x2)
    assert np.isfinite(bud0).all() and np.isfinite(bud1).all()
    assert eb.worst(x1, r0, bud0)[0] <= 1.0 and eb.worst(y, r1, bud1)[0] <= 1.0
    x1b, _ = run(cls_pos_row=1)
    r_cls = eb.worst(x1b, r0, bud0)[0]
    _, yb = run(ln1_of_input=True)
    r_in = eb.worst(yb, r1, bud1)[0]
    print(f"pre-ln {mode} x2={x2}: CLS from pos[1] {r_cls:.3g}, layer_norm1 of the input {r_in:.3g}")
    assert r_cls > 1.0 and r_in > 1.0


def _pool_emulate(x, g, b, proj, normalize, mutation=None, eps=1e-5):
    """pool_project_kernel in fp32 and in its order: thread t holds x[t]; wave_sum, 16 partials added in turn; centred
    squares the same way; y = c * rstd * g + b; per output p the lanes' fmaf chains over d = lane * 4 + 256 i + j and the
    butterfly; lane 0 of wave p % 16 adds the squares of its outputs in turn, 16 partials, 1 / sqrtf, product."""
    n, D = x.shape
    P = proj.shape[0]
    eps = F32(eps)
    wide = D > 1024       # pool_project_kernel<WIDE>: thread t holds x[t] and x[t + 1024]
    W = 2048 if wide else 1024
    xp = np.zeros((n, W), F32)
    xp[:, :D] = x

    def block_total(v):   # [n, 1024] -> [n]
        return _seq_sum(_butterfly(v.reshape(n, 16, 64))[:, :, 0])

    def thread_sum(v):    # what a thread hands to wave_sum: its element, or (WIDE) xv + xw
        return _f32(v[:, :1024] + v[:, 1024:]) if wide else v

    def thread_sq(v):     # c * c, or (WIDE) fmaf(cw, cw, c * c)
        sq = _f32(v[:, :1024] * v[:, :1024])
        return _f32(v[:, 1024:].astype(np.float64) ** 2 + sq) if wide else sq

    mean = _f32(block_total(thread_sum(xp)) / F32(D))[:, None]
    c = np.where(np.arange(W) < D, _f32(xp - mean), F32(0))
    if mutation == "single_pass":
        var = _f32(_f32(block_total(thread_sq(xp)) / F32(D)) - _f32(mean[:, 0] * mean[:, 0]))
    else:
        var = _f32(block_total(thread_sq(c)) / F32(D))
    with np.errstate(invalid="ignore", divide="ignore"):
        if mutation == "eps_outside":
            rstd = _f32(F32(1) / _f32(np.sqrt(var) + eps))
        else:
            rstd = _f32(F32(1) / np.sqrt(_f32(var + eps)))
        y = _f32(_f32(_f32(c[:, :D] * rstd[:, None]) * g) + b)
    if mutation == "y_bf16":
        y = eb.round_to(y, "bf16")
    a = np.zeros((n, P, 64), F32)
    lane = np.arange(64)
    for i in range((D + 255) // 256):
        for j in range(4):
            d = lane * 4 + 256 * i + j
            ok = lane * 4 + 256 * i < D
            dd = np.where(ok, d, 0)
            term = proj[:, dd].astype(np.float64)[None, :, :] * y[:, dd].astype(np.float64)[:, None, :]
            a = np.where(ok, _f32(term + a), a)
    o = _butterfly(a)[:, :, 0]                                         # [n, P]
    if not normalize:
        return o
    osq = eb.round_to(o, "fp16") if mutation == "norm_fp16" else o
    sq = np.zeros((n, 16), F32)
    for p in range(P):
        sq[:, p % 16] = _f32(sq[:, p % 16] + _f32(osq[:, p] * osq[:, p]))
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = _f32(F32(1) / np.sqrt(_seq_sum(sq)))
        return _f32(o * rn[:, None])


POOL_CASES = [(64, 1), (320, 17), (512, 64), (768, 512), (1020, 768), (1024, 1024)]
# widths and proj_dims inside mcm_create's envelope and off the checkpoints': 64 x an odd number, whole 256-column rounds of
# the projection plus a partial one, two elements per thread with the second round partial (1088, 1216); P below the 16 waves
# of the workgroup, and no multiple of 16
POOL_CASES += [(192, 4), (192, 260), (320, 100), (320, 1020), (832, 260), (832, 4), (1088, 1020), (1088, 4), (1216, 100),
               (1216, 260)]


@pytest.mark.parametrize("D,P", POOL_CASES)
def test_pool_project_emulation_within_budget(D, P):
    x = ends._pool_rows(25, D, D)
    g, b, proj = ends._pool_params(D, P, D + P)
    for normalize in (False, True):
        ref, bud = eb.pool_project_budget(x, g, b, proj, normalize)
        assert np.isfinite(bud).all()
        r = eb.worst(_pool_emulate(x, g, b, proj, normalize), ref, bud)[0]
        print(f"pool D={D} P={P} normalize={normalize}: {r:.3g}")
        assert r <= 1.0, (D, P, normalize, r)


@pytest.mark.parametrize("mutation", ["single_pass", "eps_outside", "y_bf16", "norm_fp16"])
def test_pool_project_mutations_break_the_budget(mutation):
    """E[x^2] - mean^2 (shows on the rows of mean 1e3), eps added to the standard deviation instead of the variance, the
    projection fed a bf16-rounded y, the norm taken from fp16-rounded outputs."""
    for D, P in ((512, 64), (768, 512), (1024, 768), (1088, 260)):
        x = ends._pool_rows(25, D, D)
        g, b, proj = ends._pool_params(D, P, D + P)
        ref, bud = eb.pool_project_budget(x, g, b, proj, True)
        with np.errstate(invalid="ignore"):
            r = eb.worst(_pool_emulate(x, g, b, proj, True, mutation), ref, bud)[0]
        print(f"pool {mutation} D={D} P={P}: budget ratio {r:.3g}")
        assert r > 1.0, (mutation, D, P, r)


def test_pool_project_zero_norm_has_no_finite_budget():
    """gamma = beta = 0: the output is 0 and its norm 0; the kernel returns 0 * inf, the reference x / x.norm() is 0 / 0: the
    one case excluded from the budgets (pinned on the GPU as well)."""
    x = ends._pool_rows(5, 512, 1)
    z = np.zeros(512, F32)
    proj = ends._pool_params(512, 64, 0)[2]
    assert (_pool_emulate(x, z, z, proj, False) == 0).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(_pool_emulate(x, z, z, proj, True)).all()
    assert np.isinf(eb.pool_project_budget(x, z, z, proj, True)[1]).all()


def test_eos_taken_as_the_last_argmax_breaks_the_pool_budget():
    """Prompts padded with the EOS id: the pooled row is the FIRST position of the largest id."""
    rng = np.random.default_rng(0)
    K, S, D, P = 4, 16, 128, 64
    ids = rng.integers(1, 1000, size=(K, S))
    for k in range(K):
        ids[k, 5 + k:] = 49407
    assert list(eb.eos_rows(ids)) == [k * S + 5 + k for k in range(K)]
    last = np.arange(K) * S + (S - 1 - ids[:, ::-1].argmax(axis=1))
    x = rng.standard_normal((K * S, D)).astype(F32)
    g, b, proj = ends._pool_params(D, P, 1)
    ref, bud = eb.pool_project_budget(x[eb.eos_rows(ids)], g, b, proj, True)
    assert eb.worst(_pool_emulate(x[eb.eos_rows(ids)], g, b, proj, True), ref, bud)[0] <= 1.0
    r = eb.worst(_pool_emulate(x[last], g, b, proj, True), ref, bud)[0]
    print(f"EOS as the last argmax: budget ratio {r:.3g}")
    assert r > 1.0


def _bank_emulate(f, K, T, acc16=False):
    P = f.shape[1]
    f = f.reshape(K, T, P)
    a = np.zeros((K, P), F32)
    for t in range(T):
        a = eb.round_to(a + f[:, t], "fp16") if acc16 else _f32(a + f[:, t])
    a = _f32(a / F32(T))
    lanes = np.zeros((K, 64), F32)
    for d in range(P):
        lanes[:, d % 64] = _f32(lanes[:, d % 64] + _f32(a[:, d] * a[:, d]))
    rn = _f32(F32(1) / np.sqrt(_butterfly(lanes)[:, 0]))
    return _f32(a * rn[:, None])


@pytest.mark.parametrize("P", [64, 512, 768])
def test_bank_reduce_emulation_within_budget_and_fp16_mean_breaks_it(P):
    for K, T in ((1, 1), (3, 7), (5, 80)):
        f = ends._bank_rows(K, T, P, K + T + P)
        ref, bud = eb.bank_reduce_budget(f, K, T)
        assert np.isfinite(bud).all()
        r = eb.worst(_bank_emulate(f, K, T), ref, bud)[0]
        assert r <= 1.0, (P, K, T, r)
        if T > 1:
            r_bad = eb.worst(_bank_emulate(f, K, T, acc16=True), ref, bud)[0]
            print(f"bank P={P} K={K} T={T}: correct {r:.3g}, mean accumulated in fp16 {r_bad:.3g}")
            assert r_bad > 1.0
