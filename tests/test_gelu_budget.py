"""The exact-GELU budget of tests/gelu_budget.py, proved on the CPU in the manner of tests/test_error_budget.py: a
kernel-order fp32 emulation of common.hpp's gelu_erf behind the emulated GEMM stays inside it in every output mode (bf16,
fp16, fp32, split fp16), the two plausible wrong activations (QuickGELU, the tanh form) break it in every mode with the
accumulation term included, and the naive fp32 0.5 x (1 + erf(x / sqrt 2)) stays inside it (the point of stating the
activation term relative to |x|).  The emulation takes its constants from common.hpp itself, so it cannot drift from the
kernel."""
import os
import re

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gelu_budget as gb
from tests import test_error_budget as teb

torch = pytest.importorskip("torch")

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["bf16", "fp16", "fp32", "split"]


def _consts():
    """The float literals of gelu_erf in common.hpp, in source order: p / sqrt 2, 1, -log2(e) / 2, the six coefficients of h
    (highest power first)."""
    src = open(os.path.join(ROOT, "mcm_amd", "csrc", "common.hpp")).read()
    body = re.search(r"float gelu_erf\(float x\) \{(.*?)\n\}", src, re.S).group(1)
    body = body[:body.index("h = (h * t) * e")]
    lits = [F32(v) for v in re.findall(r"(-?\d+\.\d+)f", body)]
    assert len(lits) == 9 and lits[1] == 1.0, lits
    return lits[0], lits[2], lits[3:]


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _gelu_erf_f32(v, nudge=None):
    """common.hpp gelu_erf operation by operation in fp32.  nudge: a Generator; v_rcp_f32 and v_exp_f32 are then moved one
    ulp up or down at random from the correctly rounded value (the hardware's are accurate to 1 ulp, not correctly rounded)."""
    ps, k, c = _consts()
    v = np.asarray(v, F32)
    ax = np.abs(v)
    t = (1.0 / _fma(ax, ps, F32(1.0)).astype(np.float64)).astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        arg = ((ax * ax).astype(F32) * k).astype(F32)
        e = np.exp2(arg.astype(np.float64)).astype(F32)
    if nudge is not None:
        t = np.nextafter(t, np.where(nudge.random(t.shape) < 0.5, F32(0), F32(2)).astype(F32))
        e = np.nextafter(e, np.where(nudge.random(e.shape) < 0.5, F32(0), F32(2)).astype(F32))
    h = np.full_like(t, c[0])
    for ck in c[1:]:
        h = _fma(h, t, ck)
    h = ((h * t).astype(F32) * e).astype(F32)
    return (v * np.where(v >= 0, (F32(1.0) - h).astype(F32), h)).astype(F32)


def _erf_naive_f32(v):
    """0.5 x (1 + erf(x / sqrt 2)) with every operation in fp32 (torch's fp32 erf)."""
    t = torch.from_numpy(np.ascontiguousarray(v, F32))
    return (t * 0.5 * (1.0 + torch.erf(t * F32(0.7071067811865476)))).numpy()


def _quick_gelu_f32(v):
    return teb._f32(v / (1.0 + np.exp(-1.702 * v.astype(np.float64))))


ACTS = {"erf": _gelu_erf_f32, "naive": _erf_naive_f32, "quick": _quick_gelu_f32, "tanh": teb._tanh_gelu}


def _case(M, N, K, mode, seed):
    """Pre-activations over [-8, 8]: column n sits around bias[n] = -8 + 16 n / (N - 1) with a spread of 0.25, so every part
    of the axis is hit, the stretch [-4, -2.5] where the wrong activations differ most from GELU relative to the store's
    half-ulp included (N / 10 columns of it)."""
    rng = np.random.default_rng(seed)
    x = (0.25 * rng.standard_normal((M, K))).astype(F32)
    w = (rng.standard_normal((N, K)) * K ** -0.5).astype(F32)
    bias = np.linspace(-8.0, 8.0, N).astype(F32)
    op = "fp16" if mode == "split" else mode
    if op != "fp32":
        x, w = eb.round_to(x, op), eb.round_to(w, op)
    return x, w, bias


def _ratio(mode, act, M=24, N=320, K=128, seed=0, nudge=None, only=None):
    x, w, bias = _case(M, N, K, mode, seed)
    v = teb._f32(teb._dot_seq(x, w, 64 if mode != "fp32" else 32) + bias[None, :])
    y = ACTS[act](v) if nudge is None else _gelu_erf_f32(v, nudge)
    lin, s = eb.gemm_reference(x, w, bias)
    ref, bud = gb.gemm_gelu_budget(lin, s, "fp16" if mode == "split" else mode, out_split=mode == "split")
    if mode == "split":
        hi, lo = eb.split2_f16(y)
        got = hi.astype(np.float64) + lo.astype(np.float64)
    elif mode == "fp32":
        got = y
    else:
        got = eb.round_to(y, mode)
    if only is not None:
        keep = (lin >= only[0]) & (lin <= only[1])
        assert keep.sum() > 100
        return eb.worst(np.asarray(got, np.float64)[keep], ref[keep], bud[keep])[0]
    return eb.worst(got, ref, bud)[0]


def test_derivative_constant():
    x = np.linspace(-10, 10, 1_200_001)
    phi = np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)
    Phi = gb.gelu_erf64(x[x != 0]) / x[x != 0]
    d = np.abs(Phi + (x * phi)[x != 0])
    i = int(np.argmax(d))
    print(f"max |GELU'| = {d[i]:.5f} at x = {x[x != 0][i]:.4f}")
    assert 1.1288 < d[i] <= gb.GELU_ERF_DERIV and abs(x[x != 0][i] - np.sqrt(2)) < 1e-3


def test_fit_error_of_the_polynomial():
    """The approximation alone, in float64 with the fp32 constants of common.hpp: |t P(t) exp(-x^2 / 2) - erfc(|x| / sqrt 2) / 2|
    is 6.0e-9 = 0.10 u32 at worst (the fit in exact coefficients: 4.2e-9; the rest is their rounding to fp32).  The bar is a
    quarter of a unit roundoff, 1.5e-8: below it the approximation is invisible beside the >= 3 u32 of fp32 arithmetic, so
    all of gelu_erf's error is that arithmetic.  A coefficient wrong in its 7th digit fails this long before it shows in a
    budget."""
    ps, k, c = (np.float64(v) if np.isscalar(v) else [np.float64(u) for u in v] for v in _consts())
    ax = np.linspace(0.0, 16.0, 3_200_001)
    t = 1.0 / (1.0 + ps * ax)
    h = np.full_like(t, c[0])
    for ck in c[1:]:
        h = h * t + ck
    h = h * t * np.exp2(ax * ax * k)
    want = gb.gelu_erf64(-ax)
    want = np.where(ax > 0, -want / np.where(ax > 0, ax, 1.0), 0.5)   # Phi(-|x|) = 0.5 erfc(|x| / sqrt 2)
    err = np.abs(h - want)
    i = int(np.argmax(err))
    print(f"fit error of h: {err[i]:.3e} = {err[i] / eb.U32:.3f} u32 at |x| = {ax[i]:.4f}")
    assert err[i] <= 0.25 * eb.U32


def test_the_constant_is_one_the_reference_arithmetic_meets():
    """torch's fp32 gelu against the fp64 reference: below C_GELU_ERF u32 |x| (6.38 on the 5e7 points of the derivation; a
    4e6-point subset here), and NOT bounded relative to |ref| in the negative tail."""
    rng = np.random.default_rng(0)
    x = np.concatenate([np.linspace(-12, 12, 3_000_001), 2.0 * rng.standard_normal(1_000_000)]).astype(F32)
    x = x[x != 0]
    got = torch.nn.functional.gelu(torch.from_numpy(x)).numpy().astype(np.float64)
    ref = gb.gelu_erf64(x)
    r = np.abs(got - ref) / (eb.U32 * np.abs(x.astype(np.float64)))
    print(f"torch fp32 gelu: worst {r.max():.2f} u32 |x| at x = {x[int(np.argmax(r))]:.4f}")
    assert r.max() <= gb.C_GELU_ERF
    tail = (x < -11.5) & (ref != 0)
    assert (np.abs(got - ref)[tail] >= 0.5 * np.abs(ref[tail])).any()


def test_device_form_alone_meets_the_activation_term():
    """gelu_erf's emulation on a dense grid and on the awkward inputs, against act_budget; finite in, finite out."""
    rng = np.random.default_rng(1)
    x = np.concatenate([np.linspace(-12, 12, 2_000_001), 2.0 * rng.standard_normal(500_000),
                        [0.0, -0.0, 1e-45, -1e-45, 1e-30, -1e-30, -13.5, -20, -50, 50, 1e20, -1e20, 3.4e38, -3.4e38]]).astype(F32)
    ref = gb.gelu_erf64(x)
    for nudge in (None, rng):
        got = _gelu_erf_f32(x, nudge)
        assert np.isfinite(got).all()
        r, i = eb.worst(got, ref, gb.act_budget(x, ref))
        print(f"gelu_erf emulation{' (rcp / exp nudged 1 ulp)' if nudge else ''}: worst {r:.3f} of the budget at x = {x[i]!r}")
        assert r <= 1.0


@pytest.mark.parametrize("mode", MODES)
def test_correct_emulation_within_budget(mode):
    rng = np.random.default_rng(5)
    for seed, (M, N, K) in enumerate([(24, 320, 128), (9, 192, 64), (5, 640, 768)]):
        r = _ratio(mode, "erf", M, N, K, seed)
        rn = _ratio(mode, "erf", M, N, K, seed, nudge=rng)
        print(f"BUDGET gelu-erf-emulation {mode} {r:.3f} (nudged {rn:.3f}) M={M} N={N} K={K}")
        assert r <= 1.0 and rn <= 1.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wrong", ["quick", "tanh"])
def test_wrong_activations_break_the_budget(mode, wrong):
    """QuickGELU and the tanh form in place of GELU, accumulation term included: far outside in every mode, on the whole
    axis and on the stretch [-4, -2.5] alone."""
    r = _ratio(mode, wrong)
    rs = _ratio(mode, wrong, only=(-4.0, -2.5))
    print(f"BUDGET gelu-erf-mutation {wrong} {mode} {r:.1f} ([-4, -2.5]: {rs:.1f})")
    assert r > 10.0 and rs > 10.0


@pytest.mark.parametrize("mode", MODES)
def test_naive_fp32_erf_form_is_inside_the_budget(mode):
    """0.5 x (1 + erf(x / sqrt 2)) in fp32 cancels completely below x ~ -5.5 — an error of all of |ref| and of a fraction
    of a u32 of |x|: inside a budget relative to |x|."""
    r = _ratio(mode, "naive")
    print(f"BUDGET gelu-erf-naive {mode} {r:.3f}")
    assert r <= 1.0
