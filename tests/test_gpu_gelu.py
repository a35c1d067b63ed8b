"""The exact-GELU MLPs (mcm_config.v_hidden_act / t_hidden_act = MCM_ACT_GELU; EPI_GELU_ERF / EPI_GELU_ERF_X2) on the GPU:
  * the fc1 epilogue through mcm_op_linear_ex + MCM_LINEAR_ACT_GELU against the fp64 reference under tests/gelu_budget.py, in
    every mode and split form, at the shapes the size policy routes to each of the four kernels, pre-activations over [-8, 8];
    bit-equal across every forced GEMM variant of the harness library;
  * the device function gelu_erf on every finite fp32 bit pattern (mcm_debug_op_act);
  * whole towers: the fp32 arm against HF CLIPModel with hidden_act = "gelu" on the device, the split-activation arm against
    the fp32 arm, the bf16 arm once, and the same weights under a QuickGELU handle as the negative control;
  * batch-split invariance and determinism, bitwise; the CLI at a small size.

Each budget check prints "BUDGET <what> <mode> <worst max|got - ref| / budget>" (run with -s to collect them)."""
import ctypes

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gelu_budget as gb
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREC = {"bf16": 0, "fp32": 1, "fp16": 2}
DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
SPLIT_W, SPLIT_X, SPLIT_OUT, ACT_GELU = 1, 2, 4, 8
EINVAL = -1


def _tiny(harness, precision="fp16"):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny-gelu")
    return NativeCLIP(geo, synth_state_dict(geo, 0, "fp16-exact"), precision=precision, max_batch=64, max_prompt_tokens=4096,
                      harness=harness)


@pytest.fixture(scope="module")
def net():
    """An fp16 handle of the SHIPPED library: its own kernel choice, no switches."""
    n = _tiny(False)
    yield n
    n.close()


@pytest.fixture(scope="module")
def harness_net():
    n = _tiny(True)
    yield n
    n._lib.mcm_debug_gemm_variant(-1)
    n.close()


_ptr = gs.ptr


_check = gs.check_budget


# ---- the fc1 epilogue, operator level -------------------------------------------------------------------------------------
FORMS = {  # id: (operand mode, flags)
    "bf16": ("bf16", 0), "fp16": ("fp16", 0), "fp32": ("fp32", 0),
    "fp16-X": ("fp16", SPLIT_X), "fp16-X-OUT": ("fp16", SPLIT_X | SPLIT_OUT),
    "bf16-W": ("bf16", SPLIT_W), "fp16-W": ("fp16", SPLIT_W), "fp16-W-X-OUT": ("fp16", SPLIT_W | SPLIT_X | SPLIT_OUT),
}


def _split_dev(v32):
    """fp32 [M, K] on the device -> its split fp16 image [M, 2K] (error_budget.split_image's bits: no value near the range
    edge here)."""
    M, K = v32.shape
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    return torch.stack((hi.view(M, K // 64, 64), lo.view(M, K // 64, 64)), dim=2).reshape(M, 2 * K).contiguous()


def _operands(M, N, K, mode, flags, seed):
    """x, w as the call takes them (device) and getters of their exact values; lin ~ bias[n] + N(0, 0.25): the bias sweeps
    [-8, 8] over the columns."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x32 = 0.25 * torch.randn((M, K), generator=g, device="cuda")
    w32 = torch.randn((N, K), generator=g, device="cuda") * K ** -0.5
    bias = torch.linspace(-8.0, 8.0, N, device="cuda")
    if flags & SPLIT_X:
        x = _split_dev(x32)
        x_rows = lambda ri: eb.merge_image(x[ri].cpu().numpy())  # noqa: E731
    else:
        x = x32.to(DTYPE[mode])
        x_rows = lambda ri: x[ri].double().cpu().numpy()  # noqa: E731
    return x, x_rows, w32, bias


def _run(n, mode, flags, x, w, bias, M, N, K, epi=1):
    out_split = bool(flags & SPLIT_OUT)
    y = torch.zeros((M, 2 * N if out_split else N), device="cuda", dtype=torch.float16 if out_split else DTYPE[mode])
    rc = n._lib.mcm_op_linear_ex(n._h, PREC[mode], _ptr(x), _ptr(w), _ptr(bias), _ptr(y), None, M, N, K, epi, flags | ACT_GELU, None)
    assert rc == 0, n._lib.mcm_last_error(n._h)
    torch.cuda.synchronize()
    return y


def _weight(n, mode, flags, w32):
    """The weight as the call takes it and its exact value (host fp64)."""
    if flags & SPLIT_W:
        N, K = w32.shape
        img = torch.empty((N, 2 * K), device="cuda", dtype=DTYPE[mode])
        assert n._lib.mcm_op_split_weight(n._h, PREC[mode], _ptr(w32), N, K, _ptr(img), None) == 0
        torch.cuda.synchronize()
        return img, eb.merge_image(img.double().cpu().numpy())
    w = w32.to(DTYPE[mode])
    return w, w.double().cpu().numpy()


def _op_check(n, form, M, N, K, seed, rows=None, what="gelu-erf"):
    mode, flags = FORMS[form]
    x, x_rows, w32, bias = _operands(M, N, K, mode, flags, seed)
    w, wm = _weight(n, mode, flags, w32)
    y = _run(n, mode, flags, x, w, bias, M, N, K)
    rows = np.arange(M) if rows is None else rows
    ri = torch.from_numpy(rows).cuda()
    lin, s = eb.gemm_reference(x_rows(ri), wm, bias.cpu().numpy())
    assert lin.min() < -7.5 and lin.max() > 7.5 and ((lin > -4) & (lin < -2.5)).sum() > 100
    out_split = bool(flags & SPLIT_OUT)
    got = eb.merge_image(y[ri].cpu().numpy()) if out_split else y[ri].double().cpu().numpy()
    assert np.isfinite(got).all()
    ref, bud = gb.gemm_gelu_budget(lin, s, mode, out_split=out_split)
    return _check(what, form, got, ref, bud, f"M={M} N={N} K={K}")


# (tag, M, N, K): the fc1 problems as the size policy routes them on 256 CUs
LARGE = [
    ("B16-b512-pingpong", 512 * 197, 3072, 768),
    ("L14-b256-pingpong", 256 * 257, 4096, 1024),
    ("ragged-p256", 1000 * 77, 2048, 512),
]
SMALL = [
    ("tile128", 2040, 4096, 1024),
    ("tile64", 1000, 3072, 768),
    ("tile64-cls", 32, 3072, 768),
]


@pytest.mark.parametrize("form", ["bf16", "fp16"])
@pytest.mark.parametrize("tag,M,N,K", LARGE, ids=[s[0] for s in LARGE])
def test_fc1_full_size_16bit_within_budget(net, tag, M, N, K, form):
    _op_check(net, form, M, N, K, seed=M + N, rows=eb.sample_rows(M), what=f"gelu-erf-{tag}")


@pytest.mark.parametrize("form", ["fp32", "fp16-X", "fp16-X-OUT", "bf16-W", "fp16-W", "fp16-W-X-OUT"])
@pytest.mark.parametrize("tag,M,N,K", [("B16-b128-pingpong", 25600, 3072, 768), ("ragged-p256", 25216, 3072, 768)],
                         ids=["pingpong", "ragged-p256"])
def test_fc1_full_size_other_forms_within_budget(net, tag, M, N, K, form):
    """The exact-fp32 arm, the split-activation arm's forms and split weights at a batch-128 ViT-B/16 fc1: whole tiles
    (ping-pong kernel) and the unpadded ragged M (plain persistent kernel)."""
    _op_check(net, form, M, N, K, seed=M + N + 1, rows=eb.sample_rows(M), what=f"gelu-erf-{tag}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tag,M,N,K", SMALL, ids=[s[0] for s in SMALL])
def test_fc1_small_shapes_every_element_within_budget(net, tag, M, N, K, form):
    _op_check(net, form, M, N, K, seed=M + N + 2, what=f"gelu-erf-{tag}")


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
def test_every_gemm_variant_gives_the_same_bits(net, harness_net, mode):
    """Whole tiles and a ragged problem under every kept variant of the harness library and the shipped library's own choice:
    one bit pattern.  Variant 9, the arms' text of the ping-pong kernel, has no erf epilogue: the call is refused, never run
    through an arm's QuickGELU."""
    for M, N, K in ((1024, 512, 192), (1000, 208, 64)):
        x, _, w32, bias = _operands(M, N, K, mode, 0, seed=M + K)
        w = w32.to(DTYPE[mode])
        want = _run(net, mode, 0, x, w, bias, M, N, K)
        lin, s = eb.gemm_reference(x.double().cpu().numpy(), w.double().cpu().numpy(), bias.cpu().numpy())
        ref, bud = gb.gemm_gelu_budget(lin, s, mode)
        _check("gelu-erf-variants", mode, want.double().cpu().numpy(), ref, bud, f"M={M} N={N} K={K}")
        for v in (-1, 0, 3, 4, 5, 11):
            assert harness_net._lib.mcm_debug_gemm_variant(v) == 0
            try:
                got = _run(harness_net, mode, 0, x, w, bias, M, N, K)
            finally:
                harness_net._lib.mcm_debug_gemm_variant(-1)
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (mode, v, M, N, K)
        assert harness_net._lib.mcm_debug_gemm_variant(9) == 0
        try:
            y = torch.zeros((M, N), device="cuda", dtype=DTYPE[mode])
            L, h = harness_net._lib, harness_net._h
            assert L.mcm_op_linear_ex(h, PREC[mode], _ptr(x), _ptr(w), _ptr(bias), _ptr(y), None, M, N, K, 1, ACT_GELU, None) != 0
            assert L.mcm_op_linear_ex(h, PREC[mode], _ptr(x), _ptr(w), _ptr(bias), _ptr(y), None, M, N, K, 1, 0, None) == 0
        finally:
            harness_net._lib.mcm_debug_gemm_variant(-1)
        torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["fp16-X", "fp16-X-OUT", "fp16-W", "bf16-W", "fp16-W-X-OUT"])
def test_split_forms_give_the_same_bits_in_every_kernel(net, form):
    """The split forms refuse forced variants, so the kernels are compared through the size policy: the first rows of one
    problem computed as part of M = 25 600 (whole tiles: ping-pong), of M = 25 216 (ragged: plain persistent), as M = 2 048
    (128x128 tile kernel at N = 4 096) and as M = 1 000 / 32 (64x128 tile kernel) — a row's bits must not depend on it."""
    mode, flags = FORMS[form]
    N, K = 4096, 768
    x, _, w32, bias = _operands(25600, N, K, mode, flags, seed=77)
    w, _ = _weight(net, mode, flags, w32)
    want = _run(net, mode, flags, x, w, bias, 25600, N, K)
    for M in (25216, 2048, 1000, 32):
        got = _run(net, mode, flags, x, w, bias, M, N, K)
        assert torch.equal(got.view(torch.uint8), want[:M].view(torch.uint8)), (form, M)


def test_the_flag_is_refused_where_it_has_no_meaning(net):
    x = torch.zeros((64, 64), device="cuda", dtype=torch.float16)
    y = torch.zeros((64, 128), device="cuda", dtype=torch.float16)
    r = torch.zeros((64, 64), device="cuda")
    L, h = net._lib, net._h
    for epi in (0, 2):
        assert L.mcm_op_linear_ex(h, 2, _ptr(x), _ptr(x), None, _ptr(y), _ptr(r), 64, 64, 64, epi, ACT_GELU, None) == EINVAL
    assert L.mcm_op_linear_ex(h, 2, _ptr(x), _ptr(x), None, _ptr(y), None, 64, 64, 64, 1, 16, None) == EINVAL
    assert L.mcm_op_linear_ex(h, 0, _ptr(x), _ptr(x), None, _ptr(y), None, 64, 64, 64, 1, ACT_GELU | SPLIT_OUT, None) == EINVAL  # bf16
    assert L.mcm_op_linear_ex(h, 2, _ptr(x), _ptr(x), None, _ptr(y), None, 64, 64, 64, 1, ACT_GELU, None) == 0
    torch.cuda.synchronize()


def test_create_rejects_an_unknown_activation(net):
    from mcm_amd.config import geometry

    for field in ("v_hidden_act", "t_hidden_act"):
        for bad in (2, -1):
            cfg = geometry("tiny").to_c(precision=2, max_batch=4, max_prompt_tokens=256)
            setattr(cfg, field, bad)
            h = ctypes.c_void_p()
            assert net._lib.mcm_create(ctypes.byref(cfg), ctypes.byref(h)) == EINVAL and not h.value


# ---- the device function on every finite fp32 input -----------------------------------------------------------------------
def test_gelu_erf_on_every_finite_fp32(harness_net):
    """All 2 x (2^31 - 2^23) finite bit patterns in chunks of 2^26, compared on the device with 0.5 x erfc(-x / sqrt 2) in
    float64 under the activation term of the budget, C_GELU_ERF u32 |x| + one fp32 ulp of the reference; no finite input
    gives NaN (or inf)."""
    L, h = harness_net._lib, harness_net._h
    n = 1 << 26
    base = torch.arange(n, device="cuda", dtype=torch.int64)
    y = torch.empty(n, device="cuda", dtype=torch.float32)
    worst, worst_x, worst_abs, worst_abs_x = 0.0, 0.0, 0.0, 0.0
    for sign in (0, 1 << 31):
        for start in range(0, 0x7F800000, n):
            bits = base[: min(n, 0x7F800000 - start)] + (start + sign)
            x = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)   # two's-complement wrap of the sign bit
            assert L.mcm_debug_op_act(h, 2, _ptr(x), _ptr(y), x.numel(), None) == 0
            got = y[: x.numel()]
            assert bool(torch.isfinite(got).all()), f"non-finite output in chunk {start + sign:#x}"
            x64 = x.double()
            ref = 0.5 * x64 * torch.special.erfc(-x64 * 0.7071067811865476)
            e = torch.frexp(ref.abs())[1] - 1
            e = torch.where(ref == 0, torch.full_like(e, -126), e).clamp(min=-126)
            bud = gb.C_GELU_ERF * eb.U32 * x64.abs() + torch.ldexp(torch.ones_like(ref), e - 23)
            err = (got.double() - ref).abs()
            r = err / bud
            i = int(torch.argmax(r))
            if float(r[i]) > worst:
                worst, worst_x = float(r[i]), float(x[i])
            nz = x64 != 0
            q = torch.where(nz, err / (eb.U32 * x64.abs()).clamp(min=1e-300), torch.zeros_like(err))
            big = x64.abs() > 2.0 ** -100   # (below, the ulp of the reference is what the error is measured in)
            q = torch.where(big, q, torch.zeros_like(q))
            j = int(torch.argmax(q))
            if float(q[j]) > worst_abs:
                worst_abs, worst_abs_x = float(q[j]), float(x[j])
    print(f"BUDGET gelu-erf-device-function fp32 {worst:.3f} at x = {worst_x!r}; worst |error| = {worst_abs:.2f} u32 |x| at "
          f"x = {worst_abs_x!r}")
    assert worst <= 1.0


# ---- towers -------------------------------------------------------------------------------------------------------------
def _nets_scores(geo, sd, px, ids, mask, precisions, layers_note=""):
    from mcm_amd.engine import NativeCLIP

    out = {}
    bank = None
    for p in precisions:
        n = NativeCLIP(geo, sd, precision=p, max_batch=px.shape[0], max_prompt_tokens=100 * 16)
        try:
            if bank is None:   # the text tower is fp32 in every handle: one bank
                bank = n.get_text_features(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), normalize=True)
            out[p] = n.score_images(px, bank).double()
            if p == "fp16":
                out["x2"] = n.score_images_x2(px, bank).double()
                assert n.saturation_count() == 0
        finally:
            n.close()
    return out, bank


def _tower_vs_hf(ckpt, layers=None, with_controls=False):
    """tests/test_gpu_l14_336.py::test_full_tower_vs_hf_and_the_split_arm on a `gelu` checkpoint, its bars unchanged."""
    import dataclasses

    from mcm_amd.config import geometry
    from mcm_amd.synth import make_token_ids
    from mcm_amd.weights import synth_state_dict
    from oracle.hf_reference import HFReference

    geo = geometry(ckpt)
    if layers is not None:
        geo = dataclasses.replace(geo, name=f"{ckpt}-{layers}L", v_layers=layers, t_layers=layers)
    sd = synth_state_dict(geo, 0, "fp16-exact")
    ids, mask = make_token_ids(100, seed=2)
    B = 32
    g = torch.Generator(device="cuda").manual_seed(7)
    px = torch.randn((B, 3, geo.image_size, geo.image_size), device="cuda", generator=g)
    s, bank = _nets_scores(geo, sd, px, ids, mask, ["fp32", "fp16"] + (["bf16"] if with_controls else []))
    hf = HFReference(geo, sd, device="cuda")
    assert hf.model.config.vision_config.hidden_act == "gelu" and hf.model.config.text_config.hidden_act == "gelu"
    hf.set_bank(ids, mask)
    shf = hf.score_batch(px).double()
    del hf
    torch.cuda.empty_cache()
    d_hf = (s["fp32"] - shf).abs()
    d16, d2 = float((s["fp16"] - s["fp32"]).abs().max()), float((s["x2"] - s["fp32"]).abs().max())
    ulp = float(np.spacing(np.float32(shf.abs().max().item())))
    print(f"{geo.name}: |fp32 arm - HF| max {float(d_hf.max()) / ulp:.2f} ulp rms {float(d_hf.pow(2).mean().sqrt()) / ulp:.2f} ulp "
          f"(ulp {ulp:.2e}); |d score| fp16 arm {d16:.2e}, split-activation arm {d2:.2e} (scores ~ {float(s['fp32'].abs().mean()):.3e})")
    assert float(d_hf.pow(2).mean().sqrt()) <= 2 * ulp and float(d_hf.max()) <= 4 * ulp, ulp
    assert d2 <= 2e-9 and d2 <= 0.1 * d16, (d2, d16)
    if not with_controls:
        return
    # the same weights, pixels and prompts under the QuickGELU geometry: the negative control (the test can see the activation)
    # and the yardstick of the bf16 arm
    base = geometry(ckpt[:-len("-laion2b")])
    q, _ = _nets_scores(base, sd, px, ids, mask, ["fp32", "bf16"])
    d_neg = float((q["fp32"] - shf).abs().max())
    rms = lambda d: float(d.pow(2).mean().sqrt())  # noqa: E731  (over the 32 scores: steadier than their max)
    dbf, dbf_q = rms(s["bf16"] - s["fp32"]), rms(q["bf16"] - q["fp32"])
    print(f"{geo.name}: QuickGELU handle vs HF-gelu max {d_neg:.2e} = {d_neg / (4 * ulp):.0f} x the bar; bf16 arm vs fp32 arm rms "
          f"{dbf:.2e} (QuickGELU model: {dbf_q:.2e})")
    assert d_neg > 100 * 4 * ulp
    # The bf16 arm's distance from the fp32 arm is the rounding of its MFMA operands (u = 2^-8 per activation and weight),
    # which is the same in both models; the activation only changes which values are rounded.  The rms distance within a
    # factor 2 of the QuickGELU model's own, and finite.
    assert np.isfinite(dbf) and dbf <= 2.0 * dbf_q, (dbf, dbf_q)


def test_b16_laion2b_tower_vs_hf_the_split_arm_and_the_controls():
    _tower_vs_hf("ViT-B/16-laion2b", with_controls=True)


def test_l14_laion2b_tower_vs_hf_and_the_split_arm():
    _tower_vs_hf("ViT-L/14-laion2b")


def test_scores_do_not_depend_on_the_batch_and_repeat_bitwise():
    """96 images at once (persistent kernels) against the same images in batches of 8 and 40 (tile kernels), twice: the same
    float32 scores, bit for bit, in the fp16 arm and the split-activation arm of a `gelu` handle."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.synth import make_token_ids
    from mcm_amd.weights import synth_state_dict

    geo = geometry("ViT-B/16-laion2b")
    sd = synth_state_dict(geo, 0, "fp16-exact")
    ids, mask = make_token_ids(100, seed=2)
    g = torch.Generator(device="cuda").manual_seed(9)
    px = torch.randn((96, 3, 224, 224), device="cuda", generator=g)
    n = NativeCLIP(geo, sd, precision="fp16", max_batch=96, max_prompt_tokens=100 * 16)
    try:
        bank = n.get_text_features(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), normalize=True)
        for fn in (n.score_images, n.score_images_x2):
            whole = fn(px, bank).clone()
            again = fn(px, bank).clone()
            parts = torch.cat([fn(px[a:b], bank).clone() for a, b in ((0, 8), (8, 48), (48, 96))])
            assert torch.equal(whole, again) and torch.equal(whole, parts), fn.__name__
        assert n.saturation_count() == 0
    finally:
        n.close()


def test_cli_laion2b_fp16_refined_against_fp32(tmp_path, monkeypatch):
    """`--CLIP_ckpt ViT-B/16-laion2b --synthetic` at a small size: the fp16 run with threshold refinement against `--dtype
    fp32` — AUROC within 1e-4, FPR95 equal."""
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    common = ["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/16-laion2b", "--synthetic", "--synthetic-n", "200", "-b", "64"]
    r32 = cli.main(common + ["--dtype", "fp32", "--name", "g_fp32"])
    r16 = cli.main(common + ["--dtype", "fp16", "--name", "g_fp16"])
    assert "refine" in r16
    for k in r32["measures"]:
        a32, _, f32 = r32["measures"][k]
        a16, _, f16 = r16["measures"][k]
        print(f"laion2b CLI {k}: AUROC fp32 {a32:.6f} fp16 {a16:.6f}, FPR95 fp32 {f32:.6f} fp16 {f16:.6f}")
        assert abs(a16 - a32) <= 1e-4 and f16 == f32, (k, r16["measures"][k], r32["measures"][k])
    assert (tmp_path / "results/ImageNet10/MCM/CLIP_ViT-B/16-laion2b_T_1_ID_g_fp16/g_fp16.csv").exists(), list(tmp_path.rglob("*.csv"))
