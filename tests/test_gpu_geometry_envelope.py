"""Every kind of geometry mcm_create accepts (include/mcm.h, the comment above mcm_create; tests/geometry_envelope.py), away
from the shipped checkpoints' shapes: the kernel paths only such geometries reach under the fp64 budgets of
tests/error_budget.py, the whole towers against the C oracle (itself held to HF CLIPModel at these geometries by
tests/test_geometry_envelope_cpu.py), and the refusals one step outside the envelope.

Operator level (each check prints "BUDGET <family> <mode> <worst max|got - ref| / budget>", run with -s to collect them):
  * the ping-pong GEMM with an odd number of K-steps and several tiles per workgroup (the stage parity of its flat two-stage
    pipeline is carried from one tile into the next), every epilogue, the split-activation and split-weight forms;
  * the persistent GEMM with a ragged last N tile under many row tiles, whole and ragged M;
  * LayerNorm and pool_project at widths with whole 256-column slots plus a partial one, proj_dim down to 4;
  * attention at 1, 5, 17, 20 heads of 64 and 4, 8, 12 heads of 80, and the causal fp32 form up to the longest prompt it launches;
  * the vision front at patch sizes 4, 7, 8, 24, 32 (two tokens) and 64, on the pixel-gathering and the patchify route.
Whole towers: MCM scores of every envelope geometry in every arm at the bounds tests/test_gpu_h14.py holds H14-2L-quick to
(fp32 and the split-activation arm 2e-6, fp16 2e-4, bf16 1e-3), float and uint8 ingest, batch-split invariance; the text tower
at 32, 248 and 306 positions at every sequence-length class.

Measured on one MI355X (EXPERIMENTS.md, "The envelope of accepted geometries", has the table per geometry and arm): worst
max|score - oracle| fp32 1.5e-8, split-activation 1.5e-8, fp16 4.8e-6, bf16 3.0e-5 (both at the 2-token, 4 x 80 tower); text
features within 1.9e-7; every operator family inside its budget (the 16-bit ones at the half ulp of their output format)."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from tests import error_budget as eb
from tests import geometry_envelope as ge
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import test_gpu_attention_hd80 as hd80  # noqa: E402
from tests import test_gpu_error_budget as ops  # noqa: E402
from tests import test_gpu_split_budget as split  # noqa: E402
from tests import test_gpu_tower_ends_budget as ends  # noqa: E402
from tests.test_gpu_h14 import _linear_check  # noqa: E402

PREC = {"bf16": 0, "fp32": 1, "fp16": 2}
DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
MODES = ["bf16", "fp16", "fp32"]
_ptr = gs.ptr
_check = functools.partial(gs.check_budget, finite_budget=True)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tiny(harness):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    return NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=64, max_prompt_tokens=4096, harness=harness)


@pytest.fixture(scope="module")
def net():
    """A handle of the shipped library: its own kernel choice."""
    n = _tiny(False)
    yield n
    assert n.kernel_faults == 0
    n.close()


@pytest.fixture(scope="module")
def hnet():
    """A handle of the harness library: forced GEMM variants, the persistent grid, head_dim as an argument."""
    n = _tiny(True)
    yield n
    n._lib.mcm_debug_gemm_variant(-1)
    n._lib.mcm_debug_persistent_grid(0)
    assert n.kernel_faults == 0
    n.close()


# ---- ping-pong GEMM: an odd number of K-steps carried across the tiles of a workgroup ------------------------------------
# 4096 rows are 16 row tiles; on 8 workgroups (one per XCD) each walks 2 tiles at N = 256 and 4 at N = 512, so with nk odd the
# second tile's first K-step lands in the other LDS stage than the first tile's did.  K-steps: 1, 3, 5.
PP_M = 4096
PP_K = {"bf16": (64, 192, 320), "fp16": (64, 192, 320), "fp32": (32, 96, 160)}


@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("N", [256, 512])
def test_pingpong_gemm_odd_ksteps_across_tiles_within_budget(hnet, N, prec):
    """Harness variant 5 on a grid of 8: every element of every epilogue (store, QuickGELU, residual, and the erf GELU through
    mcm_op_linear_ex).
    What it would catch: gemm_pp_kernel reads step s from LDS stage sr = s & 1 and stages step s + 1 into sr ^ 1, s counted
    over all tiles of the workgroup.  With the stage taken as 0 at a tile's first step, the second tile of a workgroup with nk
    odd computes its first K-step from the stage that still holds the previous tile's second-to-last one: whole 256 x 256
    tiles off by O(1) (tests/test_geometry_envelope_cpu.py models the schedule: stale exactly when nk is odd and a workgroup
    has a second tile, which these shapes are and no earlier shape of the suite was)."""
    lib = hnet._lib
    try:
        assert lib.mcm_debug_gemm_variant(5) == 0 and lib.mcm_debug_persistent_grid(8) == 0
        for K in PP_K[prec]:
            for epi in (0, 1, 2):
                ops._gemm_check(hnet, PP_M, N, K, prec, epi, seed=N + K + epi, what="gemm-pp-odd")
            _linear_check(hnet, "pp-odd-erf", N, K, 1, PP_M, prec, np.arange(PP_M))
    finally:
        lib.mcm_debug_gemm_variant(-1)
        lib.mcm_debug_persistent_grid(0)


@pytest.mark.parametrize("form", ["fp16-X", "fp16-X-OUT", "bf16-W", "fp16-W", "fp16-W-X-OUT"])
@pytest.mark.parametrize("N", [256, 512])
def test_pingpong_gemm_split_forms_three_logical_ksteps_across_tiles_within_budget(hnet, N, form):
    """K = 192 in the split forms (two or four passes per logical K-step: kstep_off's xsplit / ksplit arms) on a grid of 8.  The
    split forms refuse a forced variant, so the kernel is the size policy's choice: 16 or 32 whole tiles on 8 workgroups are
    more than half a round, which is the ping-pong kernel (gemm.hip size_policy / gemm_route), and 2 or 4 whole rounds leave
    no sliver to cut."""
    lib = hnet._lib
    try:
        assert lib.mcm_debug_gemm_variant(-1) == 0 and lib.mcm_debug_persistent_grid(8) == 0
        for epi in (0, 1, 2):
            _linear_check(hnet, "pp-odd-split", N, 192, epi, PP_M, form, np.arange(PP_M))
    finally:
        lib.mcm_debug_persistent_grid(0)


@pytest.mark.parametrize("prec", MODES)
def test_pingpong_gemm_odd_ksteps_shipped_policy_within_budget(net, prec):
    """The shipped library on the whole part: 48 x 3 whole tiles are past half a round (the ping-pong kernel), 3 and 5 K-steps."""
    M, N = 12288, 768
    rows = eb.sample_rows(M)
    for K in PP_K[prec][1:]:
        for epi in (0, 1, 2):
            ops._gemm_check(net, M, N, K, prec, epi, seed=K + epi, rows=rows, what="gemm-pp-odd-shipped")
        _linear_check(net, "pp-odd-shipped-erf", N, K, 1, M, prec, rows)


# ---- persistent GEMM: a ragged last N tile under many row tiles -------------------------------------------------------------
RAGGED_N = [320, 960, 1152]          # 64, 192 and 128 columns in the last 256-column tile


@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("variant", [3, 4], ids=["persist256", "persist256-counted-stores"])
def test_persistent_gemm_ragged_n_many_row_tiles_within_budget(hnet, variant, prec):
    """16 whole row tiles, and 16 plus one row, dealt to the 8 XCDs; sampled rows (both sides of every 64-row boundary, the
    first and last 256: the ragged last row tile whole).
    What it would catch: the last N tile computes 256 columns from W rows clamped to N - 1 (gemm_p256_kernel, "edge tile") and
    stores only those below N.  Without that column test, row m's columns N ... would land on the next row's columns 0 ...
    255 - N % 256 (ldo = N), which another tile writes at another time: whichever store comes last, consecutive sampled rows
    hold a neighbour's values in their leading columns — and the residual epilogue adds into them a second time."""
    lib = hnet._lib
    try:
        assert lib.mcm_debug_gemm_variant(variant) == 0
        for M in (4096, 4097):
            rows = eb.sample_rows(M)
            for N in RAGGED_N:
                for K in PP_K[prec][1:]:
                    for epi in (0, 1, 2):
                        ops._gemm_check(hnet, M, N, K, prec, epi, seed=M + N + K + epi, rows=rows, what=f"gemm-ragged-n-v{variant}")
    finally:
        lib.mcm_debug_gemm_variant(-1)


@pytest.mark.parametrize("prec", MODES)
def test_persistent_gemm_ragged_n_shipped_policy_within_budget(net, prec):
    """66 x 2 tiles with a ragged last row (one row) and a ragged last N tile: past half a round and not whole tiles, so the
    shipped policy takes the persistent kernel.  The last row is among the sampled ones."""
    M, N = 16641, 320
    rows = eb.sample_rows(M)
    assert rows[-1] == M - 1
    K = PP_K[prec][2]
    for epi in (0, 1, 2):
        ops._gemm_check(net, M, N, K, prec, epi, seed=K + epi, rows=rows, what="gemm-ragged-n-shipped")


# ---- LayerNorm: whole 256-column vector slots plus a partial one ------------------------------------------------------------
ENV_D = [192, 320, 832, 1088, 1216]
GUARD = 1.0e3        # what lies behind the rows: a lane that reads past its row's end takes these into the statistics


def _ln_case(M, D, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, D)) * 2 + 0.5).astype(np.float32)
    x[0] *= 100.0                          # a loud row
    x[-1, D // 256 * 256:] += 50.0         # outliers, all of them in the partial slot
    if M > 2:
        x[1] = (1e3 + 1e-2 * rng.standard_normal(D)).astype(np.float32)
        x[2, ::7] += 30.0
    g = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    xd = _dev(np.concatenate([x, np.full((1, D), GUARD, np.float32)]))     # one guard row behind the M rows
    return x, g, b, xd


@pytest.mark.parametrize("mode", MODES + ["fp32-out", "split"])
@pytest.mark.parametrize("D", ENV_D)
def test_layernorm_partial_slot_within_budget(net, D, mode):
    for M in (1, 5):
        x, g, b, xd = _ln_case(M, D, D + M)
        gd, bd = _dev(g), _dev(b)
        if mode == "split":
            y = torch.zeros((M, 2 * D), device="cuda", dtype=torch.float16)
            rc = net._lib.mcm_op_layernorm_split(net._h, _ptr(xd), _ptr(gd), _ptr(bd), _ptr(y), M, D, 1e-5, None)
            assert rc == 0, net._lib.mcm_last_error(net._h)
            torch.cuda.synchronize()
            split._canonical("layernorm", y)
            ref, bud = eb.layernorm_split_budget(x, g, b)
            got = eb.merge_image(y.cpu().numpy())
        else:
            prec = "fp16" if mode == "fp32-out" else mode      # fp32-out: a 16-bit handle mode writing fp32 rows
            out = "fp32" if mode == "fp32-out" else mode
            y = torch.zeros((M, D), device="cuda", dtype=DTYPE[out])
            rc = net._lib.mcm_op_layernorm(net._h, PREC[prec], _ptr(xd), _ptr(gd), _ptr(bd), _ptr(y), M, D, 1e-5,
                                           int(mode == "fp32-out"), None)
            assert rc == 0, net._lib.mcm_last_error(net._h)
            torch.cuda.synchronize()
            ref, bud = eb.layernorm_budget(x, g, b, out)
            got = y.float().cpu().numpy()
        _check("layernorm-env", mode, got, ref, bud, f"D={D} M={M}")


# ---- pool_project -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 192, 320, 1088, 1216])
def test_pool_project_envelope_widths_within_budget(hnet, D):
    """proj_dim 4 (fewer outputs than the workgroup has waves), 100, 260 and 1020; 5 rows pooled by stride and by index, raw and
    normalised; one guard row behind the pooled ones."""
    n, stride = 5, 17
    for P in (4, 100, 260, 1020):
        g, b, proj = ends._pool_params(D, P, D + P)
        gd, bd, pd = _dev(g), _dev(b), _dev(proj)
        pooled = ends._pool_rows(n, D, seed=D + P)
        x = np.full((n * stride + 1, D), GUARD, np.float32)
        x[:n * stride:stride] = pooled
        idx = (np.arange(n, dtype=np.int32) * stride)[::-1].copy()
        xd = _dev(x)
        for normalize in (0, 1):
            for by_index in (False, True):
                rc, out = ends._pool(hnet, xd, idx if by_index else None, 0 if by_index else stride, n, D, gd, bd, pd, P, normalize)
                assert rc == 0, hnet._lib.mcm_last_error(hnet._h)
                ref, bud = eb.pool_project_budget(pooled[::-1] if by_index else pooled, g, b, proj, bool(normalize))
                _check("pool-env" if normalize else "pool-env-raw", "fp32", out.cpu().numpy(), ref, bud,
                       f"D={D} P={P} by_index={by_index}")


# ---- attention: head counts ---------------------------------------------------------------------------------------------------
ATTN_L = [2, 17, 65]


@pytest.mark.parametrize("mode", MODES + ["split"])
@pytest.mark.parametrize("heads", [1, 5, 17, 20])
def test_attention_head_counts_of_64_within_budget(net, heads, mode):
    for L in ATTN_L:
        for nseq in (1, 3):
            if mode == "split":
                img = split._attn_img(nseq, L, heads, seed=L + heads)
                out = split._attention_split(net, _dev(img), nseq, L, heads)
                split._attn_check("attention-env", img, out, nseq, L, heads)
            else:
                qkv = ops._attn_qkv(nseq, L, heads, mode, seed=L * 7 + heads)
                out = ops._attention(net, mode, qkv, nseq, L, heads, False)
                ops._attn_check("attention-env", mode, qkv, out, nseq, L, heads, False)


@pytest.mark.parametrize("mode", MODES + ["split"])
@pytest.mark.parametrize("heads", [4, 8, 12])
def test_attention_head_counts_of_80_within_budget(hnet, heads, mode):
    """(A split row is whole 64-column blocks: heads x 80 a multiple of 64, which 4, 8 and 12 are.)"""
    for L in ATTN_L:
        for nseq in (1, 3):
            qd = hd80._device_operands(mode, hd80._qkv(nseq, L, heads, seed=L + heads))
            rc, out = hd80._run(hnet, mode, qd, nseq, L, heads)
            assert rc == 0, hnet._lib.mcm_last_error(hnet._h)
            assert torch.isfinite(out.float()).all()
            hd80._budget_check("env", mode, qd, out, nseq, L, heads)


@pytest.mark.parametrize("L", [78, 248, ge.MAX_POSITIONS_LIMIT])
def test_causal_fp32_attention_past_77_within_budget(net, L):
    """The text tower's attention (attn_f32_kernel<true>) at Long-CLIP's 248 positions and at the longest sequence it launches."""
    nseq, heads = 2, 3
    qkv = ops._attn_qkv(nseq, L, heads, "fp32", seed=L)
    out = ops._attention(net, "fp32", qkv, nseq, L, heads, True)
    ops._attn_check("attention-causal-long", "fp32", qkv, out, nseq, L, heads, True)


def test_causal_fp32_attention_refuses_one_past_its_longest_sequence(net):
    """Refused by launch_lds before anything is launched: the output is untouched."""
    nseq, L, heads = 1, ge.MAX_POSITIONS_LIMIT + 1, 1
    qkv = ops._attn_qkv(nseq, L, heads, "fp32", seed=1)
    out = torch.full((nseq * L, heads * 64), 7.0, device="cuda")
    rc = net._lib.mcm_op_attention(net._h, PREC["fp32"], _ptr(qkv), _ptr(out), nseq, L, heads, 1, None)
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 7.0).all())


# ---- vision front -------------------------------------------------------------------------------------------------------------
def _front_geo(name, P, image, width=768, heads=12):
    """A one-layer tower (the front does not depend on the layers behind it) with a narrow MLP."""
    from mcm_amd.config import ClipGeometry

    return ClipGeometry(name, image_size=image, patch_size=P, v_width=width, v_heads=heads, v_layers=1, v_mlp=64, t_width=64,
                        t_heads=1, t_layers=1, t_mlp=64, proj_dim=64)


def _takes_pixels(P, precision):
    """gemm_patch_takes_pixels' geometry rule (gemm.hip): P a multiple of a 16-byte chunk and a divisor of a 128-byte K-step,
    no K padding; the problem size is the caller's."""
    es = 4 if precision == "fp32" else 2
    kalign = 128 // es
    return P % (16 // es) == 0 and (128 // es) % P == 0 and (3 * P * P) % kalign == 0


# (P, image, images past which the persistent kernel takes the patch GEMM of a 768-wide tower on 256 CUs: 3 N tiles, more than
# 128 tiles in all = 43 row tiles of 256 patch rows)
FRONT_BIG = [(8, 64, 172), (64, 128, 2752)]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("P,image,big", FRONT_BIG, ids=["P8", "P64"])
def test_vision_front_patch_8_and_64_both_routes_within_budget(P, image, big, precision):
    """The pixel-gathering patch GEMM (gemm_p256_kernel<..., PXF>: its dpy / pxl / py0 arithmetic at 8 rows of 8 pixels per
    K-step and at one row of 64) and the patchify route (mcm_debug_patch_fold 0: patchify8_kernel), at a batch the persistent
    kernel takes (sampled rows) and at batch 3 (every element); uint8 pixels at batch 3."""
    geo = _front_geo(f"front-p{P}", P, image)
    assert ge.accepted(geo) is None
    f = ends.Front(geo, precision, max_batch=big, x2_max_batch=3 if precision == "fp16" else None)
    lib = f.net._lib
    gathers = _takes_pixels(P, precision)
    assert gathers == (not (P == 64 and precision == "fp32"))      # (an fp32 K-step is 32 elements: half a row of 64)
    try:
        px = ends._pixels(big, image, seed=P)
        rows = ends._full_rows(big, f.np)
        for fold in (1, 0):
            assert lib.mcm_debug_patch_fold(fold) == 0
            assert f.patchify_launches(px) == (0 if fold and gathers else 1), fold
            ends._front_check(f, px, px, False, f"P={P} B={big} fold={fold}", rows=rows)
            assert f.patchify_launches(px[:3]) == 1
            ends._front_check(f, px[:3], px[:3], False, f"P={P} B=3 fold={fold}")
            if precision == "fp16":
                ends._front_check(f, px[:3], px[:3], True, f"P={P} B=3 fold={fold}")
        u8 = ends._u8(3, image, seed=P)
        assert lib.mcm_debug_patch_fold(1) == 0
        ends._front_check(f, _dev(eb.u8_normalise(u8)), _dev(u8), False, f"P={P} B=3 u8")
        assert f.net.kernel_faults == 0
    finally:
        lib.mcm_debug_patch_fold(1)
        f.close()


# (envelope geometry, a batch whose patch rows pass a 256-row tile): P = 24 (patchify8 at 3 chunks per pixel row), P = 4 and 7
# (the generic patchify, K padded from 48 and 147), P = 8 at 192 columns, and the 2-token tower
FRONT_SMALL = [("p24", 65), ("w1088", 17), ("w320-h5x64", 17), ("w192", 17), ("w320-h4x80-2tok", 257), ("p64", 65)]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name,big", FRONT_SMALL, ids=[n for n, _ in FRONT_SMALL])
def test_vision_front_envelope_patch_sizes_within_budget(name, big, precision):
    """Every element of stage 0 (the patch embedding) and stage 1 (CLS row, pre_layrnorm, layer 0's layer_norm1: at 320 and 1088
    columns the partial vector slot of layernorm_pre_kernel), fp32 NCHW and uint8 NHWC pixels, the workspace poisoned; the fp16
    handle also runs the split-activation arm."""
    geo = ge.ENVELOPE[name]
    batches = [1, 3, big]
    f = ends.Front(geo, precision, max_batch=big, x2_max_batch=big if precision == "fp16" else None)
    try:
        assert big * f.np > 256
        for B in batches:
            for x2 in ((False, True) if precision == "fp16" else (False,)):
                tag = f"{name} B={B}"
                px = ends._pixels(B, geo.image_size, seed=B + len(name))
                ends._front_check(f, px, px, x2, tag, poison=1)
                u8 = ends._u8(B, geo.image_size, seed=B)
                ends._front_check(f, _dev(eb.u8_normalise(u8)), _dev(u8), x2, tag + " u8", poison=1)
        assert f.net.kernel_faults == 0
    finally:
        f.close()


# ---- whole towers -------------------------------------------------------------------------------------------------------------
TOWERS = [n for n in ge.ENVELOPE if n not in ge.TEXT_ONLY]
ARM_TOL = {"fp32": 2e-6, "x2": 2e-6, "fp16": 2e-4, "bf16": 1e-3}      # tests/test_gpu_h14.py, on a score in [0, 1]
K_PROMPTS, N_IMAGES = 10, 3


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Weights, inputs and the oracle's MCM scores of 3 images (float and uint8 pixels), computed once per geometry."""
    from mcm_amd.synth import make_pixels, make_token_ids
    from mcm_amd.weights import synth_state_dict
    from oracle import oracle as orc

    geo = ge.ENVELOPE[name]
    sd = synth_state_dict(geo, 0)
    ids, mask = make_token_ids(K_PROMPTS, seed=2)
    px, _ = make_pixels(N_IMAGES, geo.image_size, K_PROMPTS, ood=False, seed=1)
    u8 = np.random.default_rng(3).integers(0, 256, size=(N_IMAGES, geo.image_size, geo.image_size, 3), dtype=np.uint8)
    o = orc.OracleCLIP(geo, sd)
    txt = o.encode_text(ids)
    want = orc.score_features(o.encode_image(px), txt, 1.0, 0)
    want_u8 = orc.score_features(o.encode_image(eb.u8_normalise(u8)), txt, 1.0, 0)
    for a in (px, u8, want, want_u8, ids, mask):
        a.setflags(write=False)
    return geo, sd, ids, mask, px, u8, want, want_u8


def _tower_arms(tag, geo, sd, ids, mask, px, u8, want, want_u8):
    """Every arm at B = 3 and B = 1 against `want`; the fp16 handle also runs the split-activation arm and the batch-split
    check; the counters stay 0.  Returns {arm: max|score - want|}."""
    from mcm_amd.engine import NativeCLIP

    worst = {}
    pxd, u8d = torch.tensor(px).cuda(), torch.tensor(u8).cuda()      # (copies: the shared reference arrays are read-only)
    for precision in ("fp32", "fp16", "bf16"):
        n = NativeCLIP(geo, sd, precision=precision, max_batch=8, max_prompt_tokens=1024)
        try:
            txt = n.get_text_features(input_ids=torch.tensor(ids), attention_mask=torch.tensor(mask), normalize=True)
            arms = [(precision, n.score_images)] + ([("x2", n.score_images_x2)] if precision == "fp16" else [])
            for arm, score in arms:
                for B in (N_IMAGES, 1):
                    got = score(pxd[:B], txt, 1.0, "MCM").cpu().numpy()
                    got_u8 = score(u8d[:B], txt, 1.0, "MCM").cpu().numpy()
                    assert np.isfinite(got).all() and np.isfinite(got_u8).all()
                    err = max(float(np.abs(got - want[:B]).max()), float(np.abs(got_u8 - want_u8[:B]).max()))
                    print(f"ENVELOPE {tag} B={B} {arm}: max|score - reference| {err:.3e} (bound {ARM_TOL[arm]:.0e})")
                    worst[arm] = max(worst.get(arm, 0.0), err)
            if precision == "fp16":   # determinism and batch-split invariance
                a = n.score_images(pxd, txt).clone()
                b = n.score_images(pxd, txt).clone()
                parts = torch.cat([n.score_images(pxd[:1], txt).clone(), n.score_images(pxd[1:], txt).clone()])
                assert torch.equal(a, b) and torch.equal(a, parts)
                assert n.saturation_count() == 0
            assert n.kernel_faults == 0
        finally:
            n.close()
    return worst


@pytest.mark.parametrize("name", TOWERS)
def test_envelope_towers_against_the_c_oracle(name):
    worst = _tower_arms(name, *_reference(name))
    for arm, err in worst.items():
        assert err < ARM_TOL[arm], (name, arm, err)


def test_envelope_tower_exact_gelu_against_hf_on_the_cpu():
    """The C oracle computes QuickGELU only: the 384-wide geometry with the exact GELU in both towers against HF CLIPModel
    (fp32, CPU), same arms and bounds."""
    from mcm_amd.weights import synth_state_dict
    from oracle.hf_reference import HFReference

    geo0, _, ids, mask, px, u8, _, _ = _reference("w384")
    geo = dataclasses.replace(geo0, name="w384-gelu", v_hidden_act="gelu", t_hidden_act="gelu")
    sd = synth_state_dict(geo, 0)
    hf = HFReference(geo, sd, device="cpu")
    assert hf.model.config.vision_config.hidden_act == "gelu" and hf.model.config.text_config.hidden_act == "gelu"
    hf.set_bank(ids.copy(), mask.copy())
    want = hf.score_batch(torch.tensor(px)).numpy()
    want_u8 = hf.score_batch(torch.from_numpy(eb.u8_normalise(u8))).numpy()
    worst = _tower_arms("w384-gelu", geo, sd, ids, mask, px, u8, want, want_u8)
    for arm, err in worst.items():
        assert err < ARM_TOL[arm], (arm, err)


def test_320_wide_with_4_and_with_5_heads_are_told_apart():
    """The same weights read as 4 heads of 80 and as 5 heads of 64: each matches the oracle of its own head count (fp32 arm,
    2e-6 on the score, 1e-6 on a unit-norm feature) and the two differ."""
    from mcm_amd.engine import NativeCLIP
    from oracle import oracle as orc

    g5, sd, ids, mask, px, _, _, _ = _reference("w320-h5x64")
    g4 = dataclasses.replace(g5, name="w320-h4x80", v_heads=4)
    assert ge.accepted(g4) is None
    feats = {}
    for geo in (g5, g4):
        o = orc.OracleCLIP(geo, sd)
        n = NativeCLIP(geo, sd, precision="fp32", max_batch=8, max_prompt_tokens=1024)
        try:
            got = n.get_image_features(torch.tensor(px).cuda(), normalize=True).cpu().numpy()
            assert n.kernel_faults == 0
        finally:
            n.close()
        d = float(np.abs(got - o.encode_image(px)).max())
        print(f"ENVELOPE {geo.name}: max|image feature - oracle| {d:.3e}")
        assert d < 1e-6, (geo.name, d)
        feats[geo.v_heads] = got
    assert np.abs(feats[4] - feats[5]).max() > 1e-3


# ---- the text tower at other lengths than 77 ----------------------------------------------------------------------------------
TEXT_FEATURE_TOL = 1e-6      # tests/test_geometry_envelope_cpu.py: two fp32 implementations of a 2-layer tower, unit-norm rows


@pytest.mark.parametrize("name", ge.TEXT_ONLY)
def test_text_tower_at_other_position_counts_against_the_oracle(name):
    """max_positions 32, 248 (Long-CLIP) and the last value mcm_create accepts: sequence lengths 1, 77, 78, max - 1 and max,
    prompts that fill the row and prompts that end early; one token more is MCM_ERANGE with nothing launched."""
    from mcm_amd.abi import DEFINES
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict
    from oracle import oracle as orc

    geo = ge.ENVELOPE[name]
    assert ge.accepted(geo, max_prompt_tokens=4096) is None
    sd = synth_state_dict(geo, 0)
    o = orc.OracleCLIP(geo, sd)
    n = NativeCLIP(geo, sd, precision="fp16", max_batch=8, max_prompt_tokens=4096)
    try:
        for S in ge.prompt_lengths(geo.max_positions):
            ids = ge.prompts(6, S, seed=S)
            got = n.get_text_features(input_ids=torch.from_numpy(ids), normalize=True).cpu().numpy()
            d = float(np.abs(got - o.encode_text(ids)).max())
            print(f"ENVELOPE {name} S={S}: max|text feature - oracle| {d:.3e}")
            assert np.isfinite(got).all() and d < TEXT_FEATURE_TOL, (S, d)
        S = geo.max_positions + 1
        ids = ge.prompts(2, S, seed=0)
        out = torch.full((2, geo.proj_dim), 7.0, device="cuda")
        rc = n._lib.mcm_encode_text_ex(n._h, ids.ctypes.data_as(ctypes.c_void_p), 2, S, 1, out.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == DEFINES["MCM_ERANGE"] and b"max_position_embeddings" in n._lib.mcm_last_error(n._h)
        assert bool((out == 7.0).all())
        assert n.kernel_faults == 0
    finally:
        n.close()


# ---- one step outside the envelope ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,kw", ge.REFUSED, ids=[g.name for g, _ in ge.REFUSED])
def test_create_refuses_one_step_outside_the_envelope(geo, kw):
    """mcm_create returns MCM_EINVAL with a message naming the rule, before it touches the device's memory."""
    from mcm_amd.config import CConfig  # noqa: F401  (the struct to_c fills)
    from mcm_amd.engine import load_library

    words = ge.accepted(geo, **kw)
    assert words is not None
    lib = load_library(False)
    cfg = geo.to_c(max_batch=8, max_prompt_tokens=kw.get("max_prompt_tokens", 1024))
    h = ctypes.c_void_p()
    rc = lib.mcm_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -1 and not h.value, (geo.name, rc)
    assert words.encode() in lib.mcm_last_error(None), (words, lib.mcm_last_error(None))
