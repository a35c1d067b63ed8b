"""Both ends of the towers against fp64 references under the derived budgets of tests/error_budget.py (proved to
discriminate on the CPU by tests/test_error_budget.py):
  * the vision front through mcm_debug_vision_front (harness library; the function mcm_encode_image* itself runs): the patch
    embedding (patchify / patchify8 / the split and uint8 gathers, the EPI_PATCH epilogue of the tile kernel and of the
    persistent kernel, plain and pixel-gathering) and the fused CLS row + pre_layrnorm + layer 0 layer_norm1 pass, at every
    geometry, operand mode, pixel format, small batches on every element and full-size batches on sampled rows;
  * the uint8 normalise, bit for bit against numpy float32 on all 256 x 3 (value, channel) pairs;
  * pool_project_kernel (mcm_debug_op_pool_project), text_embed_kernel (mcm_debug_op_text_embed, bit for bit) and
    bank_reduce_kernel (mcm_reduce_bank).

Each budget check prints "BUDGET <family> <mode> <worst max|got - ref| / budget>" (run with -s to collect them)."""
import ctypes
import functools
import dataclasses

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTYPE = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
F32_NCHW, U8_NHWC = 0, 1
EINVAL = -1
PRE = "vision_model."


_ptr = gs.ptr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_check = functools.partial(gs.check_budget, finite_budget=True)


# ---- handles -----------------------------------------------------------------------------------------------------------
def _geo(name):
    """The named geometry; the full checkpoints with one encoder layer per tower (the front and the pooling kernels do not
    depend on the layers behind them, and a handle is then created in a fraction of the time).  A ClipGeometry is taken as
    it is (tests/test_gpu_geometry_envelope.py)."""
    from mcm_amd.config import CHECKPOINTS, ClipGeometry, geometry

    if isinstance(name, ClipGeometry):
        return name
    geo = geometry(name)
    return dataclasses.replace(geo, name=name + "-1L", v_layers=1, t_layers=1) if name in CHECKPOINTS else geo


class Front:
    """A harness handle and the fp32 masters its front reads."""

    def __init__(self, name, precision, max_batch, regime="fp16-exact", weight_operands="auto", x2_max_batch=None):
        from mcm_amd.engine import NativeCLIP
        from mcm_amd.weights import synth_state_dict

        self.geo = geo = _geo(name)
        sd = synth_state_dict(geo, 0, regime)
        self.precision = precision
        self.net = NativeCLIP(geo, sd, precision=precision, max_batch=max_batch, max_prompt_tokens=256, harness=True,
                              weight_operands=weight_operands, x2_max_batch=x2_max_batch)
        self.P, self.np, self.ntok, self.D = geo.patch_size, geo.n_patches, geo.v_tokens, geo.v_width
        kreal = 3 * self.P * self.P
        kalign = 128 // (4 if precision == "fp32" else 2)
        self.kpad = (kreal + kalign - 1) // kalign * kalign
        w = np.zeros((self.D, self.kpad), np.float32)
        w[:, :kreal] = sd[PRE + "embeddings.patch_embedding.weight"].reshape(self.D, kreal)
        self.w = eb.weight_values(w, precision, self.net.split_weights)
        self.pos = sd[PRE + "embeddings.position_embedding.weight"]
        self.cls = sd[PRE + "embeddings.class_embedding"]
        self.g0, self.b0 = sd[PRE + "pre_layrnorm.weight"], sd[PRE + "pre_layrnorm.bias"]
        self.g1, self.b1 = (sd[PRE + "encoder.layers.0.layer_norm1." + k] for k in ("weight", "bias"))

    def close(self):
        self.net.close()

    def run(self, px, x2, stage, poison=0):
        """mcm_debug_vision_front on device pixels (fp32 NCHW or uint8 NHWC): (residual rows, operand rows or None)."""
        B = px.shape[0]
        rows = B * self.ntok
        resid = torch.empty((rows, self.D), device="cuda", dtype=torch.float32)
        ln = None
        if stage == 1:
            ln = torch.empty((rows, 2 * self.D if x2 else self.D), device="cuda", dtype=DTYPE[self.precision])
        net = self.net
        rc = net._lib.mcm_debug_vision_front(net._h, _ptr(px), U8_NHWC if px.dtype == torch.uint8 else F32_NCHW, int(x2), B,
                                             stage, poison, _ptr(resid), _ptr(ln), None)
        assert rc == 0, net._lib.mcm_last_error(net._h)
        torch.cuda.synchronize()
        return resid, ln

    def patchify_launches(self, px):
        """patchify launches of one stage-0 call (0: the patch GEMM gathered the pixels itself)."""
        self.net.profile(True)
        self.net.profile_read()
        self.run(px, False, 0)
        n = self.net.profile_read()["patchify"]["launches"]
        self.net.profile(False)
        return n


def _patch_rows(px, P, rows):
    """Rows of the patch matrix of device fp32 NCHW pixels (data movement only), on the host."""
    B, C, S, _ = px.shape
    g = S // P
    m = px.reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P)
    return m[torch.from_numpy(rows).cuda()].cpu().numpy()


def _front_check(f, px32, px_in, x2, tag, rows=None, poison=0, stages=(0, 1)):
    """px32: the fp32 NCHW pixels the operand is rounded from (device); px_in: what the entry point is given (px32, or the
    uint8 image px32 was computed from).  rows: patch-matrix rows to check (all by default; the CLS rows are always checked).
    Returns the stage-0 residual rows."""
    mode = "x2" if x2 else f.precision
    B = px32.shape[0]
    rows = np.arange(B * f.np) if rows is None else rows
    trow = eb.token_rows(B, f.np, rows)
    crow = np.arange(B) * f.ntok
    r0, _ = f.run(px_in, x2, 0, poison)
    pm = np.zeros((len(rows), f.kpad), np.float32)
    pm[:, :3 * f.P * f.P] = _patch_rows(px32, f.P, rows)
    ref, bud = eb.patch_embed_budget(eb.operand_values(pm, f.precision, x2), f.w, f.pos, f.np, rows)
    tr = torch.from_numpy(trow).cuda()
    _check("patch-u8" if px_in.dtype == torch.uint8 else "patch", mode, r0[tr].cpu().numpy(), ref, bud, tag)
    if 1 not in stages:
        return r0
    r1, ln = f.run(px_in, x2, 1, poison)
    allr = np.concatenate([crow, trow])
    ar = torch.from_numpy(allr).cuda()
    x0 = np.concatenate([np.broadcast_to(eb.cls_row(f.cls, f.pos), (B, f.D)), r0[tr].cpu().numpy()])
    x1 = r1[ar].cpu().numpy()
    assert np.isfinite(x1).all(), f"{tag}: a non-finite residual row"
    (ref0, bud0), (ref1, bud1) = eb.pre_ln_budgets(x0, x1, f.g0, f.b0, f.g1, f.b1, f.precision, x2)
    _check("pre-ln", mode, x1, ref0, bud0, tag)
    got = ln[ar]
    got = eb.merge_image(got.cpu().numpy()) if x2 else got.float().cpu().numpy()
    assert np.isfinite(got).all(), f"{tag}: a non-finite operand row"
    _check("ln1", mode, got, ref1, bud1, tag)
    assert np.abs(ref1).max() + bud1.max() < eb.FP16_MAX
    assert f.net.saturation_count() == 0
    return r0


def _pixels(B, S, seed, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    px = torch.randn((B, 3, S, S), generator=g, device=device) * 1.2
    px[:, :, ::7, ::5] *= 2.0 ** -9       # small pixels next to large ones
    return px


def _u8(B, S, seed):
    u8 = np.random.default_rng(seed).integers(0, 256, size=(B, S, S, 3), dtype=np.uint8)
    u8.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]     # every (value, channel) pair
    return u8


# ---- vision front, small: every element --------------------------------------------------------------------------------
SMALL = ["tiny", "B16-2L", "ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px"]
# batches: 1, 3 and one whose patch rows pass a 256-row tile (at 196 patches and up that is batch 2; 3 is past it as well)
BIG = {"tiny": 17, "B16-2L": 2, "ViT-B/32": 6, "ViT-B/16": 2, "ViT-L/14": 2, "ViT-L/14@336px": 2}


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", SMALL)
def test_vision_front_small_within_budget(name, precision):
    """Every element of stage 0 and stage 1, fp32 and uint8 pixels, batches 1, 3 and one past a 256-row tile; the fp16 handle
    also runs the split-activation arm.  fp16-valued masters: one fp16 operand per weight in fp16 mode, split weights in
    bf16 mode.  L/14 (padded K) runs with the workspace poisoned as well."""
    batches = sorted({1, 3, BIG[name]})
    f = Front(name, precision, max_batch=max(batches), x2_max_batch=max(batches) if precision == "fp16" else None)
    try:
        assert f.net.split_weights == (precision == "bf16")
        S = f.geo.image_size
        assert max(batches) * f.np > 256
        for B in batches:
            for x2 in ((False, True) if precision == "fp16" else (False,)):
                tag = f"{name} B={B}"
                px = _pixels(B, S, seed=B + 10 * len(name))
                r0 = _front_check(f, px, px, x2, tag)
                u8 = _u8(B, S, seed=B)
                pu = _dev(eb.u8_normalise(u8))
                ru = _front_check(f, pu, _dev(u8), x2, tag + " u8")
                if precision == "fp32":   # the fused normalise is numpy's float32 arithmetic, bit for bit
                    rf, _ = f.run(pu, False, 0)
                    t = torch.from_numpy(eb.token_rows(B, f.np)).cuda()
                    assert torch.equal(ru[t], rf[t]), f"{tag}: uint8 normalise differs from numpy float32"
                if "L/14" in name:
                    _front_check(f, px, px, x2, tag + " poisoned", poison=1)
                    _front_check(f, pu, _dev(u8), x2, tag + " u8 poisoned", poison=1)
                del r0
    finally:
        f.close()


@pytest.mark.parametrize("precision,regime,operands,split", [("fp16", "fp32", "auto", True), ("bf16", "fp16-exact", "single", False),
                                                             ("fp16", "fp32", "single", False)])
def test_vision_front_other_weight_forms_within_budget(precision, regime, operands, split):
    """The weight forms the test above does not meet: split fp16 weights (fp32-valued masters), single rounded bf16 / fp16."""
    f = Front("tiny", precision, max_batch=17, regime=regime, weight_operands=operands)
    try:
        assert f.net.split_weights == split
        for B in (3, 17):
            for x2 in ((False, True) if precision == "fp16" else (False,)):
                px = _pixels(B, 64, seed=B)
                _front_check(f, px, px, x2, f"tiny {regime} {operands} B={B}")
    finally:
        f.close()


# ---- vision front, full size: sampled rows -----------------------------------------------------------------------------
# (geometry, batch, the patch GEMM gathers pixels itself at that batch)
FULL = [("ViT-B/16", 512, True), ("ViT-B/32", 512, True), ("ViT-L/14", 256, False)]


@pytest.fixture(scope="module", params=[(n, p) for n, _, _ in FULL for p in ("fp16", "bf16")],
                ids=[f"{n}-{p}" for n, _, _ in FULL for p in ("fp16", "bf16")])
def full_front(request):
    name, precision = request.param
    B = dict((n, b) for n, b, _ in FULL)[name]
    f = Front(name, precision, max_batch=B, x2_max_batch=32 if precision == "fp16" else None)
    yield f
    f.close()


def _full_rows(B, n_patches):
    """sample_rows of the patch matrix plus every image's first patch row (the CLS rows are always checked)."""
    return eb.sample_rows(B * n_patches, np.arange(B) * n_patches)


def test_vision_front_full_size_within_budget(full_front):
    """B/16 and B/32 at batch 512, L/14 at 256: each route held to fp64 on its own (B/16: the pixel-gathering GEMM and the
    patchify route, mcm_debug_patch_fold 1 and 0), one batch on each side of the batch where the pixel-gathering route starts
    (found by bisection on the patchify launch count: the size policy of gemm.hip puts it where the persistent kernel's tiles
    pass half the CUs, batch 55 at B/16 and 220 at B/32 on a 256-CU part), uint8 pixels, and the split-activation arm at its
    batch."""
    f = full_front
    name, B, gathers = next(x for x in FULL if f.geo.name == x[0] + "-1L")
    S = f.geo.image_size
    lib = f.net._lib
    px = _pixels(B, S, seed=B)
    try:
        for fold in ((1, 0) if name == "ViT-B/16" else (1,)):
            assert lib.mcm_debug_patch_fold(fold) == 0
            assert f.patchify_launches(px) == (0 if fold and gathers else 1)
            _front_check(f, px, px, False, f"{name} B={B} fold={fold}", rows=_full_rows(B, f.np))
        assert lib.mcm_debug_patch_fold(1) == 0
        if gathers:
            lo, hi = 1, B                      # patchify runs at lo, not at hi
            assert f.patchify_launches(px[:lo]) == 1
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if f.patchify_launches(px[:mid]) else (lo, mid)
            print(f"EDGE {name} {f.precision}: the patch GEMM gathers pixels from batch {hi} on")
            for b in (lo, hi):
                _front_check(f, px[:b], px[:b], False, f"{name} B={b}", rows=_full_rows(b, f.np))
        nb = 64
        u8 = _u8(nb, S, seed=5)
        _front_check(f, _dev(eb.u8_normalise(u8)), _dev(u8), False, f"{name} B={nb} u8", rows=_full_rows(nb, f.np))
        if f.precision == "fp16":
            _front_check(f, px[:32], px[:32], True, f"{name} B=32", rows=_full_rows(32, f.np))
    finally:
        lib.mcm_debug_patch_fold(1)
    assert f.net.kernel_faults == 0


# ---- uint8 normalise, exactly ------------------------------------------------------------------------------------------
def test_uint8_normalise_is_numpy_float32_bit_for_bit():
    """All 256 x 3 (value, channel) pairs through patchify_u8_kernel in fp32 mode, read back through a patch GEMM whose weight
    picks single operand columns (an identity block: the row's dot product is the operand itself, position rows zero)."""
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = _geo("tiny")
    sd = synth_state_dict(geo, 0)
    D, P = geo.v_width, geo.patch_size
    K = 3 * P * P
    cols = [c * P * P + j for c in range(3) for j in range(D // 3)]     # D // 3 pixels of patch row 0 per channel
    w = np.zeros((D, K), np.float32)
    w[np.arange(len(cols)), cols] = 1.0
    sd[PRE + "embeddings.patch_embedding.weight"] = w.reshape(D, 3, P, P)
    sd[PRE + "embeddings.position_embedding.weight"] = np.zeros_like(sd[PRE + "embeddings.position_embedding.weight"])
    net = NativeCLIP(geo, sd, precision="fp32", max_batch=8, max_prompt_tokens=256, harness=True)
    try:
        n = D // 3
        B = -(-256 // n)
        S = geo.image_size
        u8 = np.zeros((B, S, S, 3), np.uint8)
        for v in range(256):   # value v in all three channels of pixel j = v % n of patch 0 of image v // n: k = c P P + j
            u8[v // n, (v % n) // P, (v % n) % P, :] = v
        resid = torch.empty((B * geo.v_tokens, D), device="cuda", dtype=torch.float32)
        u8_d = _dev(u8)
        rc = net._lib.mcm_debug_vision_front(net._h, _ptr(u8_d), U8_NHWC, 0, B, 0, 1, _ptr(resid), None, None)
        assert rc == 0, net._lib.mcm_last_error(net._h)
        torch.cuda.synchronize()
        got = resid[torch.arange(B, device="cuda") * geo.v_tokens + 1][:, :3 * n].cpu().numpy().reshape(B, 3, n)
        j = np.arange(n)
        want = eb.u8_normalise(u8)[:, :, j // P, j % P]
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), f"{int(bad.sum())} of 768 (value, channel) pairs differ, e.g. {got[bad][:4]} != {want[bad][:4]}"
    finally:
        net.close()


# ---- pool_project ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_harness():
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = _geo("tiny")
    net = NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=8, max_prompt_tokens=256, harness=True)
    yield net
    net.close()


def _pool_rows(n, D, seed):
    """Gaussian rows; mean 1e3 with spread 1e-2; constant; one 2^12 outlier; magnitudes 2^-12 ... 2^8 — in turn."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) * 2 + 0.5).astype(np.float32)
    kind = np.arange(n) % 5
    x[kind == 1] = (1e3 + 1e-2 * rng.standard_normal((int((kind == 1).sum()), D))).astype(np.float32)
    x[kind == 2] = np.float32(0.1) * (1 + np.arange(int((kind == 2).sum()), dtype=np.float32))[:, None]
    x[kind == 3, 5 % D] = 4096.0
    x[kind == 4] *= (2.0 ** (-12 + np.arange(int((kind == 4).sum())) % 21)).astype(np.float32)[:, None]
    return x


def _pool(net, x, idx, stride, n, D, g, b, proj, P, normalize, eps=1e-5):
    """x [rows, D] on the device; idx: host int32 row indices, or None for rows i * stride."""
    out = torch.full((n, P), float("nan"), device="cuda")
    ip = idx.ctypes.data_as(ctypes.c_void_p) if idx is not None else None
    rc = net._lib.mcm_debug_op_pool_project(net._h, _ptr(x), x.shape[0], ip, stride, n, D, _ptr(g), _ptr(b), eps, _ptr(proj),
                                            P, _ptr(out), int(normalize), None)
    if rc == 0:
        torch.cuda.synchronize()
    return rc, out


def _pool_params(D, P, seed):
    rng = np.random.default_rng(seed)
    g = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    proj = (rng.standard_normal((P, D)) * D ** -0.5).astype(np.float32)
    return g, b, proj


POOL_D = [64, 320, 512, 768, 1020, 1024]
POOL_P = [1, 17, 64, 512, 768, 1024]


@pytest.mark.parametrize("D", POOL_D)
def test_pool_project_within_budget(tiny_harness, D):
    """Every P with this D; n = 1, 5, 1000; pooling by stride (50, 197, 257, 577: the towers' CLS strides) and by index
    (unsorted, repeated, first and last row); raw and normalised."""
    net = tiny_harness
    for j, P in enumerate(POOL_P):
        g, b, proj = _pool_params(D, P, D + P)
        gd, bd, pd = _dev(g), _dev(b), _dev(proj)
        cases = [(1, 50), (5, (197, 257, 577)[j % 3]), (1000, 50), (5, None), (1000, None)] if j % 2 == 0 else \
                [(5, (577, 197, 257)[j % 3]), (1, None), (1000, None)]
        for n, stride in cases:
            rng = np.random.default_rng(n + D + P)
            if stride is not None:
                pooled = _pool_rows(n, D, seed=n + D)
                x = rng.standard_normal((n * stride, D)).astype(np.float32)   # the other rows must not matter
                x[::stride] = pooled
                idx = None
            else:
                rows = max(n, 7) * 3
                x = _pool_rows(rows, D, seed=n + D + 1)
                idx = rng.integers(0, rows, size=n).astype(np.int32)
                idx[0] = rows - 1
                if n > 1:
                    idx[-1] = 0
                if n > 4:
                    idx[2] = idx[1]
                pooled = x[idx]
            xd = _dev(x)
            for normalize in (0, 1):
                rc, out = _pool(net, xd, idx, stride or 0, n, D, gd, bd, pd, P, normalize)
                assert rc == 0, net._lib.mcm_last_error(net._h)
                ref, bud = eb.pool_project_budget(pooled, g, b, proj, bool(normalize))
                _check("pool" if normalize else "pool-raw", "fp32", out.cpu().numpy(), ref, bud,
                       f"D={D} P={P} n={n} stride={stride}")


def test_pool_project_refuses_bad_shapes_and_pins_the_zero_norm(tiny_harness):
    """D = 1028, D = 1022 and P = 1025 are refused by launch_pool_project's own guard (the entry point maps its
    hipErrorInvalidValue to MCM_EINVAL and checks only the row indices itself)."""
    net = tiny_harness
    x = torch.randn((4, 1028), device="cuda")
    for D, P in ((1028, 64), (1022, 64), (64, 1025)):
        g, b, proj = (torch.ones(D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros((P, D), device="cuda"))
        rc, _ = _pool(net, x, None, 1, 2, D, g, b, proj, P, 1)
        assert rc == EINVAL, (D, P, rc)
    g, b, proj = (torch.ones(64, device="cuda"), torch.zeros(64, device="cuda"), torch.zeros((64, 64), device="cuda"))
    assert _pool(net, x, np.array([0, 4], np.int32), 0, 2, 64, g, b, proj, 64, 1)[0] == EINVAL    # a row outside x
    assert _pool(net, x, None, 4, 2, 64, g, b, proj, 64, 1)[0] == EINVAL
    # gamma = beta = 0: every output is 0, its norm 0 — the normalised row is 0 * inf, non-finite as the reference's
    # x / x.norm() is (the one case without a finite budget); the raw row is exactly 0
    D, P = 512, 64
    xd = _dev(_pool_rows(5, D, 1))
    z = torch.zeros(D, device="cuda")
    proj = torch.randn((P, D), device="cuda")
    rc, raw = _pool(net, xd, None, 1, 5, D, z, z, proj, P, 0)
    assert rc == 0 and (raw == 0).all()
    rc, nrm = _pool(net, xd, None, 1, 5, D, z, z, proj, P, 1)
    assert rc == 0 and not torch.isfinite(nrm).any()
    _, bud = eb.pool_project_budget(xd.cpu().numpy(), np.zeros(D, np.float32), np.zeros(D, np.float32), proj.cpu().numpy(), True)
    assert np.isinf(bud).all()


# ---- text_embed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,S,K,V", [(64, 77, 3, 1000), (512, 16, 65, 49408), (768, 1, 130, 5000), (512, 77, 1000, 49408),
                                     (768, 77, 7, 49408)])
def test_text_embed_is_one_fp32_add_bit_for_bit(tiny_harness, D, S, K, V):
    net = tiny_harness
    rng = np.random.default_rng(D + S + K)
    tok = (0.5 * rng.standard_normal((V, D))).astype(np.float32)
    pos = (0.1 * rng.standard_normal((77, D))).astype(np.float32)
    ids = rng.integers(0, V, size=(K, S)).astype(np.int32)
    ids.flat[0], ids.flat[-1] = 0, V - 1
    ids.flat[1:3] = V - 1                       # repeats
    if K > 2:
        ids[1] = ids[0]
    x = torch.full((K * S, D), float("nan"), device="cuda")
    tok_d, pos_d = _dev(tok), _dev(pos)
    rc = net._lib.mcm_debug_op_text_embed(net._h, ids.ctypes.data_as(ctypes.c_void_p), V, _ptr(tok_d), _ptr(pos_d), _ptr(x),
                                          K, S, D, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    want = tok[ids.reshape(-1)] + np.tile(pos[:S], (K, 1))
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_text_embed_refuses_a_width_that_is_no_multiple_of_4(tiny_harness):
    """D = 6 is refused by launch_text_embed's own guard (mapped to MCM_EINVAL); the id range check is the entry point's."""
    net = tiny_harness
    t = torch.zeros(64, device="cuda")
    ids = np.zeros(4, np.int32)
    ip = ids.ctypes.data_as(ctypes.c_void_p)
    assert net._lib.mcm_debug_op_text_embed(net._h, ip, 4, _ptr(t), _ptr(t), _ptr(t), 1, 1, 6, None) == EINVAL
    ids[2] = 4                                    # an id outside the table is refused, nothing launched
    assert net._lib.mcm_debug_op_text_embed(net._h, ip, 4, _ptr(t), _ptr(t), _ptr(t), 1, 4, 4, None) == EINVAL


# ---- bank_reduce -------------------------------------------------------------------------------------------------------
def _bank_rows(K, T, P, seed):
    """Unit template rows [K T, P], class-major.  With T > 1 the templates of class 0 nearly cancel: T directions evenly round
    a circle sum to 0; a common offset of 1e-3 is what is left of their mean."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((K, T, P))
    if T > 1:
        u, v, z = np.linalg.qr(rng.standard_normal((P, 3)))[0].T
        ang = 2 * np.pi * np.arange(T) / T
        f[0] = np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v + 1e-3 * z
    return (f / np.linalg.norm(f, axis=2, keepdims=True)).astype(np.float32).reshape(K * T, P)


@pytest.mark.parametrize("P", [64, 512, 768])
def test_bank_reduce_within_budget(P):
    """Unit template rows; class 0's templates nearly cancel (mean of norm ~ 1e-3): the budget scales with 1 / ||mean||."""
    net = gs.widened_net(P)
    try:
        for K in (1, 3, 1000, 1001):
            for T in (1, 7, 80):
                f = _bank_rows(K, T, P, K + T + P)
                got = net.reduce_bank(_dev(f), K, T).cpu().numpy()
                ref, bud = eb.bank_reduce_budget(f, K, T)
                if T > 1:
                    assert 2e-4 < np.linalg.norm(f.reshape(K, T, P)[0].astype(np.float64).mean(axis=0)) < 5e-3
                _check("bank", "fp32", got, ref, bud, f"P={P} K={K} T={T}")
    finally:
        net.close()
