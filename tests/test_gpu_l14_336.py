"""ViT-L/14@336px (577 vision tokens: every attention launch of the vision tower on the streaming kernels) end to end, with
seeded weights in the fp16-exact regime (the situation of the real checkpoint): a 2-layer tower against the C oracle in the
three operand modes, the full 24-layer tower against HF CLIPModel (fp32, eager) and the split-activation arm against the
exact-fp32 arm, uint8 ingest with the device Resize(336) + CenterCrop(336), and one small CLI run with threshold refinement."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CKPT = "ViT-L/14@336px"
MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)
STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _cos(a, b):
    return np.sum(_unit(a) * _unit(b), axis=-1)


def _net(geo, sd, precision, max_batch, **kw):
    from mcm_amd.engine import NativeCLIP

    return NativeCLIP(geo, sd, precision=precision, max_batch=max_batch, max_prompt_tokens=100 * 16, **kw)


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_two_layer_tower_vs_oracle(precision):
    """Image features of a 2-layer L/14@336px tower against the fp32 C oracle on 2 images (the cosine bar of
    tests/test_gpu_model.py::test_other_checkpoints_vs_oracle; the fp32 arm to the oracle's round-off)."""
    from mcm_amd.config import geometry
    from mcm_amd.synth import make_pixels
    from mcm_amd.weights import synth_state_dict
    from oracle import oracle as orc

    geo = dataclasses.replace(geometry(CKPT), name="L14-336-2L", v_layers=2, t_layers=2)
    sd = synth_state_dict(geo, 0, "fp16-exact")
    px, _ = make_pixels(2, geo.image_size, 10, ood=False, seed=4)
    want = orc.OracleCLIP(geo, sd).encode_image(px)
    net = _net(geo, sd, precision, 4)
    try:
        got = net.get_image_features(pixel_values=torch.from_numpy(px).cuda()).cpu().numpy()
    finally:
        net.close()
    assert got.shape == (2, geo.proj_dim) and np.isfinite(got).all()
    cos = _cos(got, want)
    print(f"L/14@336px 2 layers {precision}: min cos vs oracle {cos.min():.9f}, "
          f"max|d| of the unit features {np.abs(_unit(got) - _unit(want)).max():.2e}")
    assert cos.min() > 0.999
    if precision == "fp32":
        np.testing.assert_allclose(_unit(got), _unit(want), rtol=0, atol=2e-6)


@pytest.fixture(scope="module")
def full_tower():
    from mcm_amd.config import geometry
    from mcm_amd.synth import make_token_ids
    from mcm_amd.weights import synth_state_dict

    geo = geometry(CKPT)
    sd = synth_state_dict(geo, 0, "fp16-exact")
    ids, mask = make_token_ids(100, seed=2)
    return geo, sd, ids, mask


def test_full_tower_vs_hf_and_the_split_arm(full_tower):
    """24 layers, 32 images, K = 100 prompts: the exact-fp32 arm scores what HF CLIPModel scores (fp32 eager, same weights and
    pixels); the split-activation arm of an fp16 handle equals the fp32 arm to fp32 round-off and is >= 10 x closer to it
    than the fp16 arm (tests/test_gpu_x2.py's bar); no fp16 activation saturated."""
    from oracle.hf_reference import HFReference

    geo, sd, ids, mask = full_tower
    B = 32
    g = torch.Generator(device="cuda").manual_seed(7)
    px = torch.randn((B, 3, geo.image_size, geo.image_size), device="cuda", generator=g)
    n32 = _net(geo, sd, "fp32", B)
    try:
        bank = n32.get_text_features(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), normalize=True)
        s32 = n32.score_images(px, bank).double()
    finally:
        n32.close()
    n16 = _net(geo, sd, "fp16", B)
    try:
        s16 = n16.score_images(px, bank).double()
        sx2 = n16.score_images_x2(px, bank).double()
        assert n16.saturation_count() == 0
    finally:
        n16.close()
    hf = HFReference(geo, sd, device="cuda")
    hf.set_bank(ids, mask)
    shf = hf.score_batch(px).double()
    del hf
    torch.cuda.empty_cache()
    d_hf = (s32 - shf).abs()
    d16, d2 = float((s16 - s32).abs().max()), float((sx2 - s32).abs().max())
    print(f"L/14@336px: |fp32 arm - HF| max {float(d_hf.max()):.2e} rms {float(d_hf.pow(2).mean().sqrt()):.2e}; "
          f"|d score| fp16 arm {d16:.2e}, split-activation arm {d2:.2e} (scores ~ {float(s32.abs().mean()):.3e})")
    # a few fp32 ulps of the scores (~1e-2 at K = 100; B/16 at K = 1000: scores ~1e-3, rms <= 1e-9 in test_gpu_headline_parity)
    ulp = float(np.spacing(np.float32(shf.abs().max().item())))
    assert float(d_hf.pow(2).mean().sqrt()) <= 2 * ulp and float(d_hf.max()) <= 4 * ulp, ulp
    assert d2 <= 2e-9 and d2 <= 0.1 * d16, (d2, d16)


def test_uint8_ingest_at_336(full_tower):
    """Odd-sized uint8 images through the device Resize(336) + CenterCrop(336) (mcm_resize_crop_u8) and the fused
    ToTensor / Normalize: the crops are the oracle's, and the scores those of the float route on the same crops."""
    geo, sd, ids, mask = full_tower
    rng = np.random.default_rng(11)
    imgs = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in
            ((337, 500), (480, 341), (999, 777), (336, 336), (211, 403))]
    net = _net(geo, sd, "fp32", 8)
    try:
        bank = net.get_text_features(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), normalize=True)
        u8 = net.resize_crop(imgs)
        assert tuple(u8.shape) == (5, 336, 336, 3)
        from oracle import oracle as orc

        for im, crop in zip(imgs, u8.cpu().numpy()):   # the crops themselves: Pillow's bytes (the oracle's, bit for bit)
            np.testing.assert_array_equal(crop, orc.resize_crop_u8(im.numpy(), 336), err_msg=str(tuple(im.shape)))
        f32 = ((u8.cpu().numpy().astype(np.float32) / np.float32(255.0) - MEAN) / STD).transpose(0, 3, 1, 2).copy()
        s_u8 = net.score_images(u8, bank).double()
        s_f = net.score_images(torch.from_numpy(f32).cuda(), bank).double()
    finally:
        net.close()
    d = float((s_u8 - s_f).abs().max())
    print(f"L/14@336px uint8 vs float route: max|d score| {d:.2e}")
    assert d <= 2e-9, d


def test_cli_l14_336_refined_fpr95_equals_the_fp32_arm(tmp_path, monkeypatch):
    """`--CLIP_ckpt ViT-L/14@336px --synthetic` on a few hundred images: the CSV is written and the fp16 run's refined FPR95
    (`--refine-threshold exact`) is the exact-fp32 run's."""
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    common = ["--in_dataset", "ImageNet10", "--CLIP_ckpt", CKPT, "--synthetic", "--synthetic-n", "200", "-b", "64"]
    r32 = cli.main(common + ["--dtype", "fp32", "--name", "l336_fp32"])
    r16 = cli.main(common + ["--dtype", "fp16", "--refine-threshold", "exact", "--name", "l336_fp16"])
    assert r16["refine"]["rescored_total"] > 0
    for k in r32["measures"]:
        assert r16["measures"][k][2] == r32["measures"][k][2], (k, r16["measures"][k], r32["measures"][k])
    csv = tmp_path / "results/ImageNet10/MCM/CLIP_ViT-L/14@336px_T_1_ID_l336_fp16/l336_fp16.csv"
    assert csv.exists(), list(tmp_path.rglob("*.csv"))
