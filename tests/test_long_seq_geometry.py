"""ViT-L/14@336px (openai/clip-vit-large-patch14-336) as a fourth checkpoint name: its geometry, hub id, HF config, the CLI
choice and its full-round batches (CPU only)."""
import pytest

from mcm_amd.config import CHECKPOINTS, HUB_IDS, geometry


def test_geometry_of_l14_336():
    g = geometry("ViT-L/14@336px")
    assert (g.image_size, g.patch_size) == (336, 14)
    assert (g.v_width, g.v_heads, g.v_layers, g.v_mlp) == (1024, 16, 24, 4096)
    assert (g.t_width, g.t_heads, g.t_layers, g.t_mlp) == (768, 12, 12, 3072)
    assert g.proj_dim == 768 and g.max_positions == 77 and g.vocab_size == 49408
    assert g.n_patches == 576 and g.v_tokens == 577
    # the same towers as ViT-L/14, only the image size differs
    l14 = geometry("ViT-L/14")
    assert {k: v for k, v in vars(g).items() if k not in ("name", "image_size")} == \
        {k: v for k, v in vars(l14).items() if k not in ("name", "image_size")}
    assert abs(g.vision_flops_per_image() / 1e9 - 381.9) < 0.1


def test_hub_id_and_the_existing_names():
    assert HUB_IDS["ViT-L/14@336px"] == "openai/clip-vit-large-patch14-336"
    assert list(CHECKPOINTS)[:3] == ["ViT-B/32", "ViT-B/16", "ViT-L/14"]
    assert HUB_IDS["ViT-L/14"] == "openai/clip-vit-large-patch14"


def test_hf_config_has_577_vision_positions():
    pytest.importorskip("transformers")
    cfg = geometry("ViT-L/14@336px").hf_configs()
    vc = cfg.vision_config
    assert (vc.image_size, vc.patch_size, vc.hidden_size, vc.num_attention_heads) == (336, 14, 1024, 16)
    assert (vc.image_size // vc.patch_size) ** 2 + 1 == 577
    assert cfg.text_config.hidden_size == 768 and cfg.projection_dim == 768


def test_hf_model_registers_577_position_embeddings():
    pytest.importorskip("transformers")
    from transformers.models.clip.modeling_clip import CLIPVisionEmbeddings

    emb = CLIPVisionEmbeddings(geometry("ViT-L/14@336px").hf_configs().vision_config)
    assert tuple(emb.position_embedding.weight.shape) == (577, 1024)


def test_cli_accepts_the_new_checkpoint_and_keeps_its_defaults(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    a = cli.process_args(["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-L/14@336px"])
    assert a.CLIP_ckpt == "ViT-L/14@336px"
    d = cli.process_args(["--in_dataset", "ImageNet10"])
    assert d.CLIP_ckpt == "ViT-B/16" and d.batch_size == 512 and d.dtype == "fp16" and d.refine_threshold == "auto"
    with pytest.raises(SystemExit):
        cli.process_args(["--CLIP_ckpt", "ViT-L/14@448px"])


def test_full_round_batches_at_577_tokens():
    b = geometry("ViT-L/14@336px").full_round_batches()
    assert b[:6] == [28, 85, 170, 227, 312, 369]
    for n in b:   # every vision GEMM fills its last tile round
        assert all(abs(v["fill"] - 1.0) < 1e-9 for v in geometry("ViT-L/14@336px").gemm_tile_rounds(n).values())
    assert geometry("ViT-L/14@336px").full_round_batches(256, 1024)[:2] == [312, 369]
