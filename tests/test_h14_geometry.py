"""ViT-H/14 (LAION-2B; laion/CLIP-ViT-H-14-laion2B-s32B-b79K) as a checkpoint name: its geometry (a 1280-wide vision tower
with 80-wide heads), hub id, HF config, the CLI choice, the C config, its full-round batches, and what mcm_create still
refuses (CPU only)."""
import ctypes
import os

import pytest

from mcm_amd import config as cfgmod
from mcm_amd.config import CHECKPOINTS, HUB_IDS, TEST_GEOMETRIES, WIDE_HEAD_CHECKPOINTS, all_checkpoints, geometry

NAME = "ViT-H/14-laion2b"


def test_geometry_of_h14():
    g = geometry(NAME)
    assert (g.image_size, g.patch_size) == (224, 14)
    assert (g.v_width, g.v_heads, g.v_layers, g.v_mlp) == (1280, 16, 32, 5120)
    assert (g.t_width, g.t_heads, g.t_layers, g.t_mlp) == (1024, 16, 24, 4096)
    assert g.proj_dim == 1024 and g.max_positions == 77 and g.vocab_size == 49408
    assert (g.v_hidden_act, g.t_hidden_act) == ("gelu", "gelu") and g.ln_eps == 1e-5
    assert g.n_patches == 256 and g.v_tokens == 257
    assert g.v_width // g.v_heads == 80 and g.t_width // g.t_heads == 64
    # about 2.1 x ViT-L/14's FLOP per image
    assert 2.0 < g.vision_flops_per_image() / geometry("ViT-L/14").vision_flops_per_image() < 2.2


def test_hub_id_and_the_existing_names():
    assert HUB_IDS[NAME] == "laion/CLIP-ViT-H-14-laion2B-s32B-b79K"
    assert list(CHECKPOINTS)[:4] == ["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px"]
    assert HUB_IDS["ViT-L/14-laion2b"] == "laion/CLIP-ViT-L-14-laion2B-s32B-b82K"
    # CHECKPOINTS stays the seven 64-wide-head names; the 80-wide one has its registry, and every lookup sees both
    assert len(CHECKPOINTS) == 7 and all(g.v_width // g.v_heads == 64 for g in CHECKPOINTS.values())
    assert list(WIDE_HEAD_CHECKPOINTS) == [NAME] and list(all_checkpoints())[-1] == NAME
    assert set(HUB_IDS) == set(all_checkpoints())


def test_test_geometries_are_the_h14_towers_with_two_layers():
    g, q = geometry("H14-2L"), geometry("H14-2L-quick")
    full = geometry(NAME)
    same = lambda a, b, skip: {k: v for k, v in vars(a).items() if k not in skip} == \
        {k: v for k, v in vars(b).items() if k not in skip}   # noqa: E731
    assert same(g, full, ("name", "v_layers", "t_layers")) and (g.v_layers, g.t_layers) == (2, 2)
    assert same(q, g, ("name", "v_hidden_act", "t_hidden_act")) and (q.v_hidden_act, q.t_hidden_act) == ("quick_gelu",) * 2
    assert set(TEST_GEOMETRIES) >= {"H14-2L", "H14-2L-quick", "B16-2L", "tiny"}


def test_hf_config_has_80_wide_vision_heads():
    pytest.importorskip("transformers")
    cfg = geometry(NAME).hf_configs()
    vc, tc = cfg.vision_config, cfg.text_config
    assert (vc.image_size, vc.patch_size, vc.hidden_size, vc.num_attention_heads) == (224, 14, 1280, 16)
    assert vc.hidden_size // vc.num_attention_heads == 80
    assert (vc.intermediate_size, vc.num_hidden_layers, vc.hidden_act) == (5120, 32, "gelu")
    assert (tc.hidden_size, tc.num_attention_heads, tc.num_hidden_layers, tc.hidden_act) == (1024, 16, 24, "gelu")
    assert tc.hidden_size // tc.num_attention_heads == 64
    assert cfg.projection_dim == 1024


def test_hf_model_registers_257_by_1280_position_embeddings():
    pytest.importorskip("transformers")
    from transformers.models.clip.modeling_clip import CLIPVisionEmbeddings

    emb = CLIPVisionEmbeddings(geometry(NAME).hf_configs().vision_config)
    assert tuple(emb.position_embedding.weight.shape) == (257, 1280)


def test_cli_accepts_the_new_checkpoint_and_keeps_its_defaults(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    a = cli.process_args(["--in_dataset", "ImageNet10", "--CLIP_ckpt", NAME])
    assert a.CLIP_ckpt == NAME
    d = cli.process_args(["--in_dataset", "ImageNet10"])
    assert d.CLIP_ckpt == "ViT-B/16" and d.batch_size == 512 and d.dtype == "fp16"
    with pytest.raises(SystemExit):
        cli.process_args(["--CLIP_ckpt", "ViT-g/14-laion2b"])


def test_c_config_carries_gelu_under_abi_5():
    c = geometry(NAME).to_c()
    assert c.abi_version == 5 and cfgmod.ABI_VERSION == 5
    assert (c.v_hidden_act, c.t_hidden_act) == (1, 1)
    assert (c.v_width, c.v_heads, c.t_width, c.t_heads, c.proj_dim) == (1280, 16, 1024, 16, 1024)
    q = geometry("H14-2L-quick").to_c()
    assert (q.v_hidden_act, q.t_hidden_act) == (0, 0)


def test_full_round_batches_at_1280_wide():
    g = geometry(NAME)
    b = g.full_round_batches()
    assert b, "no batch in [1, 2048] fills every GEMM's last round"
    for n in b:   # every vision GEMM fills its last tile round
        assert all(abs(v["fill"] - 1.0) < 1e-9 for v in g.gemm_tile_rounds(n).values()), n
    # N = 3840 / 1280 / 5120 are whole multiples of the 256-column tile, and 256 images are exactly 257 row tiles
    assert all(n % 256 == 0 for n in (3 * g.v_width, g.v_width, g.v_mlp))
    assert 256 * g.v_tokens == 257 * 256


def test_weights_guard_names_this_checkpoint(tmp_path):
    """A config.json with the H/14 shapes can only belong to this name: a QuickGELU one is refused, naming nothing else."""
    import json

    from mcm_amd.weights import check_hidden_act

    p = tmp_path / "model.safetensors"
    (tmp_path / "config.json").write_text(json.dumps({"vision_config": {"hidden_act": "gelu"}, "text_config": {"hidden_act": "gelu"}}))
    check_hidden_act(str(p), geometry(NAME))
    import dataclasses

    quick = dataclasses.replace(geometry(NAME), name="H14-quick", v_hidden_act="quick_gelu", t_hidden_act="quick_gelu")
    with pytest.raises(ValueError) as e:   # the full-depth shapes under the other activation pair: the guard names this checkpoint
        check_hidden_act(str(p), quick)
    assert NAME in str(e.value)


@pytest.fixture(scope="module")
def lib():
    from mcm_amd.engine import LIB_PATH

    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g

        g.build()
    from mcm_amd import abi

    return abi.declare(ctypes.CDLL(LIB_PATH), names=["mcm_create", "mcm_last_error"])


def test_create_still_refuses_other_head_widths_without_gpu(lib):
    h = ctypes.c_void_p()
    bad = geometry("ViT-B/16").to_c()
    bad.v_heads = 8   # head_dim 96
    assert lib.mcm_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    msg = lib.mcm_last_error(None)
    assert b"64" in msg and b"80" in msg, msg
    bad = geometry("ViT-B/16").to_c()
    bad.v_heads = 7   # not even a divisor
    assert lib.mcm_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    # the text tower: head_dim 64 only (80 = 1280 / 16 is a vision-tower width), and at most 1024 wide
    bad = geometry(NAME).to_c()
    bad.t_width, bad.t_heads = 1280, 16
    assert lib.mcm_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    assert b"text" in lib.mcm_last_error(None)
    bad = geometry(NAME).to_c()
    bad.t_width, bad.t_heads = 1280, 20   # head_dim 64, but wider than the text-side row kernels
    assert lib.mcm_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    assert b"t_width <= 1024" in lib.mcm_last_error(None)
    bad = geometry(NAME).to_c()
    bad.v_width, bad.v_heads, bad.v_mlp = 1600, 20, 6400   # head_dim 80, but wider than the vision-side row kernels
    assert lib.mcm_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    assert b"v_width <= 1280" in lib.mcm_last_error(None)
