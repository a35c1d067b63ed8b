"""The MLP activation as a property of the model (ABI 5): the OpenCLIP-trained checkpoint names resolve to the geometry of their
OpenAI namesakes with `hidden_act = "gelu"` in both towers, `to_c` / `hf_configs` carry it, the ctypes mirror has the size of
the C struct, the CLI knows the names, and a checkpoint whose `config.json` names the other activation is refused instead of
being scored wrong."""
import ctypes
import dataclasses
import json
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from mcm_amd import config as cfgmod
from mcm_amd.config import CHECKPOINTS, HUB_IDS, TEST_GEOMETRIES, CConfig, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPENAI = ["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px"]
LAION = ["ViT-B/32-laion2b", "ViT-B/16-laion2b", "ViT-L/14-laion2b"]


def test_new_checkpoints_resolve_to_their_namesakes_geometry():
    assert list(CHECKPOINTS)[:4] == OPENAI and list(CHECKPOINTS)[4:] == LAION
    for name in LAION:
        geo, base = geometry(name), geometry(name[:-len("-laion2b")])
        assert geo.name == name and (geo.v_hidden_act, geo.t_hidden_act) == ("gelu", "gelu")
        assert dataclasses.replace(geo, name=base.name, v_hidden_act="quick_gelu", t_hidden_act="quick_gelu") == base
        assert HUB_IDS[name].startswith("laion/CLIP-ViT-")
    for name in OPENAI:
        assert (geometry(name).v_hidden_act, geometry(name).t_hidden_act) == ("quick_gelu", "quick_gelu")
    for name in ("tiny-gelu", "B16-2L-gelu"):
        geo, base = geometry(name), TEST_GEOMETRIES[name[:-len("-gelu")]]
        assert (geo.v_hidden_act, geo.t_hidden_act) == ("gelu", "gelu") and geo.v_width == base.v_width


def test_hf_configs_carry_the_activation():
    pytest.importorskip("transformers")
    for name in LAION + ["tiny-gelu"]:
        c = geometry(name).hf_configs()
        assert (c.vision_config.hidden_act, c.text_config.hidden_act) == ("gelu", "gelu")
    for name in OPENAI + ["tiny", "B16-2L"]:
        c = geometry(name).hf_configs()
        assert (c.vision_config.hidden_act, c.text_config.hidden_act) == ("quick_gelu", "quick_gelu")
    mixed = dataclasses.replace(geometry("tiny"), v_hidden_act="gelu").hf_configs()
    assert (mixed.vision_config.hidden_act, mixed.text_config.hidden_act) == ("gelu", "quick_gelu")


def test_to_c_sets_the_ints():
    assert cfgmod.ABI_VERSION == 5 and cfgmod.HIDDEN_ACTS == {"quick_gelu": 0, "gelu": 1}
    c = geometry("ViT-B/16-laion2b").to_c()
    assert (c.abi_version, c.v_hidden_act, c.t_hidden_act, c.v_width, c.patch_size) == (5, 1, 1, 768, 16)
    c = geometry("ViT-B/16").to_c()
    assert (c.v_hidden_act, c.t_hidden_act) == (0, 0)
    c = dataclasses.replace(geometry("tiny"), t_hidden_act="gelu").to_c()
    assert (c.v_hidden_act, c.t_hidden_act) == (0, 1)
    with pytest.raises(ValueError, match="gelu_new"):
        dataclasses.replace(geometry("tiny"), v_hidden_act="gelu_new").to_c()


def test_cconfig_has_the_size_and_the_tail_of_the_c_struct(tmp_path):
    """A two-line probe compiled with the host compiler against include/mcm.h: sizeof(mcm_config), the offsets of the two new
    fields (they are the struct's last) and the ABI version."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcm.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d %d %d\\n", sizeof(mcm_config), offsetof(mcm_config, v_hidden_act), '
                   'offsetof(mcm_config, t_hidden_act), MCM_ABI_VERSION, MCM_ACT_QUICK_GELU, MCM_ACT_GELU, MCM_LINEAR_ACT_GELU); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    size, off_v, off_t, abi, a0, a1, flag = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(CConfig)
    assert (off_v, off_t) == (CConfig.v_hidden_act.offset, CConfig.t_hidden_act.offset) == (size - 8, size - 4)
    assert (abi, a0, a1, flag) == (cfgmod.ABI_VERSION, 0, 1, 8)


def test_cli_knows_the_new_checkpoints():
    import eval_ood_detection as cli

    for name in LAION:
        a = cli.process_args(["--in_dataset", "ImageNet10", "--CLIP_ckpt", name])
        assert a.CLIP_ckpt == name and name in HUB_IDS
    assert cli.process_args(["--in_dataset", "ImageNet10"]).CLIP_ckpt == "ViT-B/16"


def _write_checkpoint(d, geo, hf_acts=None):
    """A seeded tiny `.safetensors` under HF names in directory d, with the `config.json` HF would save (hf_acts = the
    (vision, text) hidden_act it names; None: no config.json)."""
    from safetensors.numpy import save_file

    from mcm_amd.weights import synth_state_dict

    sd = {k: np.ascontiguousarray(v) for k, v in synth_state_dict(geo, 3).items()}
    path = os.path.join(str(d), "model.safetensors")
    save_file(sd, path)
    if hf_acts is not None:
        with open(os.path.join(str(d), "config.json"), "w") as f:
            json.dump({"model_type": "clip", "projection_dim": geo.proj_dim,
                       "vision_config": {"hidden_size": geo.v_width, "hidden_act": hf_acts[0]},
                       "text_config": {"hidden_size": geo.t_width, "hidden_act": hf_acts[1]}}, f)
    return path, sd


def test_config_json_guard(tmp_path, caplog):
    pytest.importorskip("safetensors")
    from mcm_amd.weights import load_state_dict_file

    tiny, tiny_gelu = geometry("tiny"), geometry("tiny-gelu")
    (tmp_path / "g").mkdir()
    path, sd = _write_checkpoint(tmp_path / "g", tiny, ("gelu", "gelu"))
    # a match passes, by file and by directory
    for p in (path, str(tmp_path / "g")):
        got = load_state_dict_file(p, tiny_gelu)
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    # a mismatch raises and names both values
    with pytest.raises(ValueError, match=r"vision=gelu / text=gelu.*vision=quick_gelu / text=quick_gelu"):
        load_state_dict_file(path, tiny)
    (tmp_path / "q").mkdir()
    qpath, _ = _write_checkpoint(tmp_path / "q", tiny, ("quick_gelu", "quick_gelu"))
    with pytest.raises(ValueError, match="quick_gelu"):
        load_state_dict_file(qpath, tiny_gelu)
    assert set(load_state_dict_file(qpath, tiny)) == set(sd)
    # ... and the --CLIP_ckpt that would match, at a real geometry (only the config.json is read before the refusal)
    with pytest.raises(ValueError, match=r"--CLIP_ckpt ViT-B/16-laion2b matches"):
        load_state_dict_file(path, geometry("ViT-B/16"))
    with pytest.raises(ValueError, match=r"--CLIP_ckpt ViT-L/14 matches"):
        load_state_dict_file(qpath, geometry("ViT-L/14-laion2b"))
    # one tower only is a mismatch too
    (tmp_path / "m").mkdir()
    mpath, _ = _write_checkpoint(tmp_path / "m", tiny, ("gelu", "quick_gelu"))
    with pytest.raises(ValueError, match="vision=gelu / text=quick_gelu"):
        load_state_dict_file(mpath, tiny_gelu)
    # an empty directory is a missing checkpoint, and nothing is assumed about it first
    (tmp_path / "e").mkdir()
    with caplog.at_level(logging.INFO, logger="mcm_amd"):
        caplog.clear()
        with pytest.raises(FileNotFoundError):
            load_state_dict_file(str(tmp_path / "e"), tiny)
    assert not caplog.records
    # no config.json: nothing to check, one line says what is assumed (a warning: `tiny` has a twin with the other activation)
    (tmp_path / "n").mkdir()
    npath, _ = _write_checkpoint(tmp_path / "n", tiny, None)
    with caplog.at_level(logging.WARNING, logger="mcm_amd"):
        caplog.clear()
        load_state_dict_file(npath, tiny_gelu)
    lines = [r.getMessage() for r in caplog.records if "config.json" in r.getMessage()]
    assert len(lines) == 1 and "vision=gelu / text=gelu" in lines[0]
    # ... at info level for a shape that no geometry here pairs with the other activation
    lone = dataclasses.replace(tiny, name="lone", v_layers=1, t_layers=1)
    (tmp_path / "l").mkdir()
    lpath, _ = _write_checkpoint(tmp_path / "l", lone, None)
    with caplog.at_level(logging.INFO, logger="mcm_amd"):
        caplog.clear()
        load_state_dict_file(lpath, lone)
    assert [r.levelno for r in caplog.records if "config.json" in r.getMessage()] == [logging.INFO]
