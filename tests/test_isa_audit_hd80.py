"""ISA audit of the head_dim-80 attention family (attention.hip attn_hd80_kernel / attn_hd80_f32_kernel) and of the five-vector
LayerNorm instantiations (layernorm.hip, 1024 < D <= 1280), CPU only: hipcc cross-compiles gfx950 with the Makefile's shipped
flags.  Every instantiation has a zero private segment, the static LDS DESIGN.md 4.8 states, a register count inside the stated
occupancy, the MFMA shapes of its decomposition and no other, and no compiler vmcnt wait inside its tile loop."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD_LANE = 512
WAVES = 8   # attention.hip LONG_NW


def _compile(tmp_path_factory, src):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_" + src.split(".")[0])
    # the flags of mcm_amd/csrc/Makefile (no -DMCM_HARNESS: the shipped code)
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "mcm_amd", "csrc"),
           "-c", os.path.join(ROOT, "mcm_amd", "csrc", src), "-o", str(out / (src + ".o")), "-save-temps=obj"]
    subprocess.run(cmd, check=True, cwd=str(out), capture_output=True, timeout=900)
    asm = [f for f in os.listdir(out) if f.endswith("gfx950.s")]
    assert asm, os.listdir(out)
    return open(out / asm[0]).read()


@pytest.fixture(scope="module")
def attn_isa(tmp_path_factory):
    return _compile(tmp_path_factory, "attention.hip")


@pytest.fixture(scope="module")
def ln_isa(tmp_path_factory):
    return _compile(tmp_path_factory, "layernorm.hip")


def _meta(isa):
    """{kernel symbol: metadata fields} of the code object's amdhsa.kernels list."""
    res = {}
    for block in isa.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        res[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                               "group_segment_fixed_size")}
    return res


def _find(meta, pat):
    names = [n for n in meta if re.search(pat, n) and not n.endswith(".kd")]
    assert len(names) == 1, (pat, names)
    return names[0]


def _body(isa, name):
    return re.search(r"^%s:\s.*?^\.Lfunc_end" % re.escape(name), isa, re.S | re.M).group(0)


# instance -> (symbol pattern, static LDS in bytes as DESIGN.md 4.8 states it, workgroups per CU the design claims,
#              MFMA mnemonics that must be there, MFMA mnemonics that must not)
INSTANCES = {
    "attn_hd80_kernel<bf16>": (r"attn_hd80_kernelILi0ELb0E", 40960, 2, ["v_mfma_f32_16x16x32_bf16"], ["16x16x16", "16x16x4"]),
    "attn_hd80_kernel<fp16>": (r"attn_hd80_kernelILi2ELb0E", 40960, 2, ["v_mfma_f32_16x16x32_f16"], ["16x16x16", "16x16x4"]),
    "attn_hd80_kernel<fp16, X2>": (r"attn_hd80_kernelILi2ELb1E", 81920, 2, ["v_mfma_f32_16x16x32_f16"], ["16x16x16", "16x16x4"]),
    "attn_hd80_f32_kernel": (r"attn_hd80_f32_kernelILi8E", 88064, 1, ["v_mfma_f32_16x16x4_f32"], ["16x16x32", "16x16x16"]),
}


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_hd80_attention_has_no_private_segment(attn_isa, inst):
    meta = _meta(attn_isa)
    name = _find(meta, INSTANCES[inst][0])
    m = meta[name]
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    body = _body(attn_isa, name)
    assert "scratch_" not in body and "buffer_store" not in body


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_hd80_static_lds_and_registers_match_the_stated_occupancy(attn_isa, inst):
    pat, lds, wgs, _, _ = INSTANCES[inst]
    meta = _meta(attn_isa)
    m = meta[_find(meta, pat)]
    print("ISA %s: LDS %d B, %d VGPRs" % (inst, m["group_segment_fixed_size"], m["vgpr_count"]))
    assert m["group_segment_fixed_size"] == lds, m      # static: the code object states the whole footprint
    assert wgs * lds <= LDS_PER_CU, (inst, lds)
    assert (wgs + 1) * lds > LDS_PER_CU or wgs == 2, (inst, lds)   # fp32: one workgroup is what the LDS admits, as stated
    # wgs workgroups x 8 waves on 4 SIMDs: 512 / (2 wgs) VGPRs per lane at most
    assert m["vgpr_count"] <= VGPRS_PER_SIMD_LANE // (wgs * WAVES // 4), (inst, m["vgpr_count"])


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_hd80_mfma_decomposition(attn_isa, inst):
    """16-bit and split: 32-deep steps only (the third over a zero-padded tail; no 16x16x16 in the accumulator chain);
    fp32: v_mfma_f32_16x16x4_f32 only.  Per 64-key tile: 16-bit 4 x 3 (S) + 2 x 6 (row sum, five O blocks) = 24,
    split 4 x 9 + 2 x 17 = 70, fp32 4 x 20 + 16 x 5 = 160."""
    pat, _, _, want, never = INSTANCES[inst]
    meta = _meta(attn_isa)
    body = _body(attn_isa, _find(meta, pat))
    mfma = [l.split()[0] for l in body.splitlines() if l.strip().startswith("v_mfma")]
    assert mfma, inst
    for w in want:
        assert any(x.startswith(w) for x in mfma), (inst, w, sorted(set(mfma)))
    for n in never:
        assert not any(n in x for x in mfma), (inst, n, sorted(set(mfma)))
    count = {"attn_hd80_kernel<bf16>": 24, "attn_hd80_kernel<fp16>": 24, "attn_hd80_kernel<fp16, X2>": 70,
             "attn_hd80_f32_kernel": 160}[inst]
    assert len(mfma) == count, (inst, len(mfma))


@pytest.mark.parametrize("inst", [k for k in INSTANCES if "f32" not in k])
def test_hd80_tile_loop_waits_only_for_the_dma_it_counts(attn_isa, inst):
    """Inside the tile loop of the LDS-DMA kernels the one vmcnt wait is the hand-written vmcnt(0) before the barrier."""
    meta = _meta(attn_isa)
    body = _body(attn_isa, _find(meta, INSTANCES[inst][0]))
    lines = body.splitlines()
    head = [i for i, l in enumerate(lines) if "Loop Header" in l]
    assert len(head) == 1, head
    label = lines[head[0]].split(":")[0]
    back = [i for i, l in enumerate(lines) if re.search(r"s_cbranch\w*\s+%s\b|s_branch\s+%s\b" % (label, label), l)]
    end = max(back) if back else len(lines)
    loop = lines[head[0]:end + 1]
    waits = [l.strip() for l in loop if "vmcnt" in l]
    assert waits == ["s_waitcnt vmcnt(0)"], waits
    assert sum("global_load_lds_dwordx4" in l for l in loop) > 0


def test_head_dim_64_long_kernels_keep_their_footprint(attn_isa):
    """The sibling family was added beside attn_long_kernel, not into it: the 64-wide instantiations keep 32 / 64 / 68 KiB."""
    meta = _meta(attn_isa)
    assert meta[_find(meta, r"attn_long_kernelILi2ELb0E")]["group_segment_fixed_size"] == 32768
    assert meta[_find(meta, r"attn_long_kernelILi2ELb1E")]["group_segment_fixed_size"] == 65536
    assert meta[_find(meta, r"attn_long_f32_kernelILi8E")]["group_segment_fixed_size"] == 69632


LN_WIDE = {  # the five-vector instantiations: <OUT, X2, 5>
    "layernorm_kernel<bf16, 5>": r"layernorm_kernelILi0ELb0ELi5E",
    "layernorm_kernel<fp32, 5>": r"layernorm_kernelILi1ELb0ELi5E",
    "layernorm_kernel<fp16, 5>": r"layernorm_kernelILi2ELb0ELi5E",
    "layernorm_kernel<fp16, X2, 5>": r"layernorm_kernelILi2ELb1ELi5E",
    "layernorm_pre_kernel<bf16, 5>": r"layernorm_pre_kernelILi0ELb0ELi5E",
    "layernorm_pre_kernel<fp32, 5>": r"layernorm_pre_kernelILi1ELb0ELi5E",
    "layernorm_pre_kernel<fp16, 5>": r"layernorm_pre_kernelILi2ELb0ELi5E",
    "layernorm_pre_kernel<fp16, X2, 5>": r"layernorm_pre_kernelILi2ELb1ELi5E",
}


@pytest.mark.parametrize("inst", list(LN_WIDE))
def test_wide_layernorm_has_no_private_segment(ln_isa, inst):
    meta = _meta(ln_isa)
    name = _find(meta, LN_WIDE[inst])
    m = meta[name]
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert "scratch_" not in _body(ln_isa, name)
    # ... and the four-vector instantiation of the same kernel is still there, under its own symbol
    assert _find(meta, LN_WIDE[inst].replace("Li5E", "Li4E"))
