"""ISA audit of the streaming attention kernels (attention.hip attn_long_kernel / attn_long_f32_kernel), CPU only: hipcc
cross-compiles gfx950 with the Makefile's shipped flags.  Every instantiation has a zero private segment (no scratch, no
spills) and keeps no compiler vmcnt wait inside its tile loop (one would drain the LDS-DMA of the next tile behind every
tile); the LDS footprint and register count let at least two workgroups share a CU (in the 16-bit mode, which the
tower runs)."""
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


@pytest.fixture(scope="module")
def attn_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_attn")
    # the flags of mcm_amd/csrc/Makefile (no -DMCM_HARNESS: the shipped code)
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "mcm_amd", "csrc"),
           "-c", os.path.join(ROOT, "mcm_amd", "csrc", "attention.hip"), "-o", str(out / "attention.o"), "-save-temps=obj"]
    subprocess.run(cmd, check=True, cwd=str(out), capture_output=True, timeout=600)
    asm = [f for f in os.listdir(out) if f.endswith("gfx950.s")]
    assert asm, os.listdir(out)
    return open(out / asm[0]).read()


def _meta(isa):
    """{kernel symbol: metadata fields} of the code object's amdhsa.kernels list."""
    res = {}
    for block in isa.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        res[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                               "group_segment_fixed_size")}
    return res


INSTANCES = {  # demangled form -> (mode, symbol pattern)
    "attn_long_kernel<bf16>": ("16-bit", r"attn_long_kernelILi0ELb0E"),
    "attn_long_kernel<fp16>": ("16-bit", r"attn_long_kernelILi2ELb0E"),
    "attn_long_kernel<fp16, X2>": ("x2", r"attn_long_kernelILi2ELb1E"),
    "attn_long_f32_kernel": ("fp32", r"attn_long_f32_kernelILi8E"),
}


def _find(meta, pat):
    names = [n for n in meta if re.search(pat, n) and not n.endswith(".kd")]
    assert len(names) == 1, (pat, names)
    return names[0]


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_long_attention_has_no_private_segment(attn_isa, inst):
    meta = _meta(attn_isa)
    m = meta[_find(meta, INSTANCES[inst][1])]
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    name = _find(meta, INSTANCES[inst][1])
    body = re.search(r"^%s:\s.*?^\.Lfunc_end" % re.escape(name), attn_isa, re.S | re.M).group(0)
    assert "scratch_" not in body and "buffer_store" not in body


@pytest.mark.parametrize("inst", [k for k, v in INSTANCES.items() if v[0] != "fp32"])
def test_tile_loop_waits_only_for_the_dma_it_counts(attn_isa, inst):
    """Inside the tile loop of the LDS-DMA kernels the one vmcnt wait is the hand-written vmcnt(0) before the barrier."""
    meta = _meta(attn_isa)
    name = _find(meta, INSTANCES[inst][1])
    body = re.search(r"^%s:\s.*?^\.Lfunc_end" % re.escape(name), attn_isa, re.S | re.M).group(0)
    lines = body.splitlines()
    head = [i for i, l in enumerate(lines) if "Loop Header" in l]
    assert len(head) == 1, head
    # the loop runs from its header to the last backward branch to it
    label = lines[head[0]].split(":")[0]
    back = [i for i, l in enumerate(lines) if re.search(r"s_cbranch\w*\s+%s\b|s_branch\s+%s\b" % (label, label), l)]
    end = max(back) if back else len(lines)
    loop = lines[head[0]:end + 1]
    waits = [l.strip() for l in loop if "vmcnt" in l]
    assert waits == ["s_waitcnt vmcnt(0)"], waits
    assert sum("global_load_lds_dwordx4" in l for l in loop) > 0


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_two_workgroups_fit_a_cu(attn_isa, inst):
    meta = _meta(attn_isa)
    m = meta[_find(meta, INSTANCES[inst][1])]
    lds = m["group_segment_fixed_size"]
    assert lds > 0   # static: the code object states the whole footprint
    assert 2 * lds <= LDS_PER_CU, (inst, lds)
    # 2 workgroups x 8 waves = 4 waves per SIMD: at most 128 VGPRs per lane
    assert m["vgpr_count"] <= VGPRS_PER_SIMD_LANE // (2 * WAVES // 4), (inst, m["vgpr_count"])
    if INSTANCES[inst][0] == "16-bit":
        assert LDS_PER_CU // lds >= 4, (inst, lds)   # the tower's mode: LDS is not what bounds its occupancy
