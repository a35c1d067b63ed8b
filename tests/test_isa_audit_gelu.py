"""ISA audit of the ping-pong GEMM kernel with the exact-GELU epilogue, gemm_pp_kernel<bf16 | fp16, EPI_GELU_ERF> (CPU: hipcc
cross-compiles gfx950): the three properties tests/test_isa_audit.py holds the QuickGELU instantiation to — no scratch, only
the two hand-written vmcnt waits, one compute phase of 64 MFMAs — and no call: gelu_erf is v_rcp_f32 + v_exp_f32 + a Horner
chain inlined into the epilogue, not an out-of-line libm erff."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EPI_GELU_ERF = 6


@pytest.fixture(scope="module")
def gemm_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_gelu")
    # the flags of mcm_amd/csrc/Makefile (the shipped code, not the harness build)
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "mcm_amd", "csrc"),
           "-c", os.path.join(ROOT, "mcm_amd", "csrc", "gemm.hip"), "-o", str(out / "gemm.o"), "-save-temps=obj"]
    subprocess.run(cmd, check=True, cwd=str(out), capture_output=True, timeout=600)
    asm = [f for f in os.listdir(out) if f.endswith("gfx950.s")]
    assert asm, os.listdir(out)
    return open(out / asm[0]).read()


def test_the_enum_value_is_the_one_audited():
    src = open(os.path.join(ROOT, "mcm_amd", "csrc", "common.hpp")).read()
    assert re.search(r"EPI_GELU_ERF = %d," % EPI_GELU_ERF, src)


@pytest.mark.parametrize("prec", [0, 2], ids=["bf16", "fp16"])
def test_pingpong_gelu_erf_kernel_is_as_clean_as_the_quick_gelu_one(gemm_isa, prec):
    m = re.search(r"^(_ZN\S*_114gemm_pp_kernelILi%dELi%dEEEv8GemmArgs):\s.*?^\.Lfunc_end" % (prec, EPI_GELU_ERF), gemm_isa, re.S | re.M)
    assert m, "gemm_pp_kernel<%d, EPI_GELU_ERF> not found" % prec
    body = m.group(0)
    assert "scratch_" not in body
    assert len(re.findall(r"s_waitcnt vmcnt", body)) == 2  # prologue + end of the compute phase
    assert len(re.findall(r"v_mfma_f32_16x16x32", body)) == 64  # one compute phase, no duplicated loop bodies
    assert "s_swappc_b64" not in body and "s_call_b64" not in body  # nothing out of line
    # the activation itself: one reciprocal and one exponential per element, no division expansion
    assert "v_rcp_f32" in body and "v_exp_f32" in body and "v_div_scale_f32" not in body
