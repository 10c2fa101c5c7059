"""Compile-time resource checks of the twelve-wave sample kernel (sample_x3.hip; no GPU needed): three waves per SIMD need <= 168 VGPRs, and the half-step
loop must not touch scratch."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def x3(tmp_path_factory):
    import kernel_resources as kr
    path = str(tmp_path_factory.mktemp("asm") / "sample_x3.s")
    kr.compile_asm(12, path)
    recs = kr.analyse(path)
    assert len(recs) == 1
    return recs[0], open(path).read()


def test_three_waves_per_simd_and_no_scratch_in_the_half_step_loop(x3):
    rec, asm = x3
    assert rec["vgpr"] <= 168
    assert rec["scratch_insts_in_sample_loop"] == 0 and rec["flat_insts_in_sample_loop"] == 0
    assert rec["sample_loop_asm_lines"] > 2000                  # (the marker and the loop were found)
    assert re.search(r"\.max_flat_workgroup_size:\s+768", asm)
    # GRU-B's assembly block names registers of this kernel's budget only
    assert not re.search(r"\bv(1[7-9]\d|16[89]|2\d\d)\b", asm)


def test_no_new_compile_time_switches():
    src = open(os.path.join(ROOT, "lpcnet_amd", "csrc", "sample_kernel_x3.hip.h")).read() + open(os.path.join(ROOT, "lpcnet_amd", "csrc", "sample_x3.hip")).read()
    assert not re.findall(r"#\s*ifn?def\s+LPCN_\w+", src)


def test_generated_loop_is_what_the_generator_emits():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_grub_asm.py"), "--lds", "4", "--top", "168", "--name", "LPCN_GRUB_LDS168_CLOBBERS"],
                         capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "lpcnet_amd", "csrc", "grub_lds_loop_s4_v168.inc")).read()
