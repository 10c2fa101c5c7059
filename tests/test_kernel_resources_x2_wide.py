"""Compile-time resource checks of the two-group sample kernel's streamed variants (sample_x2w.hip; no GPU needed): two waves per SIMD leave 256
VGPRs, and the half-step loop must touch neither scratch nor FLAT memory -- the weights that are not register-resident come from L2 through the
ring, never from a spill."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
VARIANTS = [48, 64, 80, 96]


@pytest.fixture(scope="module")
def x2w(tmp_path_factory):
    import kernel_resources as kr
    path = str(tmp_path_factory.mktemp("asm") / "sample_x2w.s")
    kr.compile_asm(8, path, wide=True)
    return {r["NW"]: r for r in kr.analyse(path)}, open(path).read()


def test_the_unit_holds_the_streamed_variants_and_nothing_else(x2w):
    recs, asm = x2w
    assert sorted(recs) == VARIANTS
    src = open(os.path.join(ROOT, "lpcnet_amd", "csrc", "sample_variants.h")).read()
    assert re.search(r"#define LPCN_VARIANTS_X2W\(X\) " + " ".join("X\\(%d\\)" % v for v in VARIANTS) + r"\s*\n", src)
    assert len(re.findall(r"\.max_flat_workgroup_size:\s+512", asm)) == len(VARIANTS) and not re.search(r"\.max_flat_workgroup_size:\s+(?!512)\d+", asm)


@pytest.mark.parametrize("nw", VARIANTS)
def test_no_scratch_and_no_flat_access_in_the_half_step_loop(nw, x2w):
    rec = x2w[0][nw]
    assert rec["S"] == 8 and rec["vgpr"] <= 256
    assert rec["scratch_insts_in_sample_loop"] == 0 and rec["flat_insts_in_sample_loop"] == 0
    assert rec["sample_loop_asm_lines"] > 2000                  # (the marker and the loop were found)
    assert rec["vgpr_spill"] == 0 and rec["scratch_bytes"] == 0
