"""Compile-time resources of the group gather / scatter kernels (plc_kernels.hip.h; no GPU needed): plain copies, so no scratch, no LDS and no
spills.  DESIGN.md section 4.4 records their register counts."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(group_[a-z]+_kernel)E")


@pytest.mark.parametrize("name", ["group_gather_kernel", "group_scatter_kernel"])
def test_group_kernels_use_no_scratch_and_no_lds(recs, name):
    r = recs[name]
    print(name, r)
    assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert r["max_flat_workgroup_size"] == 256
