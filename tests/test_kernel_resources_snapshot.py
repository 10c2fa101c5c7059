"""Compile-time resources of the snapshot kernels (snapshot_kernels.hip.h; no GPU needed): like the stream copy kernel
(tests/test_kernel_resources_roster.py) plain copies driven by a small by-value table, so no scratch, no LDS and no spills, in workgroups of 256.
A copy loop holds one 16-byte element, two addresses and the row's fields: at 64 VGPRs or fewer a SIMD still keeps eight wavefronts of them,
the most it can, and anything above that would mean the table had been copied into registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(stream_(?:gather|scatter|copy)_kernel)E")


@pytest.mark.parametrize("kernel", ["stream_gather_kernel", "stream_scatter_kernel"])
def test_snapshot_kernels_use_no_scratch_and_no_lds(kernel, recs):
    r = recs[kernel]
    print(kernel, r, "stream_copy_kernel", recs["stream_copy_kernel"])
    assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["max_flat_workgroup_size"] == 256
    assert r["vgpr"] <= 64, r
