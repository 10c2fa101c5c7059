"""Compile-time resources of the stream copy kernel (roster_kernels.hip.h; no GPU needed): a plain copy driven by a small by-value table, so no
scratch, no LDS and no spills, in workgroups of 256."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(stream_copy_kernel)E")


def test_stream_copy_kernel_uses_no_scratch_and_no_lds(recs):
    r = recs["stream_copy_kernel"]
    print("stream_copy_kernel", r)
    assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["max_flat_workgroup_size"] == 256
