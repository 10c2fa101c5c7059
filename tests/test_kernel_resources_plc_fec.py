"""Compile-time resources of the batched FEC feed's kernel (plc_kernels.hip.h: plc_fec_feed_kernel; no GPU needed): no scratch, and its LDS is
the staging buffer of the ring's compaction -- 100 rows of 20 floats -- and nothing else."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(plc_fec_[a-z]+_kernel)E")


def test_fec_feed_kernel_uses_no_scratch_and_only_its_staging_buffer(recs):
    r = recs["plc_fec_feed_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == 100 * 20 * 4, r
    assert r["max_flat_workgroup_size"] == 256, r
