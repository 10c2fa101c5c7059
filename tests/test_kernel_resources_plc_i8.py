"""Compile-time resources of the int8 PLC prediction kernel (plc_kernels.hip.h: plc_pred_i8_kernel; no GPU needed), from the compiler's metadata
as tests/test_kernel_resources_plc.py reads the other PLC kernels': no scratch, and no more LDS than the float plc_pred_kernel.
Measured: 44 VGPRs, 5 952 bytes of LDS (the 57 inputs 240, two float states 4 096, three packed int8 vectors 1 536, the output 80); the float
kernel has 24 VGPRs and 18 752 bytes (it also keeps the dense output as floats and both GRUs' pre-activations, 12 KB, in LDS)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(plc_pred(?:_i8)?_kernel)E")


def test_int8_prediction_kernel_has_no_scratch_and_no_more_lds_than_the_float_one(recs):
    q, f = recs["plc_pred_i8_kernel"], recs["plc_pred_kernel"]
    assert q["scratch"] == 0 and q["vgpr_spill"] == 0 and q["sgpr_spill"] == 0, q
    assert q["max_flat_workgroup_size"] == 256
    assert q["lds"] <= f["lds"], (q["lds"], f["lds"])
    assert q["lds"] <= 5952, q          # the measured figure: the arrays listed above
