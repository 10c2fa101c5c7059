"""Compile-time resources of the PLC prediction kernels with S = 2, 4, 8 streams per workgroup (plc_kernels.hip.h: plc_pred_s_kernel<S>,
plc_pred_s_int8_kernel<S>; no GPU needed), from the compiler's metadata as tests/test_kernel_resources_plc.py reads the S = 1 kernels': no scratch,
256 lanes, and no static LDS -- all of a form's LDS is dynamic, sized by the blob's widths, and bounded by the form rule
(tests/test_plc_pred_form_host.py).  The S = 1 kernels are checked where they always were (test_kernel_resources_plc.py, _plc_i8.py).
Measured VGPRs: float 37 / 43 / 62 at S = 2 / 4 / 8, int8 37 / 52 / 88 (the int8 S = 8 form also parks four SGPRs in VGPR lanes: no scratch).  A
workgroup is one wave per SIMD, and the form rule lets a form run only where at most a few of its workgroups share a CU's LDS, so the LDS, not
the registers, sets how many share a CU: 88 VGPRs still allow five."""
import os
import sys

import pytest

from lpcnet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ["plc_pred_s_%skernelILi%dEE" % (q, s) for q in ("", "int8_") for s in (2, 4, 8)]
VGPR = {"plc_pred_s_kernelILi2EE": 37, "plc_pred_s_kernelILi4EE": 43, "plc_pred_s_kernelILi8EE": 62,
        "plc_pred_s_int8_kernelILi2EE": 37, "plc_pred_s_int8_kernelILi4EE": 52, "plc_pred_s_int8_kernelILi8EE": 88}          # the measured figures


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(plc_pred_s_(?:int8_)?kernelILi\d+EE)")


def test_the_six_forms_exist_without_scratch_or_static_lds(recs):
    assert callable(api.plc_pred_form_table)
    assert sorted(recs) == sorted(NAMES), sorted(recs)
    for name in NAMES:
        r = recs[name]
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, (name, r)
        assert r["lds"] == 0, (name, r)                 # the LDS base: everything is dynamic (plc_records.h: plc_pred_lds_bytes)
        assert r["vgpr"] <= VGPR[name], (name, r)
