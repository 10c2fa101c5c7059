"""Compile-time resources of the packet-loss concealment kernels (plc_kernels.hip.h; no GPU needed): none of them may use scratch -- the
Burg recursion's dynamically indexed arrays live in LDS for that reason -- and the analysis kernels beside them keep their figures."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(plc_[a-z_]+_kernel(?:I[sf]E)?|analysis_[a-z]+_kernel)E")


def test_plc_kernels_compile_without_scratch(recs):
    for name in ("plc_burg_kernel", "plc_pred_kernel", "plc_mix_kernel", "plc_fec_move_kernel"):
        r = recs[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert recs["plc_burg_kernel"]["max_flat_workgroup_size"] == 128 and recs["plc_burg_kernel"]["lds"] < 16384
    assert recs["plc_pred_kernel"]["lds"] < 32768


def test_analysis_kernels_are_unchanged_beside_them(recs):
    for name in ("analysis_spectrum_kernel", "analysis_xcorr_kernel", "analysis_pitch_kernel"):
        assert recs[name]["scratch"] == 0 and recs[name]["vgpr_spill"] == 0, name
