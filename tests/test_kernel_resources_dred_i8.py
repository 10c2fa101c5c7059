"""Compile-time resources of the int8 (DOT_PROD) forms of the two DRED kernels (dred_kernels.hip.h: dred_decode_i8_kernel<S>,
rdovae_enc_kernels.hip.h: rdovae_enc_i8_kernel<S>, S = 1, 2, 4, 8; no GPU needed): exactly these eight exist, and none uses scratch or spills a
register.  The float kernels keep their names and their own tests (test_kernel_resources_dred.py, test_kernel_resources_dred_enc.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+([a-z_]+_i8_kernelILi\d+EE)")


def test_every_int8_form_of_both_kernels_compiles_without_scratch_or_spills(recs):
    assert sorted(recs) == sorted("%s_i8_kernelILi%dEE" % (k, s) for k in ("dred_decode", "rdovae_enc") for s in (1, 2, 4, 8)), sorted(recs)
    for name, r in recs.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 1024 and r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 96, (name, r)          # (static: the streams' counts, flags and ring heads; the buffers are dynamic, sized from the widths)
