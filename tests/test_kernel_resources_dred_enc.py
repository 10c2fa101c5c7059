"""Compile-time resources of the DRED encoder's kernel (rdovae_enc_kernels.hip.h: rdovae_enc_kernel<S>, S = 1, 2, 4, 8; no GPU needed): exactly
these four instantiations exist, and none uses scratch or spills a register -- the encoder's arrays reach the kernel as a device-resident block it
walks step by step, like the decoder's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(rdovae_[a-z_]+_kernelILi\d+EE)")


def test_every_form_of_the_encode_kernel_compiles_without_scratch_or_spills(recs):
    assert sorted(recs) == ["rdovae_enc_kernelILi%dEE" % s for s in (1, 2, 4, 8)], sorted(recs)
    for name, r in recs.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 1024 and r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 128, (name, r)         # (static: the streams' counts, live flags and ring heads; the buffers are dynamic, sized from the widths)
