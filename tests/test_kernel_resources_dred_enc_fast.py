"""Compile-time resources of the DRED encoder's FAST kernel (rdovae_enc_fast_kernels.hip.h: rdovae_enc_fast_kernel<T, U>: T = 16 streams per workgroup
with U = 16 steps of weights in flight, T = 32 with U = 8; no GPU needed): no scratch, no spilled register, twelve waves at three per SIMD, and a small
static LDS -- the states, the activation buffer, gdense1's output and the staging chunks are dynamic, sized from the widths.  The set of
instantiations found is exactly the set built."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BUILT = ["rdovae_enc_fast_kernelILi16ELi16EE", "rdovae_enc_fast_kernelILi32ELi8EE"]


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(rdovae_enc_fast_kernelILi\d+ELi\d+EE)")


def test_every_fast_instantiation_compiles_without_scratch_or_spills(recs):
    assert sorted(recs) == BUILT, sorted(recs)
    for name, r in recs.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 768 and r["vgpr"] <= 168, (name, r)          # (512 registers of a SIMD lane over three waves)
        assert r["lds"] <= 512, (name, r)          # (static: the streams' counts and ring heads)
