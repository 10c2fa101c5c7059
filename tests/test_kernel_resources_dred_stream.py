"""Compile-time resources of the kernels behind lpcnet_batch_dred_init / _dred_step (dred_kernels.hip.h: dred_stream_kernel<S, I8>, S = 1, 2, 4, 8
streams per workgroup, float and int8 blocks; dred_fast_kernels.hip.h: dred_stream_fast_kernel<T, U>, T = 16 with U = 16 and T = 32 with U = 8;
no GPU needed): no scratch, no spilled register, inside the bounds the resource tests of the one-shot kernels put on their counterparts
(test_kernel_resources_dred.py, _dred_i8.py, _dred_fast.py).  The one-shot kernels themselves keep the figures they had before the stream kernels
stood beside them, and a configuration without the decoder's record has the snapshot layout it had."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STREAM = ["dred_stream_kernelILi%dELb%dEE" % (s, q) for s in (1, 2, 4, 8) for q in (0, 1)]
STREAM_FAST = ["dred_stream_fast_kernelILi16ELi16EE", "dred_stream_fast_kernelILi32ELi8EE"]
# (vgpr, sgpr, static lds) of the one-shot kernels on the commit before this feature, from tools/kernel_resources.engine_kernel_resources there
BEFORE = {
    "dred_decode_kernelILi1EE": (44, 89, 16), "dred_decode_kernelILi2EE": (56, 87, 16), "dred_decode_kernelILi4EE": (64, 84, 32), "dred_decode_kernelILi8EE": (86, 86, 64),
    "dred_decode_i8_kernelILi1EE": (50, 86, 16), "dred_decode_i8_kernelILi2EE": (71, 84, 16), "dred_decode_i8_kernelILi4EE": (90, 82, 32),
    "dred_decode_i8_kernelILi8EE": (106, 82, 64),
    "dred_fast_kernelILi16ELi16EE": (136, 78, 64), "dred_fast_kernelILi32ELi8EE": (146, 74, 128),
}


@pytest.fixture(scope="module")
def recs():
    import kernel_resources as kr
    return kr.engine_kernel_resources(r"N4lpcn\d+(dred_[a-z0-9_]+_kernelI(?:L[ib]\d+E)+E)")


def test_every_stream_instantiation_compiles_without_scratch_or_spills(recs):
    assert sorted(k for k in recs if "stream" in k) == sorted(STREAM + STREAM_FAST), sorted(recs)
    for name in STREAM:
        r = recs[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 1024 and r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= (96 if name.endswith("Lb1EE") else 64), (name, r)          # (static: the streams' counts and live flags)
    for name in STREAM_FAST:
        r = recs[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 768 and r["vgpr"] <= 168, (name, r)          # (512 registers of a SIMD lane over three waves)
        assert r["lds"] <= 256, (name, r)          # (static: the streams' counts and first latents)


def test_the_one_shot_kernels_keep_their_figures(recs):
    assert sorted(k for k in recs if "stream" not in k) == sorted(BEFORE), sorted(recs)
    for name, (vgpr, sgpr, lds) in BEFORE.items():
        r = recs[name]
        assert (r["vgpr"], r["sgpr"], r["lds"]) == (vgpr, sgpr, lds) and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_a_configuration_without_the_record_has_the_layout_it_had(hip_lib):
    """the public ten-int configuration describes what it described: the section list and record length of every subsystem switched on, as the commit
    before this feature laid them out (ids 1 .. 20, no DRED_DEC)"""
    from lpcnet_amd import api
    lay = api.snapshot_layout(dict(analysis=1, encoder=1, keep=1, plc=1, plc_options=1, g1=64, g2=32, dred_enc_floats=1000, dred_enc_dframes=3))
    assert [s[0] for s in lay["sections"]] == list(range(1, 21)) and api.SNAP["DRED_DEC"] not in [s[0] for s in lay["sections"]]
    assert lay == BEFORE_LAYOUT, lay
    bare = api.snapshot_layout({})
    assert bare == BEFORE_BARE, bare


# api.snapshot_layout of those two configurations on the commit before this feature
BEFORE_LAYOUT = {"sections": [(1, 3592, 0), (2, 72, 3600), (3, 3924, 3680), (4, 72, 7616), (5, 4608, 7696), (6, 192, 12304), (7, 64, 12496), (8, 4, 12560),
                              (9, 1120, 12576), (10, 80, 13696), (11, 1536, 13776), (12, 16, 15312), (13, 4, 15328), (14, 8000, 15344), (15, 320, 23344),
                              (16, 320, 23664), (17, 144, 23984), (18, 144, 24128), (19, 36, 24272), (20, 4000, 24320)], "record_bytes": 28320}
BEFORE_BARE = {"sections": [(1, 3592, 0), (2, 72, 3600), (8, 4, 3680)], "record_bytes": 3696}
