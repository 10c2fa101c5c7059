"""The encoder (lpcnet_batch_encode*, lpcnet_batch_compute_features*), the parts that need no GPU: the C-ABI surface, the Python
surface, the fixture and its generator, and the compiler's resource figures of the encoder kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_resources  # noqa: E402
import encode_ties  # noqa: E402
import make_golden_encode as mge  # noqa: E402
import make_golden_encode_ties as mget  # noqa: E402
from lpcnet_amd import api  # noqa: E402

CSRC = os.path.join(ROOT, "lpcnet_amd", "csrc")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")
NEW_SYMBOLS = ("lpcnet_batch_encode", "lpcnet_batch_encode_device", "lpcnet_batch_encode_device_shard", "lpcnet_batch_compute_features",
               "lpcnet_batch_compute_features_device", "lpcnet_batch_encoder_enable", "lpcnet_batch_get_encoder_vq_mem",
               "lpcnet_batch_set_encoder_vq_mem")


def test_new_entry_points_are_declared_and_exported_and_no_reference_encoder_name_is(hip_lib):
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW_SYMBOLS:
        assert re.search(r"LPCNET_EXPORT int " + n + r"\(", header), n
        assert n in exported, n
    assert not [s for s in exported if s.startswith(("lpcnet_encoder_", "lpcnet_compute_", "lpcnet_encode"))]
    assert not [s for s in exported if s.startswith("lpcn_")]
    assert hip_lib.lpcnet_batch_analysis_state_size() == 3924                    # vq_mem lives beside the analysis state, not in it
    assert "pcount" in header and "stale" in header                              # the one quirk that is not reproduced is stated
    assert "getenv" not in open(os.path.join(CSRC, "encode_kernels.hip.h")).read()


def test_python_surface():
    for m in ("encode", "encode_device", "encode_device_shard", "compute_features", "compute_features_device", "encoder_enable",
              "get_encoder_vq_mem", "set_encoder_vq_mem"):
        assert callable(getattr(api.LPCNetBatch, m)), m


def test_the_fixture_is_well_formed_and_not_degenerate():
    g = np.load(mge.PATH)
    S, P = g["packets"].shape[:2]
    assert S >= 4 and P >= 60 and g["packets"].shape == (S, P, 8) and g["packets"].dtype == np.uint8
    assert g["features"].shape == (S, 4 * P, 36) and g["features"].dtype == np.float32 and np.isfinite(g["features"]).all()
    assert int(g["codebook_seed"]) == mge.CODEBOOK_SEED and g["seeds"].tolist() == list(mge.SEEDS)
    cov = mge.coverage(g["packets"])
    assert mge.is_rich(cov), cov
    f = mge.packet_fields(g["packets"])
    assert sum(int(f[k].max()).bit_length() for k in ("c0", "pitch", "mod", "corr", "e0", "e1", "e2", "mid", "interp")) <= 64
    assert all(len(set(f[k].reshape(-1).tolist())) >= 40 for k in ("c0", "pitch", "e0", "e1", "e2", "mid")) and f["interp"].max() <= 7


def test_the_fixture_regenerates_identically_from_the_compiled_reference():
    if not os.path.exists(REF_LIB):
        pytest.skip("compiled reference absent (make -C oracle ref)")
    g, fresh = np.load(mge.PATH), mge.generate()
    assert sorted(g.files) == sorted(fresh)
    for k in g.files:
        a, b = np.asarray(g[k]), np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_the_tie_fixture_shows_the_reference_deciding_every_tie_by_the_lower_index():
    """tests/golden/golden_encode_ties_v1.npz (codebooks of tests/tools/encode_ties.py): the conditions its generator refuses to write without.
    Recorded, not required: a zero row of ceps_codebook_diff4 never won; in 251 of the 384 packets double_interp_search passed over the forbidden
    id 7 although it was the nearest (recomputed by encode_ties.interp_census, which reproduces every interp id of the fixture)"""
    g = np.load(mget.PATH)
    S, P = g["packets"].shape[:2]
    assert (S, P) == (6, 64) and g["packets"].dtype == np.uint8 and g["vq_mem"].shape == (S, 18) and g["vq_mem"].dtype == np.float32
    assert int(g["codebook_seed"]) == encode_ties.SEED and g["seeds"].tolist() == list(mget.SEEDS)
    ties = encode_ties.make(int(g["codebook_seed"]))
    for s in range(3):                                                           # every vector at four positions
        cb, group = ties["cbs"][s], ties["groups"][s]
        assert cb.shape == (1024, 17) and all(len({cb[i].tobytes() for i in np.flatnonzero(group == k)}) == 1 for k in range(256))
        assert len({cb[i].tobytes() for i in range(1024)}) == 256
        assert all(v >= 40 for v in encode_ties.placement_census(group).values())
    c = encode_ties.census(g["packets"], ties)
    assert encode_ties.conditions(c) == [], c
    assert c["packets"] == S * P and all(v >= 10 for v in c["kinds"].values()) and c["mid_first_of_equal_pair"] >= 10
    assert c["mid_zero_row"] == int(g["zero_row_winners"]) == 0 and c["interp_ids"] == list(range(8))
    assert int(g["forbidden_id7"]) == 251
    # the final vq_mem is the last packet's quantised frame 3
    f = mge.packet_fields(g["packets"][:, -1])
    cb1, cb2, cb3, _ = ties["cbs"]
    assert np.array_equal(g["vq_mem"][:, 0], ((f["c0"] - 64) / 4.0).astype(np.float32))
    assert np.array_equal(g["vq_mem"][:, 1:], (cb1[f["e0"]] + cb2[f["e1"]]) + cb3[f["e2"]])


def test_the_tie_fixture_regenerates_identically_from_the_compiled_reference():
    if not os.path.exists(REF_LIB):
        pytest.skip("compiled reference absent (make -C oracle ref)")
    g, fresh = np.load(mget.PATH), mget.generate()
    assert sorted(g.files) == sorted(fresh)
    for k in g.files:
        a, b = np.asarray(g[k]), np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_encoder_kernels_compile_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources.engine_kernel_resources(kernel_resources.ENCODE_PATTERN, asm_path=str(tmp_path / "engine.s"))
    assert set(res) == {"encode_pitch_kernelILb0E", "encode_pitch_kernelILb1E", "encode_vq_end_kernel", "encode_vq_mid_kernel"}
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] % 64 == 0 and r["vgpr"] <= 128, (name, r)
    # both VQ kernels stage a codebook in LDS and still fit two workgroups into a CU's 160 KB
    assert all(65536 < res[k]["lds"] <= 81920 for k in ("encode_vq_end_kernel", "encode_vq_mid_kernel")), res
    # the analysis kernels the encoder launches are the analysis' own
    an = kernel_resources.engine_kernel_resources(asm_path=str(tmp_path / "engine.s"))
    assert all(r["scratch"] == 0 and r["vgpr_spill"] == 0 for r in an.values()) and len(an) == 3
