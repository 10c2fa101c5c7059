"""The packet unpacker's two CPU copies against the reference, no GPU needed: orc_decode_packet (the oracle) and packet_to_features (what
lpcnet_decode runs, through lpcnet_hip_packet_features) equal the fixture tests/golden/golden_decode_v1.npz -- decode_packet of the
reference's generic-C float build over the field census of tests/tools/decode_census.py and over a real encoder's packets -- on the bit
patterns of every float, tolerance 0.  Also the census' coverage predicate, which is what makes the fixture worth comparing with."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import decode_census as dc  # noqa: E402
import make_golden_decode as mgd  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(mgd.PATH))
    g["packets"] = dc.packets()
    assert dc.crc32(g["packets"]) == int(g["packets_crc32"]), "tests/tools/decode_census.py no longer generates the packets of the fixture"
    g["enc_packets"] = np.load(mgd.ENC_PATH)["packets"]
    g["cbs"] = synth.make_codebooks(int(g["codebook_seed"]))
    return g


def chains(step, pk):
    """step(packet (8,), vq_mem (18,) in place) -> (4, >= 20) along every chain of pk from a zero memory: (features (s, P, 4, 20), memories (s, 18))"""
    feats, mems = np.zeros(pk.shape[:2] + (4, 20), np.float32), np.zeros((pk.shape[0], 18), np.float32)
    for s in range(pk.shape[0]):
        for p in range(pk.shape[1]):
            row = step(np.ascontiguousarray(pk[s, p]), mems[s])
            assert not row[:, 20:].any()
            feats[s, p] = row[:, :20]
    return feats, mems


def check(step, gold):
    got, mems = chains(step, gold["packets"])
    assert not dc.differences(got, gold["features"], gold["packets"])
    assert np.array_equal(mems.view(np.uint32), gold["vq_mem"].view(np.uint32))
    enc = gold["enc_packets"]
    got, _ = chains(step, enc)
    rows = got.reshape(enc.shape[0], -1, 20)
    k = int(gold["enc_stream"])
    assert not dc.differences(got[k:k + 1], gold["enc_features"].reshape(1, -1, 4, 20), enc[k:k + 1])
    assert [dc.crc32(r) for r in rows] == gold["enc_features_crc32"].tolist()


def test_the_census_reaches_every_field_value_and_both_pitch_clamps(gold):
    pk = gold["packets"]
    assert pk.shape == (dc.CHAINS, dc.P, 8) == (8, 64, 8)
    cov = dc.coverage(pk, gold["features"])
    assert cov["pitch_mod_pairs"] == 512 and cov["mid_triples"] == 64 and cov["c0_ids"] == 128, cov
    assert cov["corr_voiced"] == cov["corr_unvoiced"] == [0, 1, 2, 3], cov
    assert cov["mid_corners"] == [0, 4095, 4096, 8191] and cov["e_corners"] == [[0, 1023]] * 3, cov
    assert cov["clamp_low"] > 0 and cov["clamp_high"] > 0 and cov["inside"] > 0, cov
    assert cov["clamp_low"] + cov["clamp_high"] + cov["inside"] == 8 * 64 * 4
    assert dc.is_complete(cov)
    c0 = gold["features"][:, :, 3, 0]
    assert c0.min() == -16 and c0.max() == 15.75
    assert np.array_equal(dc.pack(dc.fields(pk)), pk)                             # the field parser and the packer are each other's inverse


def test_the_oracle_equals_the_fixture_on_every_chain_and_on_the_encoder_packets(gold, oracle_lib):
    cbs = [np.ascontiguousarray(c.reshape(-1)) for c in gold["cbs"]]

    def step(packet, mem):
        feats = np.zeros(4 * 36, np.float32)
        oracle_lib.orc_decode_packet(feats, mem, packet, *cbs)
        return feats.reshape(4, 36)
    check(step, gold)


def test_the_host_unpacker_equals_the_fixture_on_every_chain_and_on_the_encoder_packets(gold, hip_lib):
    api.set_codebooks(*gold["cbs"])
    check(api.packet_features, gold)


def test_the_host_entry_point_checks_its_arguments_and_the_new_names_are_exported(hip_lib):
    api.set_codebooks(*synth.make_codebooks(5))
    pk, mem, out = np.zeros(8, np.uint8), np.zeros(18, np.float32), np.zeros(4 * 36, np.float32)
    assert hip_lib.lpcnet_hip_packet_features(pk, mem, out) == 0
    import ctypes as C
    f = hip_lib.lpcnet_hip_packet_features
    saved, f.argtypes = f.argtypes, [C.c_void_p] * 3
    try:
        assert f(None, mem.ctypes.data, out.ctypes.data) == -4 and "bad arguments" in api.last_error()
        assert f(pk.ctypes.data, None, out.ctypes.data) == -4 and f(pk.ctypes.data, mem.ctypes.data, None) == -4
    finally:
        f.argtypes = saved
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    exported = [ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True).splitlines() if ln.strip()]
    for name in ("lpcnet_batch_run_decode", "lpcnet_hip_packet_features"):
        assert hasattr(hip_lib, name) and name in exported and re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
    assert "packet_to_features" not in exported and not [s for s in exported if s.startswith("lpcn_")]
    assert callable(api.LPCNetBatch.run_decode) and callable(api.packet_features)
