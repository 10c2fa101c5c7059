"""The encoder's tie rules on the device: codebooks whose entries tie on purpose (tests/tools/encode_ties.py) and the reference's decisions under
them (tests/golden/golden_encode_ties_v1.npz, made by tests/tools/make_golden_encode_ties.py from the generic-C float build).  Equal distances go
to the lower index: in a lane's own sixteen entries, at every step of the wavefront's butterfly (enc_wave_argmin), across the quarters and the
two signs of ceps_codebook_diff4, and in the survivor merge.  A reduction that loses the index order changes these bytes and no others in the suite:
the Gaussian codebooks of synth.make_codebooks never tie."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import encode_large_cases as cases  # noqa: E402
import encode_ties  # noqa: E402
import make_golden_encode as mge  # noqa: E402
import make_golden_encode_ties as mget  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    g = np.load(mget.PATH)
    P = g["packets"].shape[1]
    pcm = np.stack([synth.make_pcm(int(s), 4 * P) for s in g["seeds"]])
    assert [zlib.crc32(p.tobytes()) for p in pcm] == g["pcm_crc32"].tolist()
    return dict(P=P, pcm=pcm, packets=g["packets"], vq_mem=g["vq_mem"], ties=encode_ties.make(int(g["codebook_seed"])))


@pytest.fixture()
def tie_codebooks(gold, hip_lib):
    """the tie codebooks for one test; the suite's usual ones (make_codebooks(5)) afterwards"""
    api.set_codebooks(*gold["ties"]["cbs"])
    yield
    api.set_codebooks(*synth.make_codebooks(mge.CODEBOOK_SEED))


def assert_fixture(b, out, gold):
    bad = out != gold["packets"]
    f_got, f_want = mge.packet_fields(out), mge.packet_fields(gold["packets"])
    assert not bad.any(), (int(bad.any(axis=2).sum()), {k: int((f_got[k] != f_want[k]).sum()) for k in f_got})
    mem = np.stack([b.get_encoder_vq_mem(s) for s in range(out.shape[0])])
    assert np.array_equal(bits(mem), bits(gold["vq_mem"]))


def test_packets_and_vq_mem_equal_the_tie_fixture_in_one_call(gold, blob_f32, tie_codebooks):
    b = api.LPCNetBatch(gold["pcm"].shape[0], blob_f32)
    assert_fixture(b, b.encode(gold["pcm"]), gold)
    b.close()


def test_packets_and_vq_mem_equal_the_tie_fixture_in_calls_of_1_and_3_packets(gold, blob_f32, tie_codebooks):
    b = api.LPCNetBatch(gold["pcm"].shape[0], blob_f32)
    out, p = [], 0
    while p < gold["P"]:
        for step in (1, 3):
            out.append(b.encode(gold["pcm"][:, p * 640:(p + step) * 640]))
            p += step
    assert p == gold["P"]
    assert_fixture(b, np.concatenate(out, axis=1), gold)
    b.close()


def test_codebooks_installed_after_a_batch_exists_reach_its_device_tables(gold, blob_f32, hip_lib):
    """one batch: the usual codebooks and their fixture, then the tie codebooks and theirs, then back"""
    usual = np.load(mge.PATH)
    P = 8
    upcm = np.stack([synth.make_pcm(int(s), 4 * usual["packets"].shape[1])[:P * 640] for s in usual["seeds"]])
    usual_cbs = synth.make_codebooks(mge.CODEBOOK_SEED)
    b = api.LPCNetBatch(6, blob_f32)
    try:
        for cbs, pcm, want in ((usual_cbs, upcm, usual["packets"]), (gold["ties"]["cbs"], gold["pcm"][:, :P * 640], gold["packets"]), (usual_cbs, upcm, usual["packets"])):
            api.set_codebooks(*cbs)
            b.analysis_reset()
            assert np.array_equal(b.encode(pcm), want[:, :P])
    finally:
        api.set_codebooks(*usual_cbs)
        b.close()


def test_ties_in_every_slot_of_a_wavefront_and_a_ragged_last_workgroup(gold, blob_f32, tie_codebooks):
    """the ragged-at-3 case of tests/test_gpu_encode_large.py under the tie codebooks: 2 047 active streams x 8 packets, three items per wavefront
    in vq_end and two in vq_mid, against batches of 256 streams (one item per wavefront, the form the tie fixture pins)"""
    active, P, plan = cases.ENCODE["ragged3"]
    assert api.encode_plan(cases.N, active, P) == plan and (plan[0]["ipw_end"], plan[0]["ipw_mid"], plan[0]["last_end"], plan[0]["last_mid"]) == (3, 2, 8, 8)
    pcm = np.array(cases.big_pcm()[:, :P * 640])
    for k, s in enumerate(cases.GOLD_AT):                                       # the tie fixture's streams in place of the usual fixture's
        pcm[s] = gold["pcm"][k, :P * 640]
    assert len({row.tobytes() for row in pcm}) == cases.N
    small = api.LPCNetBatch(cases.SMALL, blob_f32)
    want, want_mem = [], []
    for k in range(0, cases.N, cases.SMALL):
        small.analysis_reset()
        want.append(small.encode(pcm[k:k + cases.SMALL]))
        want_mem.append(np.stack([small.get_encoder_vq_mem(s) for s in range(cases.SMALL)]))
    small.close()
    want, want_mem = np.concatenate(want), np.concatenate(want_mem)
    assert np.array_equal(want[list(cases.GOLD_AT)], gold["packets"][:, :P])
    c = encode_ties.census(want[:active], gold["ties"])
    assert c["e0_lowest"] == c["e1_lowest"] == c["e2_lowest"] == active * P and min(c["kinds"].values()) >= 10, c
    big = api.LPCNetBatch(cases.N, blob_f32)
    big.active = active
    out = big.encode(pcm)
    at = [s for s in cases.GOLD_AT if s < active]
    assert np.array_equal(out[at], gold["packets"][[cases.GOLD_AT.index(s) for s in at], :P])
    bad = np.flatnonzero((out[:active] != want[:active]).any(axis=(1, 2)))
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    mem = np.stack([big.get_encoder_vq_mem(s) for s in range(active)])
    assert np.array_equal(bits(mem), bits(want_mem[:active]))
    big.close()
