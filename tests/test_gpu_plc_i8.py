"""Batched packet-loss concealment of an int8 (DOT_PROD) model on the device against the reference's generic-C int8 build
(tests/golden/golden_plc_i8_v1.npz, made by tests/tools/make_golden_plc_i8.py from lpcnet_plc_update / lpcnet_plc_conceal driven stream by
stream) and against the NumPy restatement of its PLC network (tests/tools/plc_i8_model.py).  All comparisons on bit patterns."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_i8_model as pq  # noqa: E402
import plc_synth  # noqa: E402
from plc_run import run  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

B = pm.BLOCK


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_i8_v1.npz"))


@pytest.fixture(scope="module")
def blob_plc_i8(gold):
    blob = synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))
    assert np.uint32(zlib.crc32(blob)) == gold["blob_crc"]
    return blob


@pytest.fixture(scope="module")
def pcm_in(gold):
    pcm = np.stack([pm.stream_pcm(s) for s in range(pm.N_STREAMS)])
    assert np.uint32(zlib.crc32(pcm.tobytes())) == gold["in_crc"]
    return pcm


def _pred_trace(blob, n, xs, options=api.PLC_CAUSAL):
    b = api.LPCNetBatch(n, blob)
    b.plc_enable(options)
    got = np.stack([b.plc_pred(np.repeat(x[None], n, 0)) for x in xs])          # [steps][n][20]: every stream the same trace
    b.close()
    return got


def test_prediction_equals_the_reference_at_16(gold, blob_plc_i8, hip_lib):
    got = _pred_trace(blob_plc_i8, 3, pm.pred_inputs())
    for s in range(3):
        bad = np.argwhere(got[:, s].view(np.uint32) != gold["pred"].view(np.uint32))
        assert bad.size == 0, "stream %d: first differing (step, feature) %s of %d" % (s, bad[:4].tolist(), len(bad))


def test_prediction_equals_the_restatement_at_256(hip_lib):
    """the trained PLC model's width: every lane of the workgroup owns one GRU unit (three gate rows), 64 packed input dwords into GRU 2"""
    xs = pm.pred_inputs()[:12]
    blob = pq.blob_256_i8()
    net = pq.PlcNetNumpyI8(blob)
    assert (net.d1, net.g1, net.g2) == (128, 256, 256)
    want = np.stack([net.pred(x) for x in xs])
    got = _pred_trace(blob, 2, xs, api.PLC_CODEC)
    for s in range(2):
        bad = np.argwhere(got[:, s].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, "stream %d: first differing (step, feature) %s of %d" % (s, bad[:4].tolist(), len(bad))


def test_prediction_equals_the_restatement_beyond_the_workgroup_size(hip_lib):
    """128 / 512 / 264: units looped over the 256 lanes -- GRU 1 with two units on every lane, GRU 2 with a second pass of eight -- the full 128
    packed dwords into GRU 2, and g1 != g2 in the state record"""
    xs = pm.pred_inputs()[:8]
    blob = pq.blob_wide_i8()
    net = pq.PlcNetNumpyI8(blob)
    assert (net.d1, net.g1, net.g2) == (128, 512, 264)
    want = np.stack([net.pred(x) for x in xs])
    got = _pred_trace(blob, 2, xs)
    for s in range(2):
        bad = np.argwhere(got[:, s].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, "stream %d: first differing (step, feature) %s of %d" % (s, bad[:4].tolist(), len(bad))


def test_prediction_with_missing_input_blocks_equals_the_restatement(hip_lib):
    """GRU 1's index lists with a row group of no blocks, one of a single block, the others irregular"""
    xs = pm.pred_inputs()[:20]
    blob = pq.blob_sparse_i8()
    counts = pq.group_counts(np.frombuffer(pm.blob_arrays(blob)["plc_gru1_weights_idx"], np.int32), 6)
    assert counts[0] == 0 and counts[1] == 1 and all(0 < c < 32 for c in counts[2:]), counts
    net = pq.PlcNetNumpyI8(blob)
    want = np.stack([net.pred(x) for x in xs])
    got = _pred_trace(blob, 2, xs)
    for s in range(2):
        bad = np.argwhere(got[:, s].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, "stream %d: first differing (step, feature) %s of %d" % (s, bad[:4].tolist(), len(bad))


@pytest.mark.parametrize("k", range(4))
def test_end_to_end_against_the_reference(k, gold, blob_plc_i8, pcm_in, hip_lib):
    opt = pm.OPTION_SETS[k]
    lost = pm.loss_patterns()
    b = api.LPCNetBatch(pm.N_STREAMS, blob_plc_i8)
    b.plc_enable(opt)
    out = run(b, pcm_in, lost)
    b.close()
    f0, f1 = pm.FULL_FRAMES
    bad = np.argwhere(out[pm.FULL_STREAM, f0:f1] != gold["pcm_full"][k])
    if bad.size:
        fr = int(bad[0][0])
        print("options %d stream %d frame %d:\n got  %s\n want %s" % (opt, pm.FULL_STREAM, f0 + fr, out[pm.FULL_STREAM, f0 + fr].tolist(), gold["pcm_full"][k][fr].tolist()))
    assert bad.size == 0, "options %d stream %d from frame %d: first differing (frame, sample) %s of %d" % (opt, pm.FULL_STREAM, f0, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["pcm_crc"][k])
    assert bad.size == 0, "options %d: first differing (stream, block of %d frames) %s of %d" % (opt, B, bad[:6].tolist(), len(bad))
    assert (out[lost.astype(bool)] != 0).mean() > 0.5          # the concealment is not silence


def test_fec_schedules_against_the_reference(gold, blob_plc_i8, pcm_in, hip_lib):
    ops, vec = pm.fec_schedule()
    lost = pm.fec_loss_patterns()
    n = 16                                            # the FEC streams and eight without a schedule
    b = api.LPCNetBatch(n, blob_plc_i8)
    b.plc_enable(api.PLC_CAUSAL)
    out = run(b, pcm_in, lost, ops=ops, vec=vec)
    b.close()
    f0, f1 = pm.FEC_FULL_FRAMES
    bad = np.argwhere(out[pm.FEC_FULL_STREAM, f0:f1] != gold["fec_full"])
    if bad.size:
        fr = int(bad[0][0])
        print("stream %d frame %d:\n got  %s\n want %s" % (pm.FEC_FULL_STREAM, f0 + fr, out[pm.FEC_FULL_STREAM, f0 + fr].tolist(), gold["fec_full"][fr].tolist()))
    assert bad.size == 0, "stream %d from frame %d: first differing (frame, sample) %s of %d" % (pm.FEC_FULL_STREAM, f0, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["fec_crc"][:n])
    assert bad.size == 0, bad[:6].tolist()


def test_snapshot_and_rollback_mid_burst(gold, blob_plc_i8, pcm_in, hip_lib):
    lost = pm.loss_patterns()
    streams = [3, 6, 7, 9]
    b = api.LPCNetBatch(4, blob_plc_i8)
    b.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    head = run(b, pcm_in, lost, 0, 85, streams=streams)          # stream 6 (row 1) is five frames into its burst of 15
    assert lost[6, 80:85].all() and lost[6, 85:95].all()
    L = b.L
    raw = C.create_string_buffer(L.lpcnet_batch_state_size())
    assert L.lpcnet_batch_get_raw_state(b.p, 1, raw) == 0
    snap = (b.get_plc_state(1), raw.raw, b.get_analysis_state(1))
    first = run(b, pcm_in, lost, 85, 95, streams=streams)
    b.set_plc_state(1, snap[0])
    assert L.lpcnet_batch_set_raw_state(b.p, 1, C.create_string_buffer(snap[1], len(snap[1]))) == 0
    b.set_analysis_state(1, snap[2])
    again = run(b, pcm_in, lost, 85, 95, streams=streams)
    b.close()
    assert np.array_equal(first[1], again[1]) and first[1].any()
    # and both are what the reference gives: frames 0 .. 90 of stream 6 in blocks of ten
    got = pm.block_crc(np.concatenate([head, first], axis=1)[:, :90])
    assert np.array_equal(got[1], gold["pcm_crc"][2][6, :9])


def test_flavour_call_and_mixed_flavour_refusal(blob_plc_i8, hip_lib):
    b = api.LPCNetBatch(2, blob_plc_i8)
    with pytest.raises(api.LPCNetError, match=r"\(-5\)"):
        b.plc_flavour()                               # before plc_enable
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_flavour() == 1
    b.close()
    b = api.LPCNetBatch(2, synth.blob_bytes(plc_synth.make_model_with_plc()))
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_flavour() == 0
    b.close()
    # an int8 LPCNet model whose PLC arrays are float: the model loads, the PLC is refused
    mixed = pq.model_with_plc("int8", "float")
    b = api.LPCNetBatch(2, synth.blob_bytes(mixed))
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*float.*int8"):
        b.plc_enable(api.PLC_CAUSAL)
    pcm = b.synthesize(np.stack([synth.make_features(900 + s, 6) for s in range(2)]))          # (the batch still synthesises: the first frames are silence by
    assert pcm.shape == (2, 6 * 160) and pcm[:, 3 * 160:].any()                                  # the reference's feature delay, src/lpcnet.c:239, the later ones are not)
    b.close()
