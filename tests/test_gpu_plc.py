"""Batched packet-loss concealment on the device against the reference's generic-C float build (tests/golden/golden_plc_v1.npz, made by
tests/tools/make_golden_plc.py from lpcnet_plc_update / lpcnet_plc_conceal driven stream by stream).  All comparisons on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from plc_run import run  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_v1.npz"))


@pytest.fixture(scope="module")
def blob_plc():
    return synth.blob_bytes(plc_synth.make_model_with_plc())


@pytest.fixture(scope="module")
def pcm_in(gold):
    pcm = np.stack([pm.stream_pcm(s) for s in range(pm.N_STREAMS)])
    assert np.uint32(zlib.crc32(pcm.tobytes())) == gold["in_crc"]
    return pcm


B = pm.BLOCK          # the fixture checks output per block of 10 frames (plc_model.block_crc)


def test_refusals(blob_f32, blob_plc, hip_lib):
    b = api.LPCNetBatch(2, blob_f32)
    for call in (lambda: b.plc_enable(api.PLC_CAUSAL), lambda: b.plc_step(np.zeros((2, 160), np.int16), [0, 0]), lambda: b.plc_reset(),
                 lambda: b.get_plc_state(0), lambda: b.plc_burg(np.zeros((2, 160), np.float32))):
        with pytest.raises(api.LPCNetError, match=r"\(-5\)"):
            call()
    b.close()
    b = api.LPCNetBatch(2, blob_plc)
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.plc_enable(api.PLC_NONCAUSAL)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.plc_step(np.zeros((2, 160), np.int16), [0, 0])
    b.close()
    # a float LPCNet model whose PLC arrays are int8: the model loads, the PLC is refused
    mixed = synth.make_model(flavour="float")
    rng = np.random.default_rng(1)
    mixed.add("plc_dense1_weights", (rng.standard_normal((57, 128)) * 0.1).astype(np.float32), synth.WEIGHT_TYPE_FLOAT)
    mixed.add("plc_dense1_bias", np.zeros(128, np.float32), synth.WEIGHT_TYPE_FLOAT)
    plc_synth._gru(mixed, "plc_gru1", rng, 128, 16, "int8")
    plc_synth._gru(mixed, "plc_gru2", rng, 16, 16, "int8")
    mixed.add("plc_out_weights", np.zeros((16, 20), np.float32), synth.WEIGHT_TYPE_FLOAT)
    mixed.add("plc_out_bias", np.zeros(20, np.float32), synth.WEIGHT_TYPE_FLOAT)
    b = api.LPCNetBatch(2, synth.blob_bytes(mixed))
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*int8"):
        b.plc_enable(api.PLC_CAUSAL)
    b.close()


def test_burg_cepstra_equal_the_reference(gold, blob_plc, hip_lib):
    frames = pm.burg_frames()
    b = api.LPCNetBatch(frames.shape[0], blob_plc)
    b.plc_enable(api.PLC_CAUSAL)
    got = b.plc_burg(frames)
    assert np.array_equal(got.view(np.uint32), gold["burg"].view(np.uint32)), np.argwhere(got.view(np.uint32) != gold["burg"].view(np.uint32))[:8]
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.plc_burg(frames + np.float32(0.5))
    b.close()


def test_prediction_equals_the_reference_at_16_and_the_restatement_at_256(gold, blob_plc, hip_lib):
    xs = pm.pred_inputs()
    b = api.LPCNetBatch(3, blob_plc)
    b.plc_enable(api.PLC_CAUSAL)
    got = np.stack([b.plc_pred(np.repeat(x[None], 3, 0)) for x in xs])          # [steps][3][20]: three streams, the same trace
    for s in range(3):
        assert np.array_equal(got[:, s].view(np.uint32), gold["pred"].view(np.uint32))
    b.close()
    blob = pm.blob_256()
    net = pm.PlcNetNumpy(blob)
    assert (net.d1, net.g1, net.g2) == (128, 256, 256)
    want = np.stack([net.pred(x) for x in xs[:12]])
    b = api.LPCNetBatch(2, blob)
    b.plc_enable(api.PLC_CODEC)
    got = np.stack([b.plc_pred(np.repeat(x[None], 2, 0)) for x in xs[:12]])
    assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[:, 1].view(np.uint32), want.view(np.uint32))
    # and the whole step runs on that network
    out = b.plc_step(pm.stream_pcm(1, 2), [0, 1])
    assert out.shape == (2, 160)
    b.close()


@pytest.mark.parametrize("k", range(4))
def test_end_to_end_against_the_reference(k, gold, blob_plc, pcm_in, hip_lib):
    opt = pm.OPTION_SETS[k]
    lost = pm.loss_patterns()
    b = api.LPCNetBatch(pm.N_STREAMS, blob_plc)
    b.plc_enable(opt)
    out = run(b, pcm_in, lost)
    b.close()
    f0, f1 = pm.FULL_FRAMES
    bad = np.argwhere(out[pm.FULL_STREAM, f0:f1] != gold["pcm_full"][k])
    assert bad.size == 0, "options %d stream %d from frame %d: first differing (frame, sample) %s of %d" % (opt, pm.FULL_STREAM, f0, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["pcm_crc"][k])
    assert bad.size == 0, "options %d: first differing (stream, block of %d frames) %s of %d" % (opt, B, bad[:6].tolist(), len(bad))
    assert (out[lost.astype(bool)] != 0).mean() > 0.5          # the concealment is not silence


def test_fec_schedules_against_the_reference(gold, blob_plc, pcm_in, hip_lib):
    ops, vec = pm.fec_schedule()
    lost = pm.fec_loss_patterns()
    n = 16                                            # the FEC streams and eight without a schedule
    b = api.LPCNetBatch(n, blob_plc)
    b.plc_enable(api.PLC_CAUSAL)
    out = run(b, pcm_in, lost, ops=ops, vec=vec)
    b.close()
    f0, f1 = pm.FEC_FULL_FRAMES
    bad = np.argwhere(out[pm.FEC_FULL_STREAM, f0:f1] != gold["fec_full"])
    assert bad.size == 0, "stream %d from frame %d: first differing (frame, sample) %s of %d" % (pm.FEC_FULL_STREAM, f0, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["fec_crc"][:n])
    assert bad.size == 0, bad[:6].tolist()


def test_a_stream_alone_among_others_and_on_either_shard(gold, blob_plc, pcm_in, hip_lib):
    lost = pm.loss_patterns()
    T = 60
    for s in (7, 9):
        want = gold["pcm_crc"][0][s, :T // B]
        b = api.LPCNetBatch(1, blob_plc)
        b.plc_enable(api.PLC_CAUSAL)
        assert np.array_equal(pm.block_crc(run(b, pcm_in, lost, 0, T, streams=[s]))[0], want)
        b.close()
    b = api.LPCNetBatch(8, blob_plc, devices=[0, 0])
    assert len(b.shards) == 2
    b.plc_enable(api.PLC_CAUSAL)
    order = [7, 3, 9, 1, 4, 7, 9, 20]                 # streams 7 and 9 on both shards
    got = pm.block_crc(run(b, pcm_in, lost, 0, T, streams=order))
    b.close()
    for i, s in enumerate(order):
        assert np.array_equal(got[i], gold["pcm_crc"][0][s, :T // B]), (i, s)


def test_reset_and_rollback(gold, blob_plc, pcm_in, hip_lib):
    lost = pm.loss_patterns()
    streams = [3, 6, 7, 9]
    b = api.LPCNetBatch(4, blob_plc)
    b.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    head = run(b, pcm_in, lost, 0, 40, streams=streams)
    b.plc_reset(1, 2)                                 # streams 1, 2 of the batch start over; 0 and 3 go on
    tail = run(b, pcm_in[:, 40:], lost[:, 40:], 0, 50, streams=streams)
    fresh = api.LPCNetBatch(4, blob_plc)
    fresh.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    new = run(fresh, pcm_in[:, 40:], lost[:, 40:], 0, 50, streams=streams)
    fresh.close()
    assert np.array_equal(tail[1:3], new[1:3])
    want = gold["pcm_crc"][2]
    got = pm.block_crc(np.concatenate([head, tail], axis=1))
    assert np.array_equal(got[0], want[3, :9]) and np.array_equal(got[3], want[9, :9]) and np.array_equal(got[1, :4], want[6, :4])
    # snapshot of stream 0 (PLC, synthesis and analysis state), 20 more frames, roll back, the same 20 frames again
    L = b.L
    import ctypes as C
    raw = C.create_string_buffer(L.lpcnet_batch_state_size())
    assert L.lpcnet_batch_get_raw_state(b.p, 0, raw) == 0
    snap = (b.get_plc_state(0), raw.raw, b.get_analysis_state(0))
    first = run(b, pcm_in[:, 90:], lost[:, 90:], 0, 20, streams=streams)
    b.set_plc_state(0, snap[0])
    assert L.lpcnet_batch_set_raw_state(b.p, 0, C.create_string_buffer(snap[1], len(snap[1]))) == 0
    b.set_analysis_state(0, snap[2])
    again = run(b, pcm_in[:, 90:], lost[:, 90:], 0, 20, streams=streams)
    assert np.array_equal(first[0], again[0]) and np.array_equal(pm.block_crc(first[:1])[0], want[3, 9:11])
    bad = bytearray(snap[0])
    bad[0:4] = (123).to_bytes(4, "little")            # pcm_fill the state machine cannot reach
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.set_plc_state(0, bytes(bad))
    b.close()


def test_reset_across_a_shard_boundary(gold, blob_plc, pcm_in, hip_lib):
    """the reset half of test_reset_and_rollback on two shards of two streams each: plc_reset(1, 2) takes the last stream of the first shard and
    the first stream of the second"""
    lost = pm.loss_patterns()
    streams = [3, 6, 7, 9]
    b = api.LPCNetBatch(4, blob_plc, devices=[0, 0])
    assert b.shards == [(0, 2, 0), (2, 2, 0)]
    b.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    head = run(b, pcm_in, lost, 0, 40, streams=streams)
    b.plc_reset(1, 2)                                 # streams 1, 2 of the batch start over; 0 and 3 go on
    tail = run(b, pcm_in[:, 40:], lost[:, 40:], 0, 50, streams=streams)
    b.close()
    fresh = api.LPCNetBatch(4, blob_plc)
    fresh.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    new = run(fresh, pcm_in[:, 40:], lost[:, 40:], 0, 50, streams=streams)
    fresh.close()
    assert np.array_equal(tail[1:3], new[1:3])
    want = gold["pcm_crc"][2]
    got = pm.block_crc(np.concatenate([head, tail], axis=1))
    assert np.array_equal(got[0], want[3, :9]) and np.array_equal(got[3], want[9, :9]) and np.array_equal(got[1, :4], want[6, :4])


def test_device_pointer_step_and_capture_refusal(gold, blob_plc, pcm_in, hip_lib):
    import torch
    dev = torch.device("cuda:0")
    lost = pm.loss_patterns()
    n, T = 12, 40
    b = api.LPCNetBatch(n, blob_plc)
    b.plc_enable(api.PLC_CODEC)
    b.tune()
    d = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    out = np.zeros((n, T, 160), np.int16)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for t in range(T):
            frame = np.ascontiguousarray(pcm_in[:n, t])
            frame[lost[:n, t] != 0] = 0
            d.copy_(torch.from_numpy(frame))
            b.plc_step_device(d.data_ptr(), lost[:n, t], s.cuda_stream)
            out[:, t] = d.cpu().numpy()
    assert np.array_equal(pm.block_crc(out), gold["pcm_crc"][1][:n, :T // B])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.plc_step_device(d.data_ptr(), lost[:n, 0], cs)
        d.add_(0)                                     # (the capture stays usable and is not empty)
    b.sync()
    b.close()


def test_device_pointer_step_on_eight_streams_per_workgroup(gold, blob_plc, pcm_in, hip_lib):
    """the enqueue-only step on a caller's stream with the form pinned (the test above runs whatever tune() measured): the two-group kernel"""
    import torch
    lost = pm.loss_patterns()
    n, T = 12, 40
    b = api.LPCNetBatch(n, blob_plc)
    b.streams_per_workgroup = 8
    b.twelve_waves = 0
    b.plc_enable(api.PLC_CODEC)
    d = torch.zeros((n, 160), dtype=torch.int16, device=torch.device("cuda:0"))
    s = torch.cuda.Stream()
    out = np.zeros((n, T, 160), np.int16)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for t in range(T):
            frame = np.ascontiguousarray(pcm_in[:n, t])
            frame[lost[:n, t] != 0] = 0
            d.copy_(torch.from_numpy(frame))
            b.plc_step_device(d.data_ptr(), lost[:n, t], s.cuda_stream)
            out[:, t] = d.cpu().numpy()
    assert b.streams_per_workgroup == 8 and b.twelve_waves == 0
    b.sync()
    b.close()
    bad = np.argwhere(pm.block_crc(out) != gold["pcm_crc"][1][:n, :T // B])
    assert bad.size == 0, "first differing (stream, block of %d frames) %s of %d" % (B, bad[:6].tolist(), len(bad))


def test_a_batch_without_plc_is_as_before(blob_plc, hip_lib):
    """the PLC arrays in the blob change nothing for a batch that never enables the PLC"""
    from oracle import orc
    feats = np.stack([synth.make_features(900 + s, 4) for s in range(3)])
    ref = np.stack([orc.OracleModel(blob_plc).new_state().synthesize(feats[s]) for s in range(3)])
    b = api.LPCNetBatch(3, blob_plc)
    assert np.array_equal(b.synthesize(feats), ref)
    b.close()
