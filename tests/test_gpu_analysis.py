"""Feature analysis on the device (lpcnet_batch_analyze*): lpcnet_compute_single_frame_features per stream and frame, tolerance 0 on
the bit patterns of all 36 floats -- against the reference's generic-C float build (fixture tests/golden/golden_analysis_v1.npz, made by
tests/tools/make_golden_analysis.py; live against oracle/_ref where it exists), across chunkings, resets, shards, batch sizes, the
device-pointer path, a captured graph, and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from lpcnet_amd import api, synth  # noqa: E402
from oracle import orc  # noqa: E402

pytestmark = pytest.mark.gpu
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_analysis_v1.npz"))
    seeds, feats, fs = g["seeds"], g["features"], int(g["float_stream"])
    T = feats.shape[1]
    pcm = np.stack([synth.make_pcm(int(s), T) for s in seeds])
    ints = [k for k in range(len(seeds)) if k != fs]
    return dict(T=T, pcm=pcm[ints], feats=feats[ints], fpcm=(pcm[fs].astype(np.float32) / np.float32(3.0)).astype(np.float32)[None], ffeats=feats[fs][None])


def test_golden_parity_all_columns_one_call(gold, blob_f32, hip_lib):
    b = api.LPCNetBatch(gold["pcm"].shape[0], blob_f32)
    out = b.analyze(gold["pcm"])
    bad = bits(out) != bits(gold["feats"])
    assert not bad.any(), (int(bad.sum()), bad.sum(axis=(0, 1)).tolist())
    b.close()


def test_float_entry_point(gold, blob_f32, hip_lib):
    b = api.LPCNetBatch(1, blob_f32)
    assert same(b.analyze(gold["fpcm"]), gold["ffeats"])                      # non-integer samples against the fixture
    n = gold["pcm"].shape[0]
    b2 = api.LPCNetBatch(n, blob_f32)
    assert same(b2.analyze(gold["pcm"][:, :160 * 40].astype(np.float32)), gold["feats"][:, :40])      # integer-valued floats == shorts
    b.close(); b2.close()


def test_live_reference_on_fresh_seeds(blob_f32, hip_lib):
    if not os.path.exists(REF_LIB):
        pytest.skip("compiled reference absent (make -C oracle ref)")
    import make_golden_analysis as mga
    L = mga.load_ref(REF_LIB)
    T, seeds = 120, list(range(9100, 9108))
    pcm = np.stack([synth.make_pcm(s, T) for s in seeds])
    want = np.stack([mga.ref_features(L, p) for p in pcm])
    b = api.LPCNetBatch(len(seeds), blob_f32)
    assert same(b.analyze(pcm), want)
    fp = (pcm.astype(np.float32) * np.float32(0.37)).astype(np.float32)
    b.analysis_reset()
    assert same(b.analyze(fp), np.stack([mga.ref_features(L, p) for p in fp]))
    b.close()


def test_chunked_calls_and_rollback_equal_one_call(gold, blob_f32, hip_lib):
    pcm, T = gold["pcm"][:, :160 * 75], 75
    n = pcm.shape[0]
    b = api.LPCNetBatch(n, blob_f32)
    for step in (1, 7, 25):
        b.analysis_reset()
        out = np.concatenate([b.analyze(pcm[:, t * 160:min(T, t + step) * 160]) for t in range(0, T, step)], axis=1)
        assert same(out, gold["feats"][:, :T]), step
    # snapshot after 30 frames, run on, roll back, replay
    b.analysis_reset()
    b.analyze(pcm[:, :160 * 30])
    snap = [b.get_analysis_state(s) for s in range(n)]
    first = b.analyze(pcm[:, 160 * 30:])
    for s in range(n):
        b.set_analysis_state(s, snap[s])
    assert same(b.analyze(pcm[:, 160 * 30:]), first) and same(first, gold["feats"][:, 30:T])
    b.close()


def test_resets_and_state_separation(gold, blob_f32, hip_lib):
    pcm = gold["pcm"][:, :160 * 20]
    n = pcm.shape[0]
    b = api.LPCNetBatch(n, blob_f32)
    zero = bytes(b.L.lpcnet_batch_analysis_state_size())
    assert all(b.get_analysis_state(s) == zero for s in range(n))               # lpcnet_encoder_init: all zero
    syn0 = [bytes(b.get_state(s)) for s in range(n)]
    first = b.analyze(pcm)
    assert [bytes(b.get_state(s)) for s in range(n)] == syn0                    # analysis leaves the synthesis state alone
    an = [b.get_analysis_state(s) for s in range(n)]
    assert all(a != zero for a in an)
    b.synthesize(np.stack([synth.make_features(70 + s, 2) for s in range(n)]))
    b.reset()
    assert [b.get_analysis_state(s) for s in range(n)] == an                    # lpcnet_batch_reset leaves the analysis state alone
    b.analysis_reset(1, 2)                                                      # exactly streams 1 and 2 restart
    assert [b.get_analysis_state(s) == zero for s in range(n)] == [s in (1, 2) for s in range(n)]
    second = b.analyze(pcm)
    assert same(second[1:3], first[1:3]) and not same(second[0], first[0]) and not same(second[3:], first[3:])
    b.close()


def test_2048_streams_at_once_and_a_sharded_batch(blob_f32, hip_lib):
    n, T, small = 2048, 3, 64
    pcm = np.stack([synth.make_pcm(20000 + s, T) for s in range(n)])
    big = api.LPCNetBatch(n, blob_f32)
    out = big.analyze(pcm)
    big.close()
    b = api.LPCNetBatch(small, blob_f32)
    for k in range(0, n, small):
        b.analysis_reset()
        assert same(b.analyze(pcm[k:k + small]), out[k:k + small]), k
    b.close()
    sh = api.LPCNetBatch(301, blob_f32, devices=[0, 0])                           # two uneven shards on one device
    assert len(sh.shards) == 2
    got = np.concatenate([sh.analyze(pcm[:301, :160 * 2]), sh.analyze(pcm[:301, 160 * 2:])], axis=1)
    assert same(got, out[:301])
    edge = sh.shards[1][0]
    sh.analysis_reset(edge - 2, 4)                                                # two streams on either side of the shard boundary restart
    again = sh.analyze(pcm[:301, :160 * 2])
    assert same(again[edge - 2:edge + 2], out[edge - 2:edge + 2, :2])
    assert not same(again[edge - 3], out[edge - 3, :2]) and not same(again[edge + 2], out[edge + 2, :2])      # their neighbours went on
    sh.close()


def test_analysis_feeds_synthesis_on_the_device(gold, blob_f32, hip_lib):
    """analyze_device -> synthesize_device on one HIP stream, the [n][T][36] feature buffer never leaving the device, equals the
    reference's analysis (fixture) followed by the oracle's synthesis of those features"""
    import torch
    n, T = gold["pcm"].shape[0], 6
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(n, blob_f32)
    d_in = torch.from_numpy(np.ascontiguousarray(gold["pcm"][:, :160 * T])).to(dev)
    d_feat = torch.zeros((n, T, 36), dtype=torch.float32, device=dev)
    d_out = torch.zeros((n, T * 160), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        b.analyze_device(d_in.data_ptr(), False, d_feat.data_ptr(), 36, T, s.cuda_stream)
        b.synthesize_device(d_feat.data_ptr(), 36, d_out.data_ptr(), T, s.cuda_stream)
    b.sync()
    om = orc.OracleModel(blob_f32)
    want = np.stack([om.new_state().synthesize(np.ascontiguousarray(gold["feats"][k, :T])) for k in range(n)])
    assert same(d_feat.cpu().numpy(), gold["feats"][:, :T])
    assert np.array_equal(d_out.cpu().numpy(), want)
    b.close()


def test_a_linear_capture_of_analysis_and_synthesis_replays_bit_exactly(gold, blob_f32, hip_lib):
    """one real-time step -- analysis of 160 samples, then the synthesis step on its features -- captured as ONE linear chain on one
    stream and replayed; against eager calls on a second batch.  Before the analysis state exists the captured call returns the
    argument error and the capture stays usable."""
    import torch
    n, T = gold["pcm"].shape[0], 4
    dev = torch.device("cuda:0")
    pcm = gold["pcm"]
    eager = api.LPCNetBatch(n, blob_f32)
    want_f, want_p = [], []
    for t in range(T):
        f = eager.analyze(pcm[:, t * 160:(t + 1) * 160])
        want_f.append(f); want_p.append(eager.synthesize(f))
    eager.close()
    b = api.LPCNetBatch(n, blob_f32)
    d_in = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    d_feat = torch.zeros((n, 1, 36), dtype=torch.float32, device=dev)
    d_out = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    got_f, got_p = [], []
    with torch.cuda.stream(s):                                    # frame 0: synthesis eagerly (first launch), analysis state does not exist yet
        d_feat.copy_(torch.from_numpy(want_f[0]))
        b.synthesize_device(d_feat.data_ptr(), 36, d_out.data_ptr(), 1, s.cuda_stream)
        s.synchronize()
    got_f.append(want_f[0]); got_p.append(d_out.cpu().numpy().copy())
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        rc = b.L.lpcnet_batch_analyze_device(b.p, d_in.data_ptr(), 0, d_feat.data_ptr(), 36, 1, cs)
        msg = api.last_error()
        b.synthesize_device(d_feat.data_ptr(), 36, d_out.data_ptr(), 1, cs)      # the capture goes on
    assert rc == -4 and "lpcnet_batch_analysis_enable" in msg
    del g0
    b.analysis_enable(1)
    with torch.cuda.stream(s):                                    # bring the analysis state to frame 1 eagerly (also the kernels' first launch)
        d_in.copy_(torch.from_numpy(np.ascontiguousarray(pcm[:, :160])))
        b.analyze_device(d_in.data_ptr(), False, d_feat.data_ptr(), 36, 1, s.cuda_stream)
        s.synchronize()
    assert same(d_feat.cpu().numpy(), want_f[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        b.analyze_device(d_in.data_ptr(), False, d_feat.data_ptr(), 36, 1, cs)
        b.synthesize_device(d_feat.data_ptr(), 36, d_out.data_ptr(), 1, cs)
    for t in range(1, T):
        d_in.copy_(torch.from_numpy(np.ascontiguousarray(pcm[:, t * 160:(t + 1) * 160])))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got_f.append(d_feat.cpu().numpy().copy()); got_p.append(d_out.cpu().numpy().copy())
    for t in range(T):
        assert same(got_f[t], want_f[t]), t
        assert np.array_equal(got_p[t], want_p[t]), t
    assert b.get_state(0).frame_count == T
    del g
    b.close()


def test_argument_errors(blob_f32, hip_lib):
    L = hip_lib
    b = api.LPCNetBatch(2, blob_f32)
    pcm = np.zeros(2 * 160, np.int16); feat = np.zeros(2 * 36, np.float32)
    assert L.lpcnet_batch_analyze(b.p, pcm, feat, 35, 1) == -4 and "bad arguments" in api.last_error()
    assert L.lpcnet_batch_analyze(b.p, pcm, feat, 36, 0) == -4
    L.lpcnet_batch_analyze_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert L.lpcnet_batch_analyze_device(b.p, None, 0, None, 36, 1, None) == -4
    assert L.lpcnet_batch_analyze_device_shard(b.p, 1, None, 0, None, 36, 1, None) == -4 and "shard" in api.last_error()
    assert L.lpcnet_batch_analysis_reset(b.p, 1, 2) == -4 and L.lpcnet_batch_analysis_reset(b.p, -1, 1) == -4
    buf = C.create_string_buffer(L.lpcnet_batch_analysis_state_size())
    assert L.lpcnet_batch_get_analysis_state(b.p, 2, buf) == -4 and L.lpcnet_batch_set_analysis_state(b.p, -1, buf) == -4
    assert L.lpcnet_batch_get_analysis_state(b.p, 0, None) == -4
    assert L.lpcnet_batch_analysis_enable(b.p, 0) == -4
    assert L.lpcnet_batch_analyze(b.p, pcm, feat, 36, 1) == 0                   # the batch is still usable
    b.close()
    L.lpcnet_batch_create.restype = C.c_void_p
    nb = L.lpcnet_batch_create(2, 0)                                            # a batch without a model: an error, never a crash
    assert L.lpcnet_batch_analyze(nb, pcm, feat, 36, 1) == -5 and "no model" in api.last_error()
    assert L.lpcnet_batch_analysis_reset(nb, 0, 2) == -5
    L.lpcnet_batch_destroy(C.c_void_p(nb))
