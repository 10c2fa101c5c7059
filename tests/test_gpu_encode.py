"""The encoder on the device (lpcnet_batch_encode*, lpcnet_batch_compute_features*): lpcnet_encode / lpcnet_compute_features per stream
and packet, byte for byte / tolerance 0 on the bit patterns of all 36 floats -- against the reference's generic-C float build (fixture
tests/golden/golden_encode_v1.npz, made by tests/tools/make_golden_encode.py; live against oracle/_ref where it exists), across
chunkings, snapshot / rollback, interleavings of the three entry points on one state, resets, shards, batch sizes, the device-pointer
path into the decoder, a captured graph, and the argument checks."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import make_golden_encode as mge  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gold():
    g = np.load(mge.PATH)
    P = g["packets"].shape[1]
    pcm = np.stack([synth.make_pcm(int(s), 4 * P) for s in g["seeds"]])
    assert [zlib.crc32(p.tobytes()) for p in pcm] == g["pcm_crc32"].tolist()
    return dict(P=P, pcm=pcm, packets=g["packets"], feats=g["features"], cbs=synth.make_codebooks(int(g["codebook_seed"])))


@pytest.fixture()
def codebooks(gold, hip_lib):
    api.set_codebooks(*gold["cbs"])


@pytest.fixture(scope="module")
def ref_lib(gold):
    if not os.path.exists(REF_LIB):
        pytest.skip("compiled reference absent (make -C oracle ref)")
    return mge.load_ref(REF_LIB, gold["cbs"])


def test_the_fixture_is_not_degenerate(gold):
    cov = mge.coverage(gold["packets"])
    assert mge.is_rich(cov), cov
    assert gold["P"] >= 60


def test_packets_equal_the_fixture_in_one_call(gold, blob_f32, codebooks):
    b = api.LPCNetBatch(gold["pcm"].shape[0], blob_f32)
    out = b.encode(gold["pcm"])
    bad = out != gold["packets"]
    f_got, f_want = mge.packet_fields(out), mge.packet_fields(gold["packets"])
    assert not bad.any(), (int(bad.any(axis=2).sum()), {k: int((f_got[k] != f_want[k]).sum()) for k in f_got})
    b.close()


def test_compute_features_equals_the_fixture_in_all_36_floats(gold, blob_f32, hip_lib):
    b = api.LPCNetBatch(gold["pcm"].shape[0], blob_f32)
    out = b.compute_features(gold["pcm"])
    bad = bits(out) != bits(gold["feats"])
    assert not bad.any(), (int(bad.sum()), bad.sum(axis=(0, 1)).tolist())
    b.close()


def test_live_reference_on_fresh_seeds(gold, blob_f32, codebooks, ref_lib):
    P, seeds = 30, list(range(9300, 9308))
    pcm = np.stack([synth.make_pcm(s, 4 * P) for s in seeds])
    want_p, want_f = [], []
    for p in pcm:
        e = mge.RefEncoder(ref_lib); want_p.append(e.encode(p)); e.close()
        e = mge.RefEncoder(ref_lib); want_f.append(e.compute_features(p)); e.close()
    b = api.LPCNetBatch(len(seeds), blob_f32)
    assert np.array_equal(b.encode(pcm), np.stack(want_p))
    b.analysis_reset()
    assert same(b.compute_features(pcm), np.stack(want_f))
    b.close()


def test_chunked_calls_and_rollback_equal_one_call(gold, blob_f32, codebooks):
    P = 30
    pcm = gold["pcm"][:, :640 * P]
    n = pcm.shape[0]
    b = api.LPCNetBatch(n, blob_f32)
    for step in (1, 3, 10):
        b.analysis_reset()
        out = np.concatenate([b.encode(pcm[:, p * 640:min(P, p + step) * 640]) for p in range(0, P, step)], axis=1)
        assert np.array_equal(out, gold["packets"][:, :P]), step
        b.analysis_reset()
        out = np.concatenate([b.compute_features(pcm[:, p * 640:min(P, p + step) * 640]) for p in range(0, P, step)], axis=1)
        assert same(out, gold["feats"][:, :4 * P]), step
    # snapshot (analysis state + vq_mem) after 12 packets, run on, roll back, replay
    b.analysis_reset()
    b.encode(pcm[:, :640 * 12])
    snap = [(b.get_analysis_state(s), b.get_encoder_vq_mem(s)) for s in range(n)]
    assert all(np.any(m != 0) for _, m in snap)
    first = b.encode(pcm[:, 640 * 12:])
    for s in range(n):
        b.set_analysis_state(s, snap[s][0]); b.set_encoder_vq_mem(s, snap[s][1])
    assert np.array_equal(b.encode(pcm[:, 640 * 12:]), first) and np.array_equal(first, gold["packets"][:, 12:P])
    b.close()


def test_the_three_entry_points_interleave_on_one_state_like_the_reference(gold, blob_f32, codebooks, ref_lib):
    """encode / compute_features in any order, analyze followed by either, and encode - analyze - encode: each call's output equals the
    reference's driven the same way on one LPCNetEncState; analyze's own output is compared only while no four-frame call has come
    before it (afterwards the reference returns a stale slot, include/lpcnet_batch.h)."""
    pcm = gold["pcm"][:3]
    n = pcm.shape[0]
    plan = [("analyze", 3), ("encode", 2), ("compute_features", 1), ("encode", 3), ("analyze", 5), ("encode", 2), ("compute_features", 2),
            ("analyze", 1), ("compute_features", 1), ("encode", 4)]
    b = api.LPCNetBatch(n, blob_f32)
    refs = [mge.RefEncoder(ref_lib) for _ in range(n)]
    pos, four_frame_seen = 0, False
    for what, count in plan:
        ns = count * (160 if what == "analyze" else 640)
        seg = pcm[:, pos:pos + ns]
        pos += ns
        got = getattr(b, what)(seg)
        want = np.stack([getattr(refs[s], what)(seg[s]) for s in range(n)])
        if what == "encode":
            assert np.array_equal(got, want), (what, pos)
        elif what == "compute_features" or not four_frame_seen:
            assert same(got, want), (what, pos)
        four_frame_seen |= what != "analyze"
    for r in refs:
        r.close()
    b.close()


def test_analysis_reset_clears_vq_mem_and_reset_does_not(gold, blob_f32, codebooks):
    pcm = gold["pcm"][:, :640 * 5]
    n = pcm.shape[0]
    b = api.LPCNetBatch(n, blob_f32)
    assert all(not b.get_encoder_vq_mem(s).any() for s in range(n))             # zero on allocation
    first = b.encode(pcm)
    mem = [b.get_encoder_vq_mem(s) for s in range(n)]
    an = [b.get_analysis_state(s) for s in range(n)]
    assert all(m.any() for m in mem)
    b.reset()
    assert all(np.array_equal(b.get_encoder_vq_mem(s), mem[s]) for s in range(n)) and [b.get_analysis_state(s) for s in range(n)] == an
    b.analysis_reset(1, 2)                                                      # exactly streams 1 and 2 restart
    assert [not b.get_encoder_vq_mem(s).any() for s in range(n)] == [s in (1, 2) for s in range(n)]
    second = b.encode(pcm)
    assert np.array_equal(second[1:3], first[1:3]) and not np.array_equal(second[0], first[0]) and not np.array_equal(second[3:], first[3:])
    b.close()


def test_2048_streams_at_once_and_a_sharded_batch(gold, blob_f32, codebooks):
    n, P, small = 2048, 2, 64
    pcm = np.stack([synth.make_pcm(30000 + s, 4 * P) for s in range(n)])
    big = api.LPCNetBatch(n, blob_f32)
    out = big.encode(pcm)
    big.analysis_reset()
    feats = big.compute_features(pcm)
    big.close()
    b = api.LPCNetBatch(small, blob_f32)
    for k in range(0, n, small):
        b.analysis_reset()
        assert np.array_equal(b.encode(pcm[k:k + small]), out[k:k + small]), k
    b.analysis_reset()
    assert same(b.compute_features(pcm[:small]), feats[:small])
    b.close()
    one = api.LPCNetBatch(1, blob_f32)                                            # per-stream results
    for s in (0, 777, 2047):
        one.analysis_reset()
        assert np.array_equal(one.encode(pcm[s:s + 1]), out[s:s + 1]), s
    one.close()
    sh = api.LPCNetBatch(301, blob_f32, devices=[0, 0])                           # two uneven shards on one device
    assert len(sh.shards) == 2
    got = np.concatenate([sh.encode(pcm[:301, :640]), sh.encode(pcm[:301, 640:])], axis=1)
    assert np.array_equal(got, out[:301])
    sh.analysis_reset()
    assert same(sh.compute_features(pcm[:301]), feats[:301])
    sh.close()


def test_encode_feeds_decode_on_the_device(gold, blob_f32, codebooks):
    """encode_device -> decode_device on one HIP stream, the packets never leaving the device, equals decode of the fixture's packets"""
    import torch
    n, P = gold["pcm"].shape[0], 3
    dev = torch.device("cuda:0")
    ref = api.LPCNetBatch(n, blob_f32)
    want = ref.decode(np.ascontiguousarray(gold["packets"][:, :P]))
    ref.close()
    b = api.LPCNetBatch(n, blob_f32)
    d_in = torch.from_numpy(np.ascontiguousarray(gold["pcm"][:, :640 * P])).to(dev)
    d_pk = torch.zeros((n, P, 8), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((n, P * 640), dtype=torch.int16, device=dev)
    d_feat = torch.zeros((n, 4 * P, 40), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        b.encode_device(d_in.data_ptr(), d_pk.data_ptr(), P, s.cuda_stream)
        b.decode_device(d_pk.data_ptr(), d_out.data_ptr(), P, s.cuda_stream)
    b.sync()
    assert np.array_equal(d_pk.cpu().numpy(), gold["packets"][:, :P])
    assert np.array_equal(d_out.cpu().numpy(), want)
    b.analysis_reset()
    with torch.cuda.stream(s):                                    # compute_features_device with a caller's stride
        b.compute_features_device(d_in.data_ptr(), d_feat.data_ptr(), 40, P, s.cuda_stream)
    b.sync()
    f = d_feat.cpu().numpy()
    assert same(f[:, :, :36], gold["feats"][:, :4 * P]) and not f[:, :, 36:].any()
    b.close()


def test_a_linear_capture_of_encode_and_decode_replays_bit_exactly(gold, blob_f32, codebooks):
    """one 40-ms step -- encode 640 samples, decode the packet -- captured as ONE linear chain on one stream and replayed.  Before
    encoder_enable the captured call returns the argument error and the capture stays usable."""
    import torch
    n, P = gold["pcm"].shape[0], 4
    dev = torch.device("cuda:0")
    pcm = gold["pcm"]
    ref = api.LPCNetBatch(n, blob_f32)
    want = ref.decode(np.ascontiguousarray(gold["packets"][:, :P]))
    ref.close()
    b = api.LPCNetBatch(n, blob_f32)
    d_in = torch.zeros((n, 640), dtype=torch.int16, device=dev)
    d_pk = torch.zeros((n, 1, 8), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((n, 640), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    got_pk, got_pcm = [], []
    with torch.cuda.stream(s):                                    # packet 0: decode eagerly (first launch); the encoder state does not exist yet
        d_pk.copy_(torch.from_numpy(np.ascontiguousarray(gold["packets"][:, :1])))
        b.decode_device(d_pk.data_ptr(), d_out.data_ptr(), 1, s.cuda_stream)
        s.synchronize()
    got_pk.append(gold["packets"][:, :1]); got_pcm.append(d_out.cpu().numpy().copy())
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        rc = b.L.lpcnet_batch_encode_device(b.p, d_in.data_ptr(), d_pk.data_ptr(), 1, cs)
        msg = api.last_error()
        b.decode_device(d_pk.data_ptr(), d_out.data_ptr(), 1, cs)                # the capture goes on
    assert rc == -4 and "lpcnet_batch_encoder_enable" in msg
    del g0
    b.encoder_enable(1)
    with torch.cuda.stream(s):                                    # bring the encoder state to packet 1 eagerly (also the kernels' first launch)
        d_in.copy_(torch.from_numpy(np.ascontiguousarray(pcm[:, :640])))
        b.encode_device(d_in.data_ptr(), d_pk.data_ptr(), 1, s.cuda_stream)
        s.synchronize()
    assert np.array_equal(d_pk.cpu().numpy(), gold["packets"][:, :1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        b.encode_device(d_in.data_ptr(), d_pk.data_ptr(), 1, cs)
        b.decode_device(d_pk.data_ptr(), d_out.data_ptr(), 1, cs)
    for p in range(1, P):
        d_in.copy_(torch.from_numpy(np.ascontiguousarray(pcm[:, p * 640:(p + 1) * 640])))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got_pk.append(d_pk.cpu().numpy().copy()); got_pcm.append(d_out.cpu().numpy().copy())
    assert np.array_equal(np.concatenate(got_pk, axis=1), gold["packets"][:, :P])
    assert np.array_equal(np.concatenate(got_pcm, axis=1), want)
    del g
    b.close()


def test_argument_errors(gold, blob_f32, codebooks, hip_lib):
    L = hip_lib
    b = api.LPCNetBatch(2, blob_f32)
    pcm = np.zeros(2 * 640, np.int16); pk = np.zeros(2 * 8, np.uint8); feat = np.zeros(2 * 4 * 36, np.float32)
    assert L.lpcnet_batch_encode(b.p, pcm, pk, 0) == -4 and "bad arguments" in api.last_error()
    assert L.lpcnet_batch_compute_features(b.p, pcm, feat, 35, 1) == -4 and "bad arguments" in api.last_error()
    assert L.lpcnet_batch_compute_features(b.p, pcm, feat, 36, 0) == -4
    assert L.lpcnet_batch_encode_device(b.p, None, None, 1, None) == -4
    assert L.lpcnet_batch_compute_features_device(b.p, None, None, 36, 1, None) == -4
    assert L.lpcnet_batch_encode_device_shard(b.p, 1, None, None, 1, None) == -4 and "shard" in api.last_error()
    assert L.lpcnet_batch_encoder_enable(b.p, 0) == -4
    mem = np.zeros(18, np.float32)
    assert L.lpcnet_batch_get_encoder_vq_mem(b.p, 2, mem) == -4 and L.lpcnet_batch_set_encoder_vq_mem(b.p, -1, mem) == -4
    assert L.lpcnet_batch_encode(b.p, pcm, pk, 1) == 0                          # the batch is still usable
    assert L.lpcnet_batch_compute_features(b.p, pcm, feat, 36, 1) == 0
    b.close()
    L.lpcnet_batch_create.restype = C.c_void_p
    nb = L.lpcnet_batch_create(2, 0)                                            # a batch without a model: an error, never a crash
    assert L.lpcnet_batch_encode(nb, pcm, pk, 1) == -5 and "no model" in api.last_error()
    assert L.lpcnet_batch_compute_features(nb, pcm, feat, 36, 1) == -5
    assert L.lpcnet_batch_encoder_enable(nb, 1) == -5
    L.lpcnet_batch_destroy(C.c_void_p(nb))


def test_encode_without_codebooks_returns_what_decode_returns(blob_f32):
    """a fresh process, so that no codebooks are installed and no default file is found"""
    import subprocess
    code = (
        "import os, sys, tempfile\n"
        "os.chdir(tempfile.mkdtemp())\n"
        "import numpy as np\n"
        "from lpcnet_amd import api, synth\n"
        "b = api.LPCNetBatch(2, synth.blob_bytes(synth.make_model()))\n"
        "pcm = np.zeros(2 * 640, np.int16); pk = np.zeros(16, np.uint8); out = np.zeros(2 * 640, np.int16)\n"
        "rd = b.L.lpcnet_batch_decode(b.p, pk, out, 1); md = api.last_error()\n"
        "re = b.L.lpcnet_batch_encode(b.p, pcm, pk, 1); me = api.last_error()\n"
        "feat = np.zeros(2 * 4 * 36, np.float32)\n"
        "rf = b.L.lpcnet_batch_compute_features(b.p, pcm, feat, 36, 1)\n"
        "print('RESULT', rd, re, rf, int('codebooks' in md), int('codebooks' in me))\n"
        "b.close()\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("LPCNET_HIP_CODEBOOKS", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    rd, re_, rf, cd, ce = (int(x) for x in line[0].split()[1:])
    assert rd != 0 and re_ == rd and cd == 1 and ce == 1 and rf == 0
