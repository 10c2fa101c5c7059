"""The packet unpacker on the device (decode_kernel, decode_kernel.hip.h) against the reference, field by field: lpcnet_batch_run_decode --
the kernel launched as lpcnet_batch_decode launches it, its feature rows copied back -- equals decode_packet of the reference's generic-C
float build on the bit patterns of all 20 floats of every sub-frame, tolerance 0, over the field census of tests/tools/decode_census.py
(every (main_pitch, modulation) pair, every (vq_mid & 3, sign, interp_id) triple, every c0_id and corr_id, the corners of the VQ indices,
both pitch clamps) and over a real encoder's packets; fixture tests/golden/golden_decode_v1.npz, made by tests/tools/make_golden_decode.py.
Across chunkings (the VQ memory carried in registers or through memory), batch sizes that leave a workgroup half empty, the active prefix,
shards and resets; the seam advances nothing but the VQ memory.  The PCM of the census through lpcnet_batch_decode and lpcnet_decode equals
lpcnet_decode of the reference sample for sample: the frame network at the pitch clamps and at the ends of c0, with inputs the codec produces."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import decode_census as dc  # noqa: E402
import make_golden_decode as mgd  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]      # a NaN no arithmetic of the kernel produces: compared on its bits


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(mgd.PATH))
    g["packets"] = dc.packets()
    assert dc.crc32(g["packets"]) == int(g["packets_crc32"]), "tests/tools/decode_census.py no longer generates the packets of the fixture"
    g["enc_packets"] = np.load(mgd.ENC_PATH)["packets"]
    g["cbs"] = synth.make_codebooks(int(g["codebook_seed"]))
    return g


@pytest.fixture()
def codebooks(gold, hip_lib):
    api.set_codebooks(*gold["cbs"])


def rows(feat, n_packets):
    """run_decode's (n, 4P, 20) as (n, P, 4, 20)"""
    return feat.reshape(feat.shape[0], n_packets, 4, 20)


def check_chains(b, gold, order, got):
    """stream s of the batch decoded chain order[s] of the census from a zero memory: rows and final VQ memory against the fixture"""
    order = list(order)
    assert not dc.differences(rows(got, dc.P), gold["features"][order], gold["packets"][order])
    for s, c in enumerate(order):
        assert np.array_equal(bits(b.get_decoder_vq_mem(s)), bits(gold["vq_mem"][c])), (s, c)


def test_the_census_in_one_call_equals_the_reference_in_every_float(gold, blob_f32, codebooks):
    b = api.LPCNetBatch(dc.CHAINS, blob_f32)
    assert all(not b.get_decoder_vq_mem(s).any() for s in range(dc.CHAINS))
    check_chains(b, gold, range(dc.CHAINS), b.run_decode(gold["packets"]))
    b.close()


def test_chunks_of_1_3_and_64_packets_carry_the_vq_memory_like_one_call(gold, blob_f32, codebooks):
    pk = gold["packets"]
    b = api.LPCNetBatch(dc.CHAINS, blob_f32)
    for step in (1, 3, 64):
        b.reset()
        got = np.concatenate([b.run_decode(np.ascontiguousarray(pk[:, p:p + step])) for p in range(0, dc.P, step)], axis=1)
        assert got.shape == (dc.CHAINS, 4 * dc.P, 20), step
        check_chains(b, gold, range(dc.CHAINS), got)
    b.close()


@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_batch_sizes_with_a_half_empty_workgroup_and_nothing_written_past_the_batch(gold, blob_f32, codebooks, n):
    order = [(3 * s + 5) % dc.CHAINS for s in range(n)]                           # chains in another order, repeated beyond eight streams
    b = api.LPCNetBatch(n, blob_f32)
    out = np.full((n + 1, 4 * dc.P, 20), SENTINEL, np.float32)
    b.run_decode(np.ascontiguousarray(gold["packets"][order]), out=out)
    check_chains(b, gold, order, out[:n])
    assert (bits(out[n]) == bits(SENTINEL)).all()
    b.close()


def test_an_active_prefix_of_5_out_of_9_leaves_the_other_rows_and_memories_alone(gold, blob_f32, codebooks):
    n, act = 9, 5
    order = [(3 * s + 5) % dc.CHAINS for s in range(n)]
    pk = np.ascontiguousarray(gold["packets"][order])
    b = api.LPCNetBatch(n, blob_f32)
    planted = [np.arange(18, dtype=np.float32) * (s + 1) - 7 for s in range(n)]
    for s in range(act, n):
        b.set_decoder_vq_mem(s, planted[s])
    b.active = act
    out = np.full((n, 4 * dc.P, 20), SENTINEL, np.float32)
    b.run_decode(pk, out=out)
    check_chains(b, gold, order[:act], out[:act])
    assert (bits(out[act:]) == bits(SENTINEL)).all()
    for s in range(act, n):
        assert np.array_equal(bits(b.get_decoder_vq_mem(s)), bits(planted[s])), s
    b.active = n
    b.reset()
    check_chains(b, gold, order, b.run_decode(pk))
    b.close()


def test_two_uneven_shards_on_one_device(gold, blob_f32, codebooks):
    n = 5
    order = [(3 * s + 5) % dc.CHAINS for s in range(n)]
    pk = np.ascontiguousarray(gold["packets"][order])
    b = api.LPCNetBatch(n, blob_f32, devices=[0, 0])
    assert [c for _, c, _ in b.shards] == [3, 2]
    out = np.full((n + 1, 4 * dc.P, 20), SENTINEL, np.float32)
    b.run_decode(pk, out=out)
    check_chains(b, gold, order, out[:n])
    assert (bits(out[n]) == bits(SENTINEL)).all()
    b.reset()
    got = np.concatenate([b.run_decode(np.ascontiguousarray(pk[:, :7])), b.run_decode(np.ascontiguousarray(pk[:, 7:]))], axis=1)
    check_chains(b, gold, order, got)
    b.close()


def test_reset_returns_the_vq_memory_to_zero(gold, blob_f32, codebooks):
    pk = gold["packets"]
    b = api.LPCNetBatch(dc.CHAINS, blob_f32)
    b.run_decode(np.ascontiguousarray(pk[:, :20]))
    mem = [b.get_decoder_vq_mem(s) for s in range(dc.CHAINS)]
    assert all(m.any() for m in mem)
    b.reset(1, 2)                                                                 # exactly streams 1 and 2
    for s in range(dc.CHAINS):
        assert np.array_equal(bits(b.get_decoder_vq_mem(s)), bits(np.zeros(18, np.float32) if s in (1, 2) else mem[s])), s
    b.reset()
    assert all(not b.get_decoder_vq_mem(s).any() for s in range(dc.CHAINS))
    check_chains(b, gold, range(dc.CHAINS), b.run_decode(pk))
    b.close()


def test_the_seam_leaves_the_synthesis_state_and_the_kept_frame_products_alone(gold, blob_f32, codebooks):
    n, T = 2, 3
    feats = np.stack([synth.make_features(8100 + s, 2 * T + 1) for s in range(n)])
    pk = np.ascontiguousarray(gold["packets"][:n, :9])
    ns, pre = np.full(n, 80, np.int32), np.zeros(n, np.int32)
    a, ref = api.LPCNetBatch(n, blob_f32), api.LPCNetBatch(n, blob_f32)
    outs = []
    for b in (a, ref):
        b.synthesize(np.ascontiguousarray(feats[:, :T]))
        first = b.synthesize_step(np.ascontiguousarray(feats[:, T]), np.zeros((n, 160), np.int16), ns, pre, np.ones(n, np.int32))      # frame network + 80 samples
        if b is a:
            before = [bytes(b.get_state(s)) for s in range(n)]
            b.run_decode(pk)
            assert all(b.get_decoder_vq_mem(s).any() for s in range(n))
            assert [bytes(b.get_state(s)) for s in range(n)] == before
        rest = b.synthesize_step(np.ascontiguousarray(feats[:, T]), np.zeros((n, 160), np.int16), ns, pre, np.full(n, 2, np.int32))     # the kept products' other 80
        outs.append((first, rest, b.synthesize(np.ascontiguousarray(feats[:, T + 1:]))))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    assert outs[0][1][:, :80].any() and outs[0][2].any()
    assert not any(ref.get_decoder_vq_mem(s).any() for s in range(n))
    a.close(); ref.close()


def test_a_real_encoders_packets_equal_the_reference(gold, blob_f32, codebooks):
    enc = gold["enc_packets"]
    n, P = enc.shape[:2]
    b = api.LPCNetBatch(n, blob_f32)
    got = b.run_decode(enc)
    k = int(gold["enc_stream"])
    assert not dc.differences(rows(got[k:k + 1], P), gold["enc_features"].reshape(1, P, 4, 20), enc[k:k + 1])
    assert [dc.crc32(r) for r in got] == gold["enc_features_crc32"].tolist()
    b.close()


def test_the_batched_decoder_gives_the_references_pcm_for_the_whole_census(gold, blob_f32, codebooks):
    b = api.LPCNetBatch(dc.CHAINS, blob_f32)
    pcm = b.decode(gold["packets"]).reshape(dc.CHAINS, dc.P, 640)
    crc = np.array([[dc.crc32(pcm[s, p]) for p in range(dc.P)] for s in range(dc.CHAINS)], np.uint32)
    bad = np.argwhere(crc != gold["pcm_crc32"])
    assert not bad.size, (len(bad), "first (chain, packet):", bad[0].tolist(), dc.describe(gold["packets"][tuple(bad[0])]))
    k, full = int(gold["pcm_chain"]), gold["pcm"]
    assert np.array_equal(pcm[k].reshape(-1)[:full.size], full)
    check = [b.get_decoder_vq_mem(s) for s in range(dc.CHAINS)]
    assert np.array_equal(bits(np.stack(check)), bits(gold["vq_mem"]))
    b.close()


def test_the_single_stream_decoder_gives_the_references_pcm(gold, blob_f32, codebooks):
    P = 16
    k, full = int(gold["pcm_chain"]), gold["pcm"]
    assert full.size >= P * 640
    dec = api.LPCNetDecState(blob_f32)
    pcm = np.concatenate([dec.decode(p) for p in gold["packets"][k, :P]])
    assert np.array_equal(pcm, full[:P * 640])
    assert [dc.crc32(pcm[p * 640:(p + 1) * 640]) for p in range(P)] == gold["pcm_crc32"][k, :P].tolist()


def test_argument_errors_leave_the_batch_usable(gold, blob_f32, codebooks, hip_lib):
    L = hip_lib
    n = 2
    pk = np.ascontiguousarray(gold["packets"][:n, :2])
    feat = np.zeros(n * 8 * 20, np.float32)
    b = api.LPCNetBatch(n, blob_f32)
    assert L.lpcnet_batch_run_decode(b.p, pk.reshape(-1), feat, 0) == -4 and "bad arguments" in api.last_error()
    assert L.lpcnet_batch_run_decode(b.p, pk.reshape(-1), feat, -3) == -4
    f = L.lpcnet_batch_run_decode
    saved, f.argtypes = f.argtypes, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    try:
        assert f(b.p, None, feat.ctypes.data, 2) == -4 and "bad arguments" in api.last_error()
        assert f(b.p, pk.ctypes.data, None, 2) == -4
    finally:
        f.argtypes = saved
    assert not any(b.get_decoder_vq_mem(s).any() for s in range(n))               # a refused call has advanced nothing
    got = b.run_decode(pk)                                                        # the batch is still usable
    assert not dc.differences(rows(got, 2), gold["features"][:n, :2], pk)
    b.close()
    nb = L.lpcnet_batch_create(n, 0)                                              # a batch without a model: an error, never a crash
    assert L.lpcnet_batch_run_decode(nb, pk.reshape(-1), feat, 2) == -5 and "no model" in api.last_error()
    L.lpcnet_batch_destroy(C.c_void_p(nb))


def test_without_codebooks_the_seam_and_the_host_unpacker_return_the_model_error(blob_f32):
    """a fresh process, so that no codebooks are installed and no default file is found"""
    code = (
        "import os, sys, tempfile\n"
        "os.chdir(tempfile.mkdtemp())\n"
        "import numpy as np\n"
        "from lpcnet_amd import api, synth\n"
        "L = api.load_library()\n"
        "pk = np.zeros(16, np.uint8); feat = np.zeros(2 * 4 * 36, np.float32); mem = np.zeros(18, np.float32)\n"
        "rh = L.lpcnet_hip_packet_features(pk[:8], mem, feat); mh = api.last_error()\n"
        "b = api.LPCNetBatch(2, synth.blob_bytes(synth.make_model()))\n"
        "rs = L.lpcnet_batch_run_decode(b.p, pk, feat, 1); ms = api.last_error()\n"
        "print('RESULT', rh, rs, int('codebooks' in mh), int('codebooks' in ms))\n"
        "b.close()\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("LPCNET_HIP_CODEBOOKS", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    assert [int(x) for x in line[0].split()[1:]] == [-5, -5, 1, 1]
