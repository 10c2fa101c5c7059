"""The DRED encoder of an int8 (DOT_PROD) blob on the device (rdovae_enc_i8_kernel<S>) against the reference's generic-C int8 build
(tests/golden/golden_dred_enc_i8_v1.npz, made by tests/tools/make_golden_dred_enc_i8.py from oracle/_ref/liblpcnet_ref_gi.so): the width sets in
every form of the kernel with ragged counts, the state across calls, moving and clearing state, the captured uniform step, and the way into the
int8 decoder.  The per-stream state is float in the int8 build too, so reset, copy_streams and get / set state are the float batch's code on the
int8 batch.  All comparisons on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_enc_model as em  # noqa: E402
import dred_i8_model as di  # noqa: E402
from lpcnet_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

N, MD = em.N_STREAMS, em.N_DFRAMES
SENTINEL = np.float32(-12345.678)
FORMS = (1, 2, 4, 8, 0)          # nine streams: a full workgroup and one stream at 8, two full and one at 4; 0 = the table's form


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_i8_v1.npz"))


@pytest.fixture(scope="module")
def feat(gold):
    f = em.inputs()
    assert np.uint32(zlib.crc32(f.tobytes())) == gold["in_crc"]
    return f


@pytest.fixture(scope="module")
def cases(gold, hip_lib):
    """per width set: the blob and the reference's results, made once and left unchanged"""
    out = {}
    for name in em.SETS:
        blob = di.blob_enc(name)
        assert np.uint32(zlib.crc32(blob)) == gold["blob_crc_" + name]
        out[name] = dict(blob=blob, lat=gold["lat_" + name], init=gold["init_" + name], gru=gold["gru_" + name], mem_crc=gold["mem_crc_" + name],
                         mem_full=gold["mem_full_" + name], gruf=gold["gru_" + name].shape[1])
    return out


@pytest.fixture(scope="module")
def batches(cases):
    """one nine-stream batch per width set, shared by the tests; each resets it first and leaves form 0 and every stream active"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = api.LPCNetBatch(N, cases[name]["blob"])
            made[name].dred_enc_enable(MD)
        made[name].reset()
        return made[name]
    yield get
    for b in made.values():
        b.close()


def fresh(case, n=N, md=MD):
    return np.full((n, md, case["lat"].shape[2]), SENTINEL, np.float32), np.full((n, md, case["init"].shape[2]), SENTINEL, np.float32)


def assert_rows(got, case, count, what="", src=None, first=None):
    """rows below count[s] of (latents, initial states) equal the reference's rows first[s] .. of stream src[s]; the others still hold the sentinel"""
    for g, want in zip(got, (case["lat"], case["init"])):
        for s in range(g.shape[0]):
            k, f, r = int(count[s]), 0 if first is None else int(first[s]), s if src is None else int(src[s])
            assert np.array_equal(bits(g[s, :k]), bits(want[r, f:f + k])), (what, s, np.argwhere(bits(g[s, :k]) != bits(want[r, f:f + k]))[:4].tolist())
            assert (bits(g[s, k:]) == bits(SENTINEL)).all(), (what, s, "rows past the count were written")


def assert_final_states(b, case, what=""):
    """every stream's state read back equals the fixture's: the GRU states, the conv memory by CRC and stream 0's in full"""
    states = [b.get_dred_enc_state(s) for s in range(N)]
    for s, st in enumerate(states):
        assert np.array_equal(bits(st[:case["gruf"]]), bits(case["gru"][s])), (what, s)
    assert em.mem_crc(states, case["gruf"]).tolist() == case["mem_crc"].tolist(), what
    assert np.array_equal(bits(states[0][case["gruf"]:]), bits(case["mem_full"])), what


def chunk(feat, first, count, md=MD, stride=20):
    """the call's feature array: stream s's double frames first[s] .. first[s] + count[s] - 1 at rows 0 .., the rest poisoned"""
    out = np.full((feat.shape[0], 2 * md, stride), np.float32(3e4), np.float32)
    for s in range(feat.shape[0]):
        out[s, :2 * int(count[s]), :20] = feat[s, 2 * int(first[s]):2 * int(first[s] + count[s])]
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(em.SETS))
def test_encode_equals_the_int8_reference_in_every_form(name, form, cases, batches, feat):
    case, s = cases[name], em.SETS[name]
    b = batches(name)
    assert b.dred_enc_flavour() == 1
    assert b.dred_enc_info() == (MD, 40, s["latent_dim"], s["state_dim"], s["taps"], sum(s["widths"]), case["gruf"] + (s["taps"] - 1) * sum(s["widths"]))
    assert b.dred_enc_form(form) == (form if form else 1)          # (widths up to 256 fit every form; nine streams fit the CUs one to a workgroup)
    try:
        got = b.dred_encode(feat, em.COUNT, *fresh(case))
    finally:
        b.dred_enc_form(0)
    assert_rows(got, case, em.COUNT, (name, form))
    assert_final_states(b, case, (name, form))
    assert em.COUNT.min() == 0 and em.COUNT.max() == MD and np.abs(case["lat"]).max() > 1


@pytest.mark.parametrize("name", ["narrow", "tf"])
def test_state_carries_from_call_to_call(name, cases, batches, feat):
    """the 7 double frames as calls of 3 + 1 + 3 equal one call of 7"""
    case = cases[name]
    b = batches(name)
    done = np.zeros(N, np.int32)
    for k in (3, 1, 3):
        cnt = np.clip(em.COUNT - done, 0, k).astype(np.int32)
        got = b.dred_encode(chunk(feat, done, cnt), cnt, *fresh(case))
        assert_rows(got, case, cnt, (name, k), first=done)
        done += cnt
    assert_final_states(b, case, name)


def test_a_long_run_equals_the_int8_reference(cases, gold):
    f = em.long_inputs()
    assert np.uint32(zlib.crc32(f.tobytes())) == gold["long_in_crc"]
    b = api.LPCNetBatch(em.LONG_STREAMS, cases["tf"]["blob"])
    b.dred_enc_enable(em.LONG_DFRAMES)
    assert b.dred_enc_form(8) == 8
    lat, init = b.dred_encode(f, em.LONG_COUNT)
    states = [b.get_dred_enc_state(s) for s in range(em.LONG_STREAMS)]
    b.close()
    s, gruf = em.LONG_FULL_STREAM, cases["tf"]["gruf"]
    assert np.array_equal(bits(lat[s]), bits(gold["long_lat"])) and np.array_equal(bits(init[s]), bits(gold["long_init"]))
    assert em.rows_crc(lat, init, em.LONG_COUNT).tolist() == gold["long_crc"].tolist()
    assert [zlib.crc32(st[:gruf].tobytes()) for st in states] == gold["long_gru_crc"].tolist()
    assert em.mem_crc(states, gruf).tolist() == gold["long_mem_crc"].tolist()


def test_moving_and_clearing_state_on_the_int8_batch(cases, feat):
    case = cases["narrow"]
    sb = api.LPCNetBatch(N, case["blob"], devices=[0, 0])          # shards (0, 5) and (5, 4)
    sb.dred_enc_enable(MD)
    zero = np.zeros(N, np.int32)
    c1 = np.minimum(em.COUNT, 3).astype(np.int32)
    assert_rows(sb.dred_encode(chunk(feat, zero, c1), c1, *fresh(case)), case, c1, "first three")
    # set_state(get_state) is the identity, also where it turns the ring (stream 8: three double frames in, one to go)
    st8 = sb.get_dred_enc_state(8)
    sb.set_dred_enc_state(8, st8)
    assert np.array_equal(bits(sb.get_dred_enc_state(8)), bits(st8))
    # stream 0 -> slot 2 within shard 0, stream 4 -> slot 7 across the shards; then four more double frames on the new slots, one on stream 8
    st0 = sb.get_dred_enc_state(0)
    sb.copy_streams([0, 4], [2, 7])
    assert np.array_equal(bits(sb.get_dred_enc_state(2)), bits(st0)) and np.array_equal(bits(sb.get_dred_enc_state(0)), bits(st0))
    src, first, cnt = np.arange(N), np.zeros(N, np.int32), np.zeros(N, np.int32)
    src[2], src[7] = 0, 4
    first[[2, 7, 8]], cnt[[2, 7, 8]] = 3, (4, 4, 1)
    got = sb.dred_encode(chunk(feat[src], first, cnt), cnt, *fresh(case))
    assert_rows(got, case, cnt, "after the copies", src=src, first=first)
    assert np.array_equal(bits(sb.get_dred_enc_state(2)[:case["gruf"]]), bits(case["gru"][0]))
    assert zlib.crc32(sb.get_dred_enc_state(7)[case["gruf"]:].tobytes()) == case["mem_crc"][4]
    assert np.array_equal(bits(sb.get_dred_enc_state(8)[:case["gruf"]]), bits(case["gru"][8]))
    # reset(first, count) returns those streams to double frame 0 and leaves their neighbours alone
    keep = {s: sb.get_dred_enc_state(s) for s in (1, 3, 6, 8)}
    sb.reset(2, 1)
    sb.reset(7, 1)
    assert not sb.get_dred_enc_state(2).any() and not sb.get_dred_enc_state(7).any()
    assert all(np.array_equal(bits(sb.get_dred_enc_state(s)), bits(v)) for s, v in keep.items())
    cnt[:] = 0
    cnt[[2, 7]] = 3
    got = sb.dred_encode(chunk(feat[src], zero, cnt), cnt, *fresh(case))
    assert_rows(got, case, cnt, "after the reset", src=src)
    sb.close()


def test_the_uniform_step_is_captured_and_replayed(cases, feat):
    """count = NULL, one double frame per call: captured once with torch.cuda.graph, replayed double frame after double frame"""
    import torch
    case = cases["tf"]
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(N, case["blob"])
    b.dred_enc_enable(1)
    d_feat = torch.zeros((N, 2, 20), dtype=torch.float32, device=dev)
    d_lat = torch.zeros((N, 1, 80), dtype=torch.float32, device=dev)
    d_init = torch.zeros((N, 1, 24), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.dred_encode_device(d_feat.data_ptr(), 20, 1, d_lat.data_ptr(), d_init.data_ptr())          # (a first launch outside the capture)
    b.sync()
    b.reset()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=st):
        b.dred_encode_device(d_feat.data_ptr(), 20, 1, d_lat.data_ptr(), d_init.data_ptr(), hip_stream=torch.cuda.current_stream().cuda_stream)
    assert not b.get_dred_enc_state(0).any()              # (the capture ran nothing)
    lat, init = fresh(case)
    for d in range(MD):
        d_feat.copy_(torch.from_numpy(feat[:, 2 * d:2 * d + 2]))
        g.replay()
        torch.cuda.synchronize()
        lat[:, d], init[:, d] = d_lat.cpu().numpy()[:, 0], d_init.cpu().numpy()[:, 0]
    b.close()
    for s in range(N):                                    # (every stream ran all seven; the fixture has a stream's first COUNT[s])
        k = int(em.COUNT[s])
        assert np.array_equal(bits(lat[s, :k]), bits(case["lat"][s, :k])) and np.array_equal(bits(init[s, :k]), bits(case["init"][s, :k])), s


def test_encoder_output_decodes_on_the_int8_decoder(gold, feat):
    """encode_device -> dred_decode_device on one stream of a blob with both int8 halves: the newest double frame's initial state, the latents
    newest first (dred_enc_model.py), against the reference's decode of its own encoder output and the NumPy restatement of the whole way"""
    import torch
    blob = di.blob_enc("tf", with_dec=True)
    assert np.uint32(zlib.crc32(blob)) == gold["blob_crc_rt"]
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(N, blob)
    b.dred_enc_enable(MD)
    b.dred_enable(MD)
    assert b.dred_info()[1:] == b.dred_enc_info()[2:4] and b.dred_flavour() == 1 and b.dred_enc_flavour() == 1
    dcount = np.zeros(N, np.int32)
    dcount[list(em.RT_STREAMS)] = MD
    st = torch.cuda.Stream()
    d_feat = torch.from_numpy(feat).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_lat = torch.zeros((N, MD, 80), dtype=torch.float32, device=dev)
        d_init = torch.zeros((N, MD, 24), dtype=torch.float32, device=dev)
        d_out = torch.zeros((N, 4 * MD, 20), dtype=torch.float32, device=dev)
        b.dred_encode_device(d_feat.data_ptr(), 20, em.COUNT, d_lat.data_ptr(), d_init.data_ptr(), hip_stream=st.cuda_stream)
        d_state = d_init[:, MD - 1].contiguous()
        d_rev = d_lat.flip(1).contiguous()
        b.dred_decode_device(d_state.data_ptr(), d_rev.data_ptr(), dcount, d_out.data_ptr(), hip_stream=st.cuda_stream)
        out = d_out.cpu().numpy()
    b.close()
    assert np.array_equal(bits(out[list(em.RT_STREAMS)]), bits(gold["rt_feat"]))
    s = em.RT_STREAMS[0]
    enc = di.DredEncNumpyI8(blob)
    lat, init = enc.encode(enc.fresh(), feat[s], MD)
    assert np.array_equal(bits(di.DredDecNumpyI8(blob).decode(init[MD - 1], lat[::-1], MD)), bits(out[s]))


def test_the_flavour_follows_the_blob_and_a_mismatch_is_refused(cases):
    b = api.LPCNetBatch(2, cases["narrow"]["blob"])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_enc_flavour()
    b.dred_enc_enable(2)
    assert b.dred_enc_flavour() == 1
    b.close()
    f = api.LPCNetBatch(2, em.set_blob("narrow"))
    f.dred_enc_enable(2)
    assert f.dred_enc_flavour() == 0
    f.close()
    s = em.SETS["narrow"]
    kw = dict(taps=s["taps"], latent_dim=s["latent_dim"], gdense1=s["gdense1"], state_dim=s["state_dim"])
    nb = api.LPCNetBatch(2, em.blob_enc(s["widths"], gru_flavour="int8", **kw))          # int8 arrays beside a float model
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*int8.*float"):
        nb.dred_enc_enable(2)
    nb.close()
