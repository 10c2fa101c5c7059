"""The DRED decoder on the device (lpcnet_batch_dred_*: DRED_rdovae_decode_all for every stream in one launch per shard) against the reference
(tests/golden/golden_dred_v1.npz, made by tests/tools/make_golden_dred.py from the reference's generic-C float build): three width sets in every
form of the kernel, a long chain, the device and packed forms, the way into the PLC's FEC rings, and the refusals.  All comparisons on bit
patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_model as dm  # noqa: E402
import plc_model as pm  # noqa: E402
from lpcnet_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

N, ML = dm.N_STREAMS, dm.N_LATENTS
SENTINEL = np.float32(-12345.678)
FORMS = (1, 2, 4, 8, 0)          # nine streams: a full workgroup and one stream at 8, two full and one at 4; 0 = the table's form


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_v1.npz"))


@pytest.fixture(scope="module")
def cases(gold, hip_lib):
    """per width set: the blob, the inputs and the reference's features, made once and left unchanged"""
    out = {}
    for name in dm.SETS:
        blob = dm.set_blob(name)
        state, latents = dm.set_inputs(name)
        assert np.uint32(zlib.crc32(blob)) == gold["blob_crc_" + name] and np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold["in_crc_" + name]
        out[name] = (blob, state, latents, gold["feat_" + name])
    return out


@pytest.fixture(scope="module")
def batches(cases):
    """one nine-stream batch per width set, shared by the tests that leave it as they found it (form 0, every stream active)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = api.LPCNetBatch(N, cases[name][0])
            made[name].dred_enable(ML)
        return made[name]
    yield get
    for b in made.values():
        b.close()


def assert_decoded(got, want, count, what=""):
    """rows below 4 count[s] equal the reference's, the others still hold the sentinel"""
    for s in range(got.shape[0]):
        k = 4 * int(count[s])
        assert np.array_equal(bits(got[s, :k]), bits(want[s, :k])), (what, s, np.argwhere(bits(got[s, :k]) != bits(want[s, :k]))[:4].tolist())
        assert (bits(got[s, k:]) == bits(SENTINEL)).all(), (what, s, "rows past the count were written")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(dm.SETS))
def test_decode_equals_the_reference_in_every_form(name, form, cases, batches):
    _, state, latents, want = cases[name]
    b = batches(name)
    assert b.dred_form(form) == (form if form else 1)          # (nine streams fit the CUs one to a workgroup)
    try:
        got = b.dred_decode(state, latents, dm.COUNT, np.full((N, 4 * ML, 20), SENTINEL, np.float32))
    finally:
        b.dred_form(0)
    assert_decoded(got, want, dm.COUNT, (name, form))
    assert dm.COUNT.min() == 0 and dm.COUNT.max() == ML and np.abs(want).max() > 1


@pytest.mark.parametrize("form", [8, 1])
def test_a_long_chain_equals_the_reference(form, cases, gold):
    state, latents = dm.long_inputs()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold["long_in_crc"]
    b = api.LPCNetBatch(dm.LONG_STREAMS, cases["w256"][0])
    b.dred_enable(dm.LONG_LATENTS)
    assert b.dred_form(form) == form
    got = b.dred_decode(state, latents, dm.LONG_COUNT)
    b.close()
    s = dm.LONG_FULL_STREAM
    assert np.array_equal(bits(got[s]), bits(gold["long_full"]))
    assert dm.stream_crc(got, dm.LONG_COUNT).tolist() == gold["long_crc"].tolist()


def test_device_forms_and_two_shards_equal_the_host_form(cases, batches):
    import torch
    _, state, latents, want = cases["mixed"]
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state).to(dev), torch.from_numpy(latents).to(dev)
    b = batches("mixed")
    # on the batch's own stream, then on a caller's
    d_out = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out.data_ptr())
    b.sync()
    assert_decoded(d_out.cpu().numpy(), want, dm.COUNT, "own stream")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_out2 = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
        b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out2.data_ptr(), hip_stream=st.cuda_stream)
        got = d_out2.cpu().numpy()
    assert_decoded(got, want, dm.COUNT, "caller's stream")
    # a capture takes nothing: the launch depends on the host's counts
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out2.data_ptr(), hip_stream=cs)
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, [0] * N, 4 * dm.COUNT, hip_stream=cs)
        d_out2.add_(0)                                    # (the capture stays usable and is not empty)
    b.sync()
    # two unequal shards on one device: the host form, then every shard's device form
    sb = api.LPCNetBatch(N, cases["mixed"][0], devices=[0, 0])
    assert [x[:2] for x in sb.shards] == [(0, 5), (5, 4)]
    sb.dred_enable(ML)
    got = sb.dred_decode(state, latents, dm.COUNT, np.full((N, 4 * ML, 20), SENTINEL, np.float32))
    assert_decoded(got, want, dm.COUNT, "sharded host form")
    d_out3 = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for k, (first, cnt, _) in enumerate(sb.shards):
        sl = slice(first, first + cnt)
        sb.dred_decode_device(d_state[sl].data_ptr(), d_lat[sl].data_ptr(), dm.COUNT[sl], d_out3[sl].data_ptr(), shard=k)
    sb.sync()
    assert_decoded(d_out3.cpu().numpy(), want, dm.COUNT, "device shards")
    with pytest.raises(api.LPCNetError, match=r"\(-4\).*shard"):
        sb.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out3.data_ptr())
    sb.close()


def packed_selection(count):
    """first / take per stream: the whole range (streams 0 and 5), nothing of a stream that decodes (4) and of one that does not (2), the last row
    alone (6), ranges inside (1, 3, 7, 8)"""
    first = np.array([0, 1, 0, 2, 0, 0, 27, 3, 5], np.int32)
    take = np.array([28, 3, 0, 5, 0, 12, 1, 9, 11], np.int32)
    assert (first + take <= 4 * count).all() and take[0] == 4 * count[0] and take[5] == 4 * count[5] and first[6] + 1 == 4 * count[6]
    return first, take


@pytest.mark.parametrize("form", [0, 8])
def test_packed_form_is_the_permutation_of_the_plain_one(form, cases, batches):
    import torch
    _, state, latents, want = cases["small"]
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state).to(dev), torch.from_numpy(latents).to(dev)
    first, take = packed_selection(dm.COUNT)
    b = batches("small")
    b.dred_form(form)
    try:
        torch.cuda.synchronize()
        out = b.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, first, take)
        b.sync()
    finally:
        b.dred_form(0)
    assert out.shape == (int(take.sum()), 20)
    assert np.array_equal(bits(out.cpu().numpy()), bits(dm.packed(want, first, take)))
    # rows outside a stream's decoded ones: refused, nothing enqueued
    for f, t in ((first, take + (np.arange(N) == 3) * 40), (first - 2 * (np.arange(N) == 1), take), (first, take - (np.arange(N) == 2))):
        with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
            b.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, f, t)


def test_decoded_redundancy_goes_into_the_plc_without_a_host_hop(cases, gold):
    """two batches of eight streams on a blob with the PLC network and the decoder: one fed by dred_decode_packed -> plc_fec_feed_device on one
    stream, the other by the host feed with the reference's vectors; then twelve steps with a five-frame loss"""
    import torch
    n = 8
    blob = dm.set_blob("mixed", with_plc=True)
    _, state, latents, want = cases["mixed"]
    count = dm.COUNT[:n]
    first = np.zeros(n, np.int32)
    take = (4 * count).astype(np.int32)
    take[4], first[6], take[6] = 6, 3, 9
    vectors = dm.packed(want[:n], first, take)
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state[:n]).to(dev), torch.from_numpy(latents[:n]).to(dev)
    pcm = np.stack([pm.stream_pcm(s, 12) for s in range(n)])
    lost = np.zeros(12, np.uint8)
    lost[4:9] = 1

    def steps(b):
        out = np.zeros((n, 12, 160), np.int16)
        for t in range(12):
            frame = np.ascontiguousarray(pcm[:, t])
            if lost[t]:
                frame[:] = 0
            out[:, t] = b.plc_step(frame, np.full(n, lost[t], np.uint8))
        return out, [b.get_plc_state(s) for s in range(n)]

    a = api.LPCNetBatch(n, blob)
    a.plc_enable(api.PLC_CAUSAL)
    a.dred_enable(ML)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        buf = a.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), count, first, take, hip_stream=st.cuda_stream)
        dropped = a.plc_fec_feed_device(buf.data_ptr(), take, hip_stream=st.cuda_stream)          # (nothing waits between the decoder and the feed)
    a.sync()
    assert not dropped.any()
    got, got_state = steps(a)
    a.close()
    h = api.LPCNetBatch(n, blob)
    h.plc_enable(api.PLC_CAUSAL)
    assert not h.plc_fec_feed(vectors, take).any()
    ref, ref_state = steps(h)
    # (the vectors matter: without them the concealment differs)
    h.plc_reset()
    bare, _ = steps(h)
    h.close()
    assert np.array_equal(got, ref) and got_state == ref_state
    assert not np.array_equal(bare[:, 4:9], ref[:, 4:9])
    fec_read = [int(np.frombuffer(s[:36], np.int32)[6]) for s in got_state]
    assert fec_read[0] > 0 and fec_read[2] == 0, fec_read           # the lost frames read vectors where the ring had them


def test_refusals_and_the_active_prefix(cases, batches, blob_f32):
    _, state, latents, want = cases["small"]
    fresh = lambda: np.full((N, 4 * ML, 20), SENTINEL, np.float32)
    # before dred_enable; a blob without the decoder's arrays
    b = api.LPCNetBatch(N, cases["small"][0])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_decode(state, latents, dm.COUNT)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_decode_device(0, 0, dm.COUNT, 0)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_form(8)
    b.close()
    nb = api.LPCNetBatch(2, blob_f32)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*no DRED decoder"):
        nb.dred_enable(4)
    nb.close()
    b = batches("small")
    # counts outside 0 .. max_latents: nothing written
    for bad in (-1, ML + 1):
        count = dm.COUNT.copy()
        count[5] = bad
        out = fresh()
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*count"):
            b.dred_decode(state, latents, count, out)
        assert (bits(out) == bits(SENTINEL)).all()
    # the active prefix: a count on an inactive stream is refused; with zero there, the inactive rows stay and the active ones decode
    b.active = 6
    try:
        out = fresh()
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*not active"):
            b.dred_decode(state, latents, dm.COUNT, out)
        assert (bits(out) == bits(SENTINEL)).all()
        count = dm.COUNT.copy()
        count[6:] = 0
        got = b.dred_decode(state, latents, count, out)
        assert_decoded(got, want, count, "prefix of six")
        assert count[:6].sum() > 0 and (bits(got[6:]) == bits(SENTINEL)).all()
    finally:
        b.active = N
    assert_decoded(b.dred_decode(state, latents, dm.COUNT, fresh()), want, dm.COUNT, "whole batch again")
