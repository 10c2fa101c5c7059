"""The DRED decoder of an int8 (DOT_PROD) blob on the device (dred_decode_i8_kernel<S>) against the reference's generic-C int8 build
(tests/golden/golden_dred_i8_v1.npz, made by tests/tools/make_golden_dred_i8.py from oracle/_ref/liblpcnet_ref_gi.so): the width sets in every form
of the kernel, a long chain, the device and packed forms, the way into the int8 PLC's FEC rings, and the flavour the batch reports.  All
comparisons on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_i8_model as di  # noqa: E402
import dred_model as dm  # noqa: E402
import plc_model as pm  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

N, ML = dm.N_STREAMS, dm.N_LATENTS
SENTINEL = np.float32(-12345.678)
# nine streams, ragged, one count 0: at 8 a full workgroup and a last one with a single stream, at 4 two full and one; 0 = the table's form.
# w256 runs at the table's form alone (its other forms walk the same code as `mixed`'s)
CASES = [(name, form) for name in ("small", "mixed") for form in (1, 2, 4, 8)] + [("w256", 0)]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_i8_v1.npz"))


@pytest.fixture(scope="module")
def cases(gold, hip_lib):
    """per width set: the blob, the inputs and the reference's features, made once and left unchanged"""
    out = {}
    for name in dm.SETS:
        blob = di.blob_dec(name)
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


@pytest.mark.parametrize("name,form", CASES)
def test_decode_equals_the_int8_reference_in_every_form(name, form, cases, batches):
    _, state, latents, want = cases[name]
    b = batches(name)
    assert b.dred_flavour() == 1
    assert b.dred_info() == (ML, dm.SETS[name]["latent_dim"], dm.STATE_DIM)
    assert b.dred_form(form) == (form if form else 1)          # (nine streams fit the CUs one to a workgroup)
    try:
        got = b.dred_decode(state, latents, dm.COUNT, np.full((N, 4 * ML, 20), SENTINEL, np.float32))
    finally:
        b.dred_form(0)
    assert_decoded(got, want, dm.COUNT, (name, form))
    assert dm.COUNT.min() == 0 and dm.COUNT.max() == ML and np.abs(want).max() > 1


def test_a_long_chain_equals_the_int8_reference(cases, gold):
    state, latents = dm.long_inputs()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold["long_in_crc"]
    b = api.LPCNetBatch(dm.LONG_STREAMS, cases["w256"][0])
    b.dred_enable(dm.LONG_LATENTS)
    assert b.dred_form(8) == 8
    got = b.dred_decode(state, latents, dm.LONG_COUNT)
    b.close()
    s = dm.LONG_FULL_STREAM
    assert np.array_equal(bits(got[s]), bits(gold["long_full"]))
    assert dm.stream_crc(got, dm.LONG_COUNT).tolist() == gold["long_crc"].tolist()


def test_device_and_packed_forms_equal_the_reference(cases, batches):
    import torch
    _, state, latents, want = cases["small"]
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state).to(dev), torch.from_numpy(latents).to(dev)
    b = batches("small")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_out = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
        b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out.data_ptr(), hip_stream=st.cuda_stream)
        got = d_out.cpu().numpy()
    assert_decoded(got, want, dm.COUNT, "caller's stream")
    # the packed form: the whole range (streams 0 and 5), nothing of a stream that decodes (4) and of one that does not (2), the last row alone (6)
    first = np.array([0, 1, 0, 2, 0, 0, 27, 3, 5], np.int32)
    take = np.array([28, 3, 0, 5, 0, 12, 1, 9, 11], np.int32)
    assert (first + take <= 4 * dm.COUNT).all()
    for form in (0, 8):
        b.dred_form(form)
        try:
            torch.cuda.synchronize()
            out = b.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, first, take)
            b.sync()
        finally:
            b.dred_form(0)
        assert out.shape == (int(take.sum()), 20)
        assert np.array_equal(bits(out.cpu().numpy()), bits(dm.packed(want, first, take))), form


def test_decoded_redundancy_goes_into_the_int8_plc_without_a_host_hop(cases):
    """two batches of eight streams on an int8 blob with the int8 PLC network and the int8 decoder: one fed by dred_decode_packed ->
    plc_fec_feed_device on one stream, the other by the host feed with the reference's vectors; then eight steps with a three-frame loss"""
    import torch
    n, T = 8, 8
    blob = di.blob_dec("mixed", with_plc=True)
    _, state, latents, want = cases["mixed"]
    count = dm.COUNT[:n]
    first = np.zeros(n, np.int32)
    take = (4 * count).astype(np.int32)
    take[4], first[6], take[6] = 6, 3, 9
    vectors = dm.packed(want[:n], first, take)
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state[:n]).to(dev), torch.from_numpy(latents[:n]).to(dev)
    pcm = np.stack([pm.stream_pcm(s, T) for s in range(n)])
    lost = np.zeros(T, np.uint8)
    lost[3:6] = 1

    def steps(b):
        out = np.zeros((n, T, 160), np.int16)
        for t in range(T):
            frame = np.ascontiguousarray(pcm[:, t])
            if lost[t]:
                frame[:] = 0
            out[:, t] = b.plc_step(frame, np.full(n, lost[t], np.uint8))
        return out, [b.get_plc_state(s) for s in range(n)]

    a = api.LPCNetBatch(n, blob)
    a.plc_enable(api.PLC_CAUSAL)
    a.dred_enable(ML)
    assert a.plc_flavour() == 1 and a.dred_flavour() == 1
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        buf = a.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), count, first, take, hip_stream=st.cuda_stream)
        dropped = a.plc_fec_feed_device(buf.data_ptr(), take, hip_stream=st.cuda_stream)
    a.sync()
    assert not dropped.any()
    got, got_state = steps(a)
    a.close()
    h = api.LPCNetBatch(n, blob)
    h.plc_enable(api.PLC_CAUSAL)
    assert not h.plc_fec_feed(vectors, take).any()
    ref, ref_state = steps(h)
    h.plc_reset()
    bare, _ = steps(h)                                      # (the vectors matter: without them the concealment differs)
    h.close()
    assert np.array_equal(got, ref) and got_state == ref_state
    assert not np.array_equal(bare[:, 3:6], ref[:, 3:6])


def test_the_flavour_follows_the_blob_and_a_mismatch_is_refused(cases):
    b = api.LPCNetBatch(2, cases["small"][0])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_flavour()
    b.dred_enable(2)
    assert b.dred_flavour() == 1
    b.close()
    f = api.LPCNetBatch(2, dm.set_blob("small"))
    f.dred_enable(2)
    assert f.dred_flavour() == 0
    f.close()
    w = dm.SETS["small"]["widths"]
    nb = api.LPCNetBatch(2, dm.blob_dred(w, 36, gru_flavour="int8"))          # int8 arrays beside a float model
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*int8.*float"):
        nb.dred_enable(2)
    nb.close()
    nb = api.LPCNetBatch(2, synth.blob_bytes(dm.add_dred(synth.make_model(flavour="int8"), w, 36)))          # float arrays beside an int8 model
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*float.*int8"):
        nb.dred_enable(2)
    nb.close()
