"""The DRED decoder's FAST flavour on the device (lpcnet_batch_dred_set_fast; dred_fast_kernels.hip.h) against its yardstick: the envelope between
the reference's generic-C float build and its AVX2+FMA float build on the same inputs (tests/golden/golden_dred_fast_v1.npz, made by
tests/tools/make_golden_dred_fast.py).  At every latent index max |FAST - gf| <= the fixture's envelope at that index, with no slack; everything
about tiling, independence, isolation and the forms of the call is compared on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_model as dm  # noqa: E402
import make_golden_dred_fast as mf  # noqa: E402
import plc_model as pm  # noqa: E402
from lpcnet_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

N, ML = dm.N_STREAMS, dm.N_LATENTS
SENTINEL = np.float32(-12345.678)
TILES = (16, 32)                 # every tile that is built
MODES = TILES + (1,)             # ... and the engine's choice
NT = mf.TILE_STREAMS


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold(hip_lib):
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_fast_v1.npz"))


@pytest.fixture(scope="module")
def gold_parity():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_v1.npz"))


def fresh(n=N, ml=ML):
    return np.full((n, 4 * ml, 20), SENTINEL, np.float32)


def assert_inside(got, gf, env, count, what=""):
    """per latent index max |got - gf| over the streams that decode it <= env; rows past 4 count[s] still hold the sentinel.  Returns the worst
    ratio deviation / envelope"""
    worst = 0.0
    count = np.asarray(count)
    for s in range(got.shape[0]):
        assert (bits(got[s, 4 * int(count[s]):]) == bits(SENTINEL)).all(), (what, s, "rows past the count were written")
    for l in range(len(env)):
        live = count > l
        if not live.any():
            continue
        dev = float(np.abs(got[live, 4 * l:4 * l + 4].astype(np.float64) - gf[live, 4 * l:4 * l + 4].astype(np.float64)).max())
        print("%s latent %d: deviation %.3g envelope %.3g" % (what, l, dev, float(env[l])))
        assert np.isfinite(dev) and dev <= float(env[l]), (what, l, dev, float(env[l]))
        worst = max(worst, dev / float(env[l]))
    return worst


@pytest.fixture(scope="module")
def tile_case(gold):
    """the 69-stream case on the small set: blob, inputs, counts, and FAST's own output at T = 32, decoded once: what the other tile and every regrouping of the streams must reproduce bit for bit"""
    blob = dm.set_blob(mf.TILE_SET)
    state, latents = mf.tile_inputs()
    count = mf.tile_counts()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes() + count.tobytes())) == gold["tile_in_crc"]
    b = api.LPCNetBatch(NT, blob)
    b.dred_enable(ML)
    b.dred_fast = 32
    out = b.dred_decode(state, latents, count, fresh(NT))
    b.close()
    return blob, state, latents, count, out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(dm.SETS))
def test_envelope_on_the_three_width_sets(name, mode, gold, gold_parity):
    blob = dm.set_blob(name)
    state, latents = dm.set_inputs(name)
    assert np.uint32(zlib.crc32(blob)) == gold["blob_crc_" + name] and np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold["in_crc_" + name]
    gf = gold_parity["feat_" + name]
    b = api.LPCNetBatch(N, blob)
    b.dred_enable(ML)
    b.dred_fast = mode
    assert b.dred_fast == mode
    got = b.dred_decode(state, latents, dm.COUNT, fresh())
    b.close()
    worst = assert_inside(got, gf, gold["env_" + name], dm.COUNT, "%s mode %d" % (name, mode))
    print("%s mode %d: worst deviation / envelope %.4f" % (name, mode, worst))
    if name == "w256":          # the switch did something
        live = np.concatenate([bits(got[s, :4 * int(dm.COUNT[s])]).ravel() != bits(gf[s, :4 * int(dm.COUNT[s])]).ravel() for s in range(N)])
        assert live.any()


@pytest.mark.parametrize("tile", TILES)
def test_tiling_69_streams(tile, gold, tile_case):
    blob, state, latents, count, base = tile_case
    b = api.LPCNetBatch(NT, blob)
    b.dred_enable(ML)
    b.dred_fast = tile
    got = b.dred_decode(state, latents, count, fresh(NT))
    b.close()
    worst = assert_inside(got, gold["tile_gf"], gold["tile_env"], count, "tiling T=%d" % tile)
    print("tiling T=%d: worst deviation / envelope %.4f" % (tile, worst))
    assert np.array_equal(bits(got), bits(base))          # the same bits in every tile size


def test_a_streams_bits_do_not_depend_on_its_neighbours(tile_case):
    blob, state, latents, count, base = tile_case
    # three streams alone
    pick = [3, 40, 68]
    b = api.LPCNetBatch(3, blob)
    b.dred_enable(ML)
    b.dred_fast = 1
    got = b.dred_decode(state[pick], latents[pick], count[pick], fresh(3))
    b.close()
    assert count[pick].min() > 0 and np.array_equal(bits(got), bits(base[pick]))
    # all 69 in reversed order
    b = api.LPCNetBatch(NT, blob)
    b.dred_enable(ML)
    b.dred_fast = 1
    got = b.dred_decode(state[::-1], latents[::-1], count[::-1], fresh(NT))
    assert np.array_equal(bits(got[::-1]), bits(base))
    # an active prefix of 40, zero counts beyond it: the inactive rows are untouched
    b.active = 40
    c40 = count.copy()
    c40[40:] = 0
    got = b.dred_decode(state, latents, c40, fresh(NT))
    b.active = NT
    b.close()
    assert np.array_equal(bits(got[:40]), bits(base[:40])) and (bits(got[40:]) == bits(SENTINEL)).all()
    # two unequal shards on one device
    sb = api.LPCNetBatch(NT, blob, devices=[0, 0])
    assert sb.shards[0][1] != sb.shards[1][1]
    sb.dred_enable(ML)
    sb.dred_fast = 1
    got = sb.dred_decode(state, latents, count, fresh(NT))
    sb.close()
    assert np.array_equal(bits(got), bits(base))


def test_nan_and_inf_latents_stay_in_their_stream(tile_case):
    blob, state, latents, count, base = tile_case
    bad = 35                      # (inside the second tile of 32, a stream that decodes)
    lat = latents.copy()
    c = count.copy()
    c[bad] = ML
    lat[bad, 0, ::2] = np.nan
    lat[bad, 1, 1::3] = np.inf
    lat[bad, 2, 5] = -np.inf
    b = api.LPCNetBatch(NT, blob)
    b.dred_enable(ML)
    b.dred_fast = 1
    got = b.dred_decode(state, lat, c, fresh(NT))
    b.close()
    others = np.arange(NT) != bad
    assert np.array_equal(bits(got[others]), bits(base[others]))
    assert not np.isfinite(got[bad, :4]).all()


@pytest.mark.parametrize("mode", [16, 32, 1])
def test_long_chain(mode, gold):
    state, latents = dm.long_inputs()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold["long_in_crc"]
    b = api.LPCNetBatch(dm.LONG_STREAMS, dm.set_blob("w256"))
    b.dred_enable(dm.LONG_LATENTS)
    b.dred_fast = mode
    got = b.dred_decode(state, latents, dm.LONG_COUNT, fresh(dm.LONG_STREAMS, dm.LONG_LATENTS))
    b.close()
    worst = assert_inside(got, gold["long_gf"], gold["long_env"], dm.LONG_COUNT, "long mode %d" % mode)
    print("long run mode %d: worst deviation / envelope %.4f" % (mode, worst))


def test_forms_of_the_call(gold_parity):
    import torch
    name = "mixed"
    blob = dm.set_blob(name)
    state, latents = dm.set_inputs(name)
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state).to(dev), torch.from_numpy(latents).to(dev)
    b = api.LPCNetBatch(N, blob)
    b.dred_enable(ML)
    b.dred_fast = 1
    host = b.dred_decode(state, latents, dm.COUNT, fresh())
    assert not np.array_equal(bits(host), bits(np.where(np.arange(4 * ML)[None, :, None] < 4 * dm.COUNT[:, None, None], gold_parity["feat_" + name], SENTINEL)))
    # the device form on the batch's own stream and on a caller's
    d_out = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out.data_ptr())
    b.sync()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(host))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_out2 = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
        b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out2.data_ptr(), hip_stream=st.cuda_stream)
        got = d_out2.cpu().numpy()
    assert np.array_equal(bits(got), bits(host))
    # the packed form: dm.packed of the plain output
    first = np.array([0, 1, 0, 2, 0, 0, 27, 3, 5], np.int32)
    take = np.array([28, 3, 0, 5, 0, 12, 1, 9, 11], np.int32)
    assert (first + take <= 4 * dm.COUNT).all()
    torch.cuda.synchronize()
    out = b.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, first, take)
    b.sync()
    assert np.array_equal(bits(out.cpu().numpy()), bits(dm.packed(host, first, take)))
    # a capture takes nothing, with the existing message
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, d_out2.data_ptr(), hip_stream=cs)
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_decode_packed(d_state.data_ptr(), d_lat.data_ptr(), dm.COUNT, [0] * N, 4 * dm.COUNT, hip_stream=cs)
        d_out2.add_(0)
    b.sync()
    b.close()


def test_fast_redundancy_goes_into_the_plc_without_a_host_hop():
    """the shape of test_gpu_dred.py's PLC test: one batch fed by dred_decode_packed (FAST) -> plc_fec_feed_device on one stream, the other by the host
    feed with the FAST vectors; then twelve steps with a five-frame loss"""
    import torch
    n = 8
    blob = dm.set_blob("mixed", with_plc=True)
    state, latents = dm.set_inputs("mixed")
    count = dm.COUNT[:n]
    first = np.zeros(n, np.int32)
    take = (4 * count).astype(np.int32)
    take[4], first[6], take[6] = 6, 3, 9
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
    a.dred_fast = 1
    plain = a.dred_decode(state[:n], latents[:n], count, np.zeros((n, 4 * ML, 20), np.float32))
    vectors = dm.packed(plain, first, take)
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
    bare, _ = steps(h)
    h.close()
    assert np.array_equal(got, ref) and got_state == ref_state
    assert not np.array_equal(bare[:, 4:9], ref[:, 4:9])


def test_the_switch(gold_parity):
    import dred_i8_model as di
    name = "small"
    blob = dm.set_blob(name)
    state, latents = dm.set_inputs(name)
    want = gold_parity["feat_" + name]

    def parity_bits(got):
        for s in range(N):
            k = 4 * int(dm.COUNT[s])
            assert np.array_equal(bits(got[s, :k]), bits(want[s, :k])), s
            assert (bits(got[s, k:]) == bits(SENTINEL)).all()

    b = api.LPCNetBatch(N, blob)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_fast = 1
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_fast
    b.dred_enable(ML)
    assert b.dred_fast == 0
    for bad in (-1, 2, 8, 64, 33):          # (64 is not built)
        with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
            b.dred_fast = bad
    assert b.dred_fast == 0
    b.dred_fast = 1
    fast = b.dred_decode(state, latents, dm.COUNT, fresh())
    assert not np.array_equal(bits(fast), bits(np.where(np.arange(4 * ML)[None, :, None] < 4 * dm.COUNT[:, None, None], want, SENTINEL)))
    b.dred_fast = 0
    assert b.dred_fast == 0 and b.dred_form() == 1          # (dred_form keeps describing the PARITY forms)
    parity_bits(b.dred_decode(state, latents, dm.COUNT, fresh()))
    b.set_fast(True)                           # the sample kernel's switch does not touch the decoder
    assert b.dred_fast == 0
    parity_bits(b.dred_decode(state, latents, dm.COUNT, fresh()))
    b.close()
    # an int8 decoder has no FAST form yet: refused, nothing changes
    gi = np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_i8_v1.npz"))
    q = api.LPCNetBatch(N, di.blob_dec(name))
    q.dred_enable(ML)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*int8 decoder has no FAST form"):
        q.dred_fast = 1
    assert q.dred_fast == 0
    got = q.dred_decode(state, latents, dm.COUNT, fresh())
    q.close()
    for s in range(N):
        k = 4 * int(dm.COUNT[s])
        assert np.array_equal(bits(got[s, :k]), bits(gi["feat_" + name][s, :k])), s
