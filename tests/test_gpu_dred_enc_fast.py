"""The DRED encoder's FAST flavour on the device (lpcnet_batch_dred_enc_set_fast; rdovae_enc_fast_kernels.hip.h) against its yardstick: the envelope
between the reference's generic-C float build and its AVX2+FMA float build on the same inputs (tests/golden/golden_dred_enc_fast_v1.npz, made by
tests/tools/make_golden_dred_enc_fast.py).  At every double-frame index max |FAST - gf| <= the fixture's envelope at that index, with no slack, for
latents, initial states and the final state; everything about tiling, independence, chunking, state moves, isolation, the forms of the call and the
switch is compared on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_enc_model as em  # noqa: E402
import make_golden_dred_enc_fast as mk  # noqa: E402
from lpcnet_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

N, MD = em.N_STREAMS, em.N_DFRAMES
SENTINEL = np.float32(-12345.678)
TILES = (16, 32)                 # every tile that is built
MODES = TILES + (1,)             # ... and the engine's choice
NT = mk.TILE_STREAMS


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def gold(hip_lib):
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_fast_v1.npz"))


@pytest.fixture(scope="module")
def gold_parity():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_v1.npz"))


def dims(name):
    s = em.SETS[name]
    return s["latent_dim"], s["state_dim"]


def fresh(name, n=N, md=MD):
    ld, sd = dims(name)
    return np.full((n, md, ld), SENTINEL, np.float32), np.full((n, md, sd), SENTINEL, np.float32)


def states_of(b, n):
    return np.stack([b.get_dred_enc_state(s) for s in range(n)])


def chunk(feat, first, count, md):
    """the call's feature array: stream s's double frames first[s] .. first[s] + count[s] - 1 at rows 0 .., the rest poisoned"""
    out = np.full((feat.shape[0], 2 * md, 20), np.float32(3e4), np.float32)
    for s in range(feat.shape[0]):
        out[s, :2 * int(count[s])] = feat[s, 2 * int(first[s]):2 * int(first[s] + count[s])]
    return out


def encode(name, mode, feat, count, n=None, md=MD, blob=None, **kw):
    """a fresh batch at `mode`: -> (latents, initial states, every stream's state read back); rows past the counts hold the sentinel"""
    n = feat.shape[0] if n is None else n
    b = api.LPCNetBatch(n, em.set_blob(name) if blob is None else blob, **kw)
    b.dred_enc_enable(md)
    b.dred_enc_fast = mode
    assert b.dred_enc_fast == mode
    lat, init = b.dred_encode(feat, count, *fresh(name, n, md))
    st = states_of(b, n)
    b.close()
    return lat, init, st


def assert_sentinel(got, count, what=""):
    for g in got[:2]:
        for s in range(g.shape[0]):
            assert (bits(g[s, int(count[s]):]) == bits(SENTINEL)).all(), (what, s, "rows past the count were written")


@pytest.fixture(scope="module")
def tile_case(gold):
    """the 69-stream case on the narrow set: inputs, counts, and FAST's own output at T = 32, encoded once: what the other tile and every regrouping
    of the streams must reproduce bit for bit"""
    feat, count = mk.tile_inputs(), mk.tile_counts()
    assert np.uint32(zlib.crc32(feat.tobytes() + count.tobytes())) == gold["tile_in_crc"]
    return feat, count, encode(mk.TILE_SET, 32, feat, count)


@pytest.fixture(scope="module")
def tf_case(gold):
    """the nine streams at the training widths, FAST at T = 32 in one call: what every way of cutting and moving the run must reproduce"""
    feat = em.inputs()
    assert np.uint32(zlib.crc32(feat.tobytes())) == gold["in_crc"]
    return feat, encode("tf", 32, feat, em.COUNT)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(em.SETS))
def test_envelope_on_the_three_width_sets(name, mode, gold, gold_parity):
    blob, feat = em.set_blob(name), em.inputs()
    assert np.uint32(zlib.crc32(blob)) == gold["blob_crc_" + name] and np.uint32(zlib.crc32(feat.tobytes())) == gold["in_crc"]
    got = encode(name, mode, feat, em.COUNT)
    assert_sentinel(got, em.COUNT, name)
    gruf = gold_parity["gru_" + name].shape[1]
    env = np.stack([gold["env_%s_%s" % (k, name)] for k in ("lat", "init", "gru", "mem")])
    what = "%s mode %d" % (name, mode)
    # the conv memory's gf values: every stream's at the narrow set, stream 0's elsewhere
    mem = gold["mem_gf_narrow"] if name == "narrow" else gold_parity["mem_full_" + name][None]
    mem_streams = np.arange(N) if name == "narrow" else np.array([0])
    gf = (gold_parity["lat_" + name], gold_parity["init_" + name], gold_parity["gru_" + name])
    worst = mk.worst_ratio(got, gf, env, em.COUNT, gruf, what=what, kinds=(0, 1, 2))
    gf_mem = tuple(x[mem_streams] for x in gf[:2]) + (np.concatenate([gf[2][mem_streams], mem], 1),)
    worst = max(worst, mk.worst_ratio(got, gf_mem, env, em.COUNT, gruf, streams=mem_streams, what=what, kinds=(3,)))
    print("%s: worst deviation / envelope %.4f" % (what, worst))
    assert worst <= 1.0, (what, worst)
    assert not got[2][em.COUNT == 0].any()          # (a stream without a count is not touched)
    if name == "tf":            # the switch did something
        assert any(not np.array_equal(bits(got[0][s, :int(em.COUNT[s])]), bits(gf[0][s, :int(em.COUNT[s])])) for s in range(N))


@pytest.mark.parametrize("tile", TILES)
def test_tiling_69_streams(tile, gold, tile_case):
    feat, count, base = tile_case
    got = encode(mk.TILE_SET, tile, feat, count)
    assert_sentinel(got, count, "tiling")
    gruf = gold["tile_gru"].shape[1]
    env = np.stack([gold["tile_env_lat"], gold["tile_env_init"], gold["tile_env_gru"], np.zeros(MD, np.float32)])
    worst = mk.worst_ratio(got, (gold["tile_lat"], gold["tile_init"], gold["tile_gru"]), env, count, gruf, what="tiling T=%d" % tile, kinds=(0, 1, 2))
    print("tiling T=%d: worst deviation / envelope %.4f" % (tile, worst))
    assert worst <= 1.0
    assert same(got, base)          # the same bits in every tile size
    assert not got[2][count == 0].any()


def test_a_streams_bits_do_not_depend_on_its_neighbours(tile_case):
    feat, count, base = tile_case
    # three streams alone
    pick = [3, 40, 68]
    assert count[pick].min() > 0
    assert same(encode(mk.TILE_SET, 1, feat[pick], count[pick]), [x[pick] for x in base])
    # all 69 in reversed order
    assert same([x[::-1] for x in encode(mk.TILE_SET, 1, feat[::-1], count[::-1])], base)
    # an active prefix of 40, zero counts beyond it: rows, states and ring beyond it are untouched
    b = api.LPCNetBatch(NT, em.set_blob(mk.TILE_SET))
    b.dred_enc_enable(MD)
    b.dred_enc_fast = 1
    marks = {s: (np.arange(b.dred_enc_info()[6]) * 0.001 + s).astype(np.float32) for s in (40, 47, 68)}
    for s, v in marks.items():
        b.set_dred_enc_state(s, v)
    b.active = 40
    c40 = count.copy()
    c40[40:] = 0
    lat, init = b.dred_encode(feat, c40, *fresh(mk.TILE_SET, NT))
    b.active = NT
    st = states_of(b, NT)
    b.close()
    assert same((lat[:40], init[:40], st[:40]), [x[:40] for x in base]) and (bits(lat[40:]) == bits(SENTINEL)).all() and (bits(init[40:]) == bits(SENTINEL)).all()
    for s in range(40, NT):
        assert np.array_equal(bits(st[s]), bits(marks[s])) if s in marks else not st[s].any(), s
    # two unequal shards on one device
    sb = api.LPCNetBatch(NT, em.set_blob(mk.TILE_SET), devices=[0, 0])
    assert sb.shards[0][1] != sb.shards[1][1]
    sb.dred_enc_enable(MD)
    sb.dred_enc_fast = 1
    assert sb.dred_enc_fast == 1
    lat, init = sb.dred_encode(feat, count, *fresh(mk.TILE_SET, NT))
    st = states_of(sb, NT)
    sb.close()
    assert same((lat, init, st), base)


def test_nan_and_inf_features_stay_in_their_stream(tile_case):
    feat, count, base = tile_case
    bad = 35                      # (inside the second tile of 32, the third of 16)
    f, c = feat.copy(), count.copy()
    c[bad] = MD
    f[bad, 0, ::2] = np.nan
    f[bad, 3, 1::3] = np.inf
    f[bad, 4, 5] = -np.inf
    got = encode(mk.TILE_SET, 1, f, c)
    others = np.arange(NT) != bad
    assert same([x[others] for x in got], [x[others] for x in base])
    assert not np.isfinite(got[0][bad, 0]).all()


def run_in_calls(name, feat, count, plan, set_state_between=False):
    """the run cut into calls: plan = [(double frames, mode), ..]; set_state_between: every call on a fresh batch that gets the states through
    get_dred_enc_state / set_dred_enc_state.  -> (latents, initial, states) of the whole run"""
    n = feat.shape[0]
    md = max(k for k, _ in plan)
    b = api.LPCNetBatch(n, em.set_blob(name))
    b.dred_enc_enable(md)
    done = np.zeros(n, np.int32)
    lat, init = fresh(name, n, MD)
    for k, mode in plan:
        b.dred_enc_fast = mode
        cnt = np.clip(count - done, 0, k).astype(np.int32)
        l, i = b.dred_encode(chunk(feat, done, cnt, md), cnt, *fresh(name, n, md))
        for s in range(n):
            lat[s, done[s]:done[s] + cnt[s]], init[s, done[s]:done[s] + cnt[s]] = l[s, :cnt[s]], i[s, :cnt[s]]
            assert (bits(l[s, cnt[s]:]) == bits(SENTINEL)).all()
        done += cnt
        if set_state_between:
            st = states_of(b, n)
            b.close()
            b = api.LPCNetBatch(n, em.set_blob(name))
            b.dred_enc_enable(md)
            for s in range(n):
                b.set_dred_enc_state(s, st[s])
            assert same([states_of(b, n)], [st])          # (the reference's member order, head 0: what went in comes out)
    st = states_of(b, n)
    b.close()
    return lat, init, st


@pytest.mark.parametrize("name", ["tf", "narrow"])
def test_cutting_the_run_into_calls_changes_no_bit(name, tf_case):
    feat = em.inputs()
    base = tf_case[1] if name == "tf" else encode(name, 32, feat, em.COUNT)
    assert same(run_in_calls(name, feat, em.COUNT, [(3, 32), (4, 32)]), base)
    assert same(run_in_calls(name, feat, em.COUNT, [(4, 16), (3, 32)]), base)
    # three double frames, the states out and into a fresh batch, four more
    assert same(run_in_calls(name, feat, em.COUNT, [(3, 1), (4, 1)], set_state_between=True), base)


def test_copy_streams_carries_a_fast_stream_on(tf_case):
    feat, base = tf_case
    b = api.LPCNetBatch(N, em.set_blob("tf"))
    b.dred_enc_enable(4)
    b.dred_enc_fast = 1
    zero, c3 = np.zeros(N, np.int32), np.minimum(em.COUNT, 3).astype(np.int32)
    b.dred_encode(chunk(feat, zero, c3, 4), c3)
    b.copy_streams([0], [2])                  # (stream 2 has no count of its own: its slot is fresh)
    src, first, cnt = np.arange(N), np.zeros(N, np.int32), np.zeros(N, np.int32)
    src[2], first[2], cnt[2] = 0, 3, 4
    lat, init = b.dred_encode(chunk(feat[src], first, cnt, 4), cnt, *fresh("tf", N, 4))
    st = b.get_dred_enc_state(2)
    b.close()
    assert em.COUNT[0] == 7 and same((lat[2], init[2], st), (base[0][0, 3:], base[1][0, 3:], base[2][0]))


@pytest.mark.parametrize("mode", TILES)
def test_long_run(mode, gold):
    feat = em.long_inputs()
    assert np.uint32(zlib.crc32(feat.tobytes())) == gold["long_in_crc"]
    got = encode("tf", mode, feat, em.LONG_COUNT, md=em.LONG_DFRAMES)
    assert_sentinel(got, em.LONG_COUNT, "long")
    gruf = gold["long_gru"].shape[1]
    env = np.stack([gold["long_env_" + k] for k in ("lat", "init", "gru", "mem")])
    worst = mk.worst_ratio(got, (gold["long_lat"], gold["long_init"], gold["long_gru"]), env, em.LONG_COUNT, gruf, streams=mk.LONG_GF_STREAMS,
                           what="long mode %d" % mode, kinds=(0, 1, 2))
    print("long run mode %d: worst deviation / envelope %.4f" % (mode, worst))
    assert worst <= 1.0


def test_forms_of_the_call(tf_case):
    import torch
    feat, base = tf_case
    dev = torch.device("cuda:0")
    d_feat = torch.from_numpy(em.strided(feat, 36)).to(dev)
    poisoned = lambda md=MD: tuple(torch.from_numpy(x).to(dev) for x in fresh("tf", N, md))
    down = lambda pair: tuple(x.cpu().numpy() for x in pair)
    b = api.LPCNetBatch(N, em.set_blob("tf"))
    b.dred_enc_enable(MD)
    b.dred_enc_fast = 1
    # the device form on the batch's own stream (strided 36-float rows with fill behind the 20 floats) and on a caller's
    out = poisoned()
    torch.cuda.synchronize()
    b.dred_encode_device(d_feat.data_ptr(), 36, em.COUNT, out[0].data_ptr(), out[1].data_ptr())
    b.sync()
    assert same(down(out) + (states_of(b, N),), base)
    b.reset()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out2 = poisoned()
        b.dred_encode_device(d_feat.data_ptr(), 36, em.COUNT, out2[0].data_ptr(), out2[1].data_ptr(), hip_stream=st.cuda_stream)
        got = down(out2)
    assert same(got + (states_of(b, N),), base)
    # a host count array under capture is refused with the existing message
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_encode_device(d_feat.data_ptr(), 36, em.COUNT, out2[0].data_ptr(), out2[1].data_ptr(), hip_stream=cs)
        out2[0].add_(0)
    b.sync()
    b.close()
    # the uniform one-double-frame step captured and replayed twice equals two plain calls
    def two_steps(captured):
        b = api.LPCNetBatch(N, em.set_blob("tf"))
        b.dred_enc_enable(1)
        b.dred_enc_fast = 1
        d_in = torch.zeros((N, 2, 20), dtype=torch.float32, device=dev)
        d_lat, d_init = poisoned(1)
        torch.cuda.synchronize()
        step = lambda s=0: b.dred_encode_device(d_in.data_ptr(), 20, 1, d_lat.data_ptr(), d_init.data_ptr(), hip_stream=s)
        if captured:
            step()                        # (a first launch outside the capture)
            b.sync()
            b.reset()
            g, cst = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.graph(g, stream=cst):
                step(torch.cuda.current_stream().cuda_stream)
            assert not b.get_dred_enc_state(0).any()          # (the capture ran nothing)
        res = []
        for d in range(2):
            d_in.copy_(torch.from_numpy(feat[:, 2 * d:2 * d + 2]))
            torch.cuda.synchronize()
            if captured:
                g.replay()
            else:
                step()
                b.sync()
            torch.cuda.synchronize()
            res += [d_lat.cpu().numpy()[:, 0], d_init.cpu().numpy()[:, 0]]
        res.append(states_of(b, N))
        b.close()
        return res

    plain, replayed = two_steps(False), two_steps(True)
    assert same(plain, replayed)
    for s in range(N):                  # (every stream ran two; the one-call run has a stream's first COUNT[s])
        k = min(2, int(em.COUNT[s]))
        assert np.array_equal(bits(np.stack(plain[0:4:2], 1)[s, :k]), bits(base[0][s, :k])) and np.array_equal(bits(np.stack(plain[1:4:2], 1)[s, :k]), bits(base[1][s, :k]))


def test_fast_encoder_output_decodes_on_the_device_without_a_host_copy():
    """FAST encoder -> FAST decoder on one stream; the decoded features equal those of the same latents fed from the host"""
    import torch
    blob = em.set_blob("tf", with_dec=True)
    feat = em.inputs()
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(N, blob)
    b.dred_enc_enable(MD)
    b.dred_enable(MD)
    b.dred_enc_fast = 1
    b.dred_fast = 1
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
        out, lat, init = d_out.cpu().numpy(), d_lat.cpu().numpy(), d_init.cpu().numpy()
    host = b.dred_decode(init[:, MD - 1], lat[:, ::-1], dcount)
    b.close()
    assert np.array_equal(bits(out), bits(host)) and np.abs(out[list(em.RT_STREAMS)]).max() > 0 and np.isfinite(out).all()


def test_the_switch(gold_parity):
    import dred_i8_model as di
    name = "narrow"
    feat = em.inputs()
    want = (gold_parity["lat_" + name], gold_parity["init_" + name])

    def parity_bits(got, want=want):
        for g, w in zip(got, want):
            for s in range(N):
                k = int(em.COUNT[s])
                assert np.array_equal(bits(g[s, :k]), bits(w[s, :k])), s
                assert (bits(g[s, k:]) == bits(SENTINEL)).all()

    b = api.LPCNetBatch(N, em.set_blob(name))
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_enc_fast = 1
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_enc_fast
    b.dred_enc_enable(MD)
    assert b.dred_enc_fast == 0
    for bad in (-1, 2, 8, 64, 33):          # (64 is not built)
        with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
            b.dred_enc_fast = bad
    assert b.dred_enc_fast == 0
    b.dred_enc_fast = 1
    fast = b.dred_encode(feat, em.COUNT, *fresh(name))
    assert any(not np.array_equal(bits(fast[0][s, :int(em.COUNT[s])]), bits(want[0][s, :int(em.COUNT[s])])) for s in range(N))
    b.reset()
    b.dred_enc_fast = 0
    assert b.dred_enc_fast == 0 and b.dred_enc_form() == 1          # (dred_enc_form keeps describing the PARITY forms)
    parity_bits(b.dred_encode(feat, em.COUNT, *fresh(name)))
    b.reset()
    b.set_fast(True)                           # the sample kernel's switch does not reach the encoder ...
    assert b.dred_enc_fast == 0
    parity_bits(b.dred_encode(feat, em.COUNT, *fresh(name)))
    b.close()
    b = api.LPCNetBatch(N, em.set_blob("tf", with_dec=True))          # ... and neither does the decoder's
    b.dred_enc_enable(MD)
    b.dred_enable(MD)
    b.dred_fast = 1
    assert b.dred_enc_fast == 0 and b.dred_fast == 1
    parity_bits(b.dred_encode(feat, em.COUNT, *fresh("tf")), (gold_parity["lat_tf"], gold_parity["init_tf"]))
    b.close()
    # an int8 encoder has no FAST form yet: refused, nothing changes
    gi = np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_i8_v1.npz"))
    q = api.LPCNetBatch(N, di.blob_enc(name))
    q.dred_enc_enable(MD)
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*int8 encoder has no FAST form"):
        q.dred_enc_fast = 1
    assert q.dred_enc_fast == 0
    got = q.dred_encode(feat, em.COUNT, *fresh(name))
    q.close()
    parity_bits(got, (gi["lat_" + name], gi["init_" + name]))
