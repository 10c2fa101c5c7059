"""Streams that come and go on the device: the active prefix (lpcnet_batch_set_active), the device-side stream copies (lpcnet_batch_copy_streams)
and the roster that keeps a server's streams dense (lpcnet_amd/roster.py).  A few frames on at most a few dozen streams per case; every
comparison is on bit patterns, against the oracle, the committed fixtures or an undisturbed batch (whose outputs the other test files pin to
the fixtures)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plc_fec_script as fs  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402
from lpcnet_amd.roster import StreamRoster  # noqa: E402
from test_gpu_parity import feats_for, oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345
CAP, T3 = 20, 3


def raw(b, s):
    return bytes(b.get_state(s))


def pad(rows, n, fill=0):
    """rows of the active streams -> an array for the whole capacity"""
    rows = np.asarray(rows)
    out = np.full((n,) + rows.shape[1:], fill, rows.dtype)
    out[:len(rows)] = rows
    return out


@pytest.fixture(scope="module")
def feats20():
    return feats_for(range(8100, 8100 + CAP), T3)


@pytest.fixture(scope="module")
def oracle13(blob_f32, feats20):
    return oracle_run(blob_f32, feats20[:13])[0]


# ---------------------------------------------------------------------------------------------------------- 1. the prefix is a smaller batch
@pytest.mark.parametrize("S", [1, 2, 4, 8, 0], ids=["S1", "S2", "S4", "S8", "auto"])
def test_prefix_is_a_smaller_batch(S, blob_f32, feats20, oracle13, hip_lib):
    b = api.LPCNetBatch(CAP, blob_f32)
    if S:
        b.streams_per_workgroup = S
    assert b.active == CAP and b.active_streams == CAP
    b.synthesize(feats_for(range(8200, 8200 + CAP), 1))     # every stream has a state of its own
    for active in (13, 3):      # (13 at eight per workgroup: the second workgroup has one group full and one stream in the other)
        b.reset(0, active)
        b.active = active
        assert b.active == active and b.active_streams == active
        before = [raw(b, s) for s in range(active, CAP)]
        pcm = b.synthesize(feats20, preload_pcm=np.full((CAP, T3 * 160), SENTINEL, np.int16), preload=0)
        assert np.array_equal(pcm[:active], oracle13[:active])
        assert (pcm[active:] == SENTINEL).all()
        assert [raw(b, s) for s in range(active, CAP)] == before
        small = api.LPCNetBatch(active, blob_f32)
        if S:
            small.streams_per_workgroup = S
        assert np.array_equal(small.synthesize(feats20[:active]), pcm[:active])
        assert all(raw(small, s) == raw(b, s) for s in range(active))
        small.close()
    b.close()


def test_prefix_against_the_committed_fixture(blob_f32, golden, hip_lib):
    T = int(golden["n_frames"])
    b = api.LPCNetBatch(8, blob_f32)
    b.active = 3
    pcm = b.synthesize(pad(feats_for([1000, 1001, 1002], T), 8))
    for s, seed in enumerate((1000, 1001, 1002)):
        assert np.array_equal(pcm[s], golden[f"pcm_gf_{seed}"])
        assert np.array_equal(np.array(b.get_state(s).gru_a, np.float32), golden[f"gru_a_gf_{seed}"])
    assert not pcm[3:].any()
    b.close()


def test_prefix_int8(blob_i8, hip_lib):
    feats = feats_for(range(8300, 8309), T3)
    want = oracle_run(blob_i8, feats[:5])[0]
    b = api.LPCNetBatch(9, blob_i8)
    b.active = 5
    before = [raw(b, s) for s in range(5, 9)]
    pcm = b.synthesize(feats, preload_pcm=np.full((9, T3 * 160), SENTINEL, np.int16), preload=0)
    assert np.array_equal(pcm[:5], want) and (pcm[5:] == SENTINEL).all()
    assert [raw(b, s) for s in range(5, 9)] == before
    b.close()


# ---------------------------------------------------------------------------------------------------------- 2. a moved stream carries on
@pytest.mark.parametrize("through_roster", [False, True], ids=["calls", "roster"])
def test_a_moved_stream_carries_on(through_roster, blob_f32, hip_lib):
    fa = feats_for(range(8400, 8406), 8)
    fj = feats_for([8450], 2)
    a = api.LPCNetBatch(6, blob_f32)
    pa = a.synthesize(fa).reshape(6, 8, 160)
    b = api.LPCNetBatch(8, blob_f32)
    if through_roster:
        r = StreamRoster(batch=b)
        assert [r.join(("call", i)) for i in range(6)] == list(range(6)) and b.active == 6
    else:
        b.active = 6
    out = {s: [] for s in range(6)}
    p = b.synthesize(pad(fa[:, :4], 8)).reshape(8, 4, 160)
    for s in range(6):
        out[s].append(p[s])
    # stream 1 leaves: the last active stream takes its slot
    if through_roster:
        assert r.leave([("call", 1)]) == ([(5, 1)], [5]) and r.slots()[("call", 5)] == 1
    else:
        b.copy_streams([5], [1])
        b.active = 5
    assert b.active == 5
    who = [0, 5, 2, 3, 4]
    p = b.synthesize(pad(fa[who, 4:6], 8)).reshape(8, 2, 160)
    for slot, s in enumerate(who):
        out[s].append(p[slot])
    # a new stream joins in slot 5
    if through_roster:
        assert r.join("new") == 5
    else:
        b.reset(5, 1)
        b.active = 6
    p = b.synthesize(pad(np.concatenate([fa[who, 6:8], fj]), 8)).reshape(8, 2, 160)
    for slot, s in enumerate(who):
        out[s].append(p[slot])
        assert np.array_equal(np.concatenate(out[s]), pa[s]), s
        assert raw(b, slot) == raw(a, s), s
    fresh = api.LPCNetBatch(1, blob_f32)
    assert np.array_equal(fresh.synthesize(fj).reshape(2, 160), p[5]) and raw(fresh, 0) == raw(b, 5)
    for x in (a, b, fresh):
        x.close()


# ---------------------------------------------------------------------------------------------------------- 3. every subsystem moves
def test_decoder_vq_memory_moves(blob_f32, golden, hip_lib):
    api.set_codebooks(*synth.make_codebooks(5))
    rng = np.random.default_rng(31)
    pk = np.concatenate([golden["packets"][None, :4], rng.integers(0, 256, size=(2, 4, 8), dtype=np.uint8)])
    u = api.LPCNetBatch(3, blob_f32)
    want = np.concatenate([u.decode(pk[:, :2]), u.decode(pk[:, 2:])], axis=1)
    b = api.LPCNetBatch(5, blob_f32)
    b.active = 3
    first = b.decode(pad(pk[:, :2], 5))
    assert np.array_equal(first[:3], want[:, :1280]) and not first[3:].any()
    assert b.get_decoder_vq_mem(0).any() and not b.get_decoder_vq_mem(4).any()
    b.copy_streams([0, 1], [4, 3])
    assert np.array_equal(b.get_decoder_vq_mem(4).view(np.uint32), b.get_decoder_vq_mem(0).view(np.uint32))
    assert np.array_equal(b.get_decoder_vq_mem(3).view(np.uint32), b.get_decoder_vq_mem(1).view(np.uint32))
    b.active = 5
    second = b.decode(pk[[0, 1, 2, 1, 0], 2:])
    assert np.array_equal(second, want[[0, 1, 2, 1, 0], 1280:])
    # the accessor pair: a snapshot of the memory restores it
    mem = b.get_decoder_vq_mem(2)
    b.set_decoder_vq_mem(2, np.arange(18, dtype=np.float32))
    assert np.array_equal(b.get_decoder_vq_mem(2), np.arange(18, dtype=np.float32))
    b.set_decoder_vq_mem(2, mem)
    assert np.array_equal(b.get_decoder_vq_mem(2).view(np.uint32), u.get_decoder_vq_mem(2).view(np.uint32))
    u.close(); b.close()


def test_analysis_state_and_encoder_vq_memory_move(blob_f32, hip_lib):
    api.set_codebooks(*synth.make_codebooks(5))
    rng = np.random.default_rng(32)
    t = np.arange(2 * 640 + 4 * 160)
    pcm = np.stack([(6000 * np.sin(2 * np.pi * t * f / 16000.) + rng.normal(0, 300, t.size)).astype(np.int16) for f in (140., 230.)])
    head, p0, p1 = pcm[:, :640], pcm[:, 640:1280], pcm[:, 1280:]
    u = api.LPCNetBatch(2, blob_f32)
    wf, w0, w1 = u.analyze(head), u.encode(p0), u.encode(p1)
    b = api.LPCNetBatch(4, blob_f32)
    b.active = 2
    assert np.array_equal(b.analyze(pad(head, 4))[:2].view(np.uint32), wf.view(np.uint32))
    assert np.array_equal(b.encode(pad(p0, 4))[:2], w0)
    b.copy_streams([1, 0], [3, 2])
    assert b.get_analysis_state(3) == b.get_analysis_state(1) and any(b.get_analysis_state(3))
    assert np.array_equal(b.get_encoder_vq_mem(3).view(np.uint32), b.get_encoder_vq_mem(1).view(np.uint32)) and b.get_encoder_vq_mem(3).any()
    b.active = 4
    got = b.encode(p1[[0, 1, 0, 1]])
    assert np.array_equal(got, w1[[0, 1, 0, 1]])
    u.close(); b.close()


def test_kept_frame_products_move(blob_f32, hip_lib):
    f = feats_for([8500, 8501], 1)[:, 0]
    u = api.LPCNetBatch(2, blob_f32)
    z = np.zeros((2, 160), np.int16)
    u1 = u.synthesize_step(f, z, [80, 80], [0, 0], [1, 1])
    u2 = u.synthesize_step(f, z, [80, 80], [0, 0], [2, 2])
    b = api.LPCNetBatch(4, blob_f32)
    b.active = 2
    z4 = np.zeros((4, 160), np.int16)
    b1 = b.synthesize_step(pad(f, 4), z4, [80, 80, 999, -1], [0, 0, 7, 7], [1, 1, 9, 9])      # (the arguments of the inactive streams are not looked at)
    assert np.array_equal(b1[:2], u1) and not b1[2:].any()
    b.copy_streams([0, 1], [3, 2])
    b.active = 4
    b2 = b.synthesize_step(pad(f, 4), z4, [80] * 4, [0] * 4, [2] * 4)      # (a tail step needs the kept products: they came with the copy)
    assert np.array_equal(b2, u2[[0, 1, 1, 0]])
    assert raw(b, 3) == raw(u, 0) and raw(b, 2) == raw(u, 1)
    u.close(); b.close()


PLC_LOST = np.zeros((12, fs.N), np.uint8)
PLC_LOST[3:9, 1] = 1
PLC_LOST[5:7, 3] = 1
PLC_LOST[[2, 7], 4] = 1
PLC_COPY_AT = 8


@pytest.mark.parametrize("flavour", ["float", "int8"])
def test_plc_streams_move_mid_run(flavour, hip_lib):
    """Twelve frames of the FEC script's five streams (its vectors, skips and clears; the loss pattern above) in LPCNET_PLC_CODEC |
    LPCNET_PLC_DC_FILTER.  Before step 8 stream 1 is in the middle of its outage (lost in steps 3..8) with 97 vectors in its FEC ring, stream 3
    has just come out of one and holds 80 samples in its PCM queue, and stream 0 has four vectors in its deferred feature queue and a full ring
    -- the host planner's control state says so (one stream cannot have all three: the queues are empty during an outage).  All three are
    copied there and run on beside their sources."""
    blob = synth.blob_bytes(plc_synth.make_model_with_plc(flavour=flavour))
    sc = fs.script()
    opt = api.PLC_CODEC | api.PLC_DC_FILTER
    N, CAPN = fs.N, 8

    def step(bt, t, rows):
        """step t for the batch's streams: slot i carries stream rows[i] of the script"""
        r0 = fs.step_rows(sc, t)[0]
        starts = r0 + np.concatenate([[0], np.cumsum(sc["count"][t])[:-1]])
        vec = [sc["vec"][starts[s]:starts[s] + sc["count"][t, s]] for s in rows]
        n = bt.n
        count, skip, clear = (pad(sc[k][t, rows], n) for k in ("count", "skip", "clear"))
        lost = pad(PLC_LOST[t, rows], n, 1)                  # (lost = 1 on the inactive streams changes nothing)
        skip[len(rows):] = 3
        clear[len(rows):] = 1
        dropped = bt.plc_fec_feed(vec + [np.zeros((0, 20), np.float32)] * (n - len(rows)), count, skip, clear)
        assert not dropped[len(rows):].any()
        frame = pad(sc["pcm"][rows, t], n)
        frame[lost != 0] = 0
        return bt.plc_step(frame, lost)

    u = api.LPCNetBatch(N, blob)
    u.plc_enable(opt)
    want = np.stack([step(u, t, list(range(N))) for t in range(12)], axis=1)
    b = api.LPCNetBatch(CAPN, blob)
    b.plc_enable(opt)
    b.active = N
    idle = [b.get_plc_state(s) for s in range(N, CAPN)]
    for t in range(PLC_COPY_AT):
        assert np.array_equal(step(b, t, list(range(N)))[:N], want[:, t])
    assert [b.get_plc_state(s) for s in range(N, CAPN)] == idle and [raw(b, s) for s in range(N, CAPN)] == [raw(b, CAPN - 1)] * (CAPN - N)
    ctl = np.stack([np.frombuffer(b.get_plc_state(s)[:36], np.int32) for s in range(N)])
    assert ctl[1, 2] == 1 and ctl[1, 4] > ctl[1, 6] > 0      # stream 1: blend set -- mid-outage --, unread vectors in the ring
    assert ctl[3, 0] == 80                                   # stream 3: samples in the PCM queue
    assert ctl[0, 8] == 4 and ctl[0, 4] == 100               # stream 0: deferred features, a full ring
    # a count on an inactive stream is refused and no ring has moved
    states = [b.get_plc_state(s) for s in range(CAPN)]
    bad = np.zeros(CAPN, np.int32)
    bad[N + 1] = 1
    with pytest.raises(api.LPCNetError):
        b.plc_fec_feed(np.zeros((1, 20), np.float32), bad)
    assert [b.get_plc_state(s) for s in range(CAPN)] == states
    b.copy_streams([1, 3, 0], [5, 6, 7])
    for s, d in ((1, 5), (3, 6), (0, 7)):
        assert b.get_plc_state(d) == b.get_plc_state(s) and raw(b, d) == raw(b, s)
        assert b.get_analysis_state(d) == b.get_analysis_state(s)
    b.active = CAPN
    rows = list(range(N)) + [1, 3, 0]
    for t in range(PLC_COPY_AT, 12):
        assert np.array_equal(step(b, t, rows), want[rows, t]), t
    for slot, s in enumerate(rows):
        assert b.get_plc_state(slot) == u.get_plc_state(s) and raw(b, slot) == raw(u, s)
    u.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 4. arguments
def test_bad_pair_lists_and_counts_are_refused_with_nothing_changed(blob_f32, hip_lib):
    b = api.LPCNetBatch(6, blob_f32)
    b.synthesize(feats_for(range(8600, 8606), 1))
    states = [raw(b, s) for s in range(6)]
    for src, dst in (([0, 1], [2, 2]), ([0, 1], [1, 2]), ([0, 2], [1, 0]), ([0], [0]), ([0], [6]), ([-1], [0]), ([6], [0])):
        with pytest.raises(api.LPCNetError):
            b.copy_streams(src, dst)
    assert [raw(b, s) for s in range(6)] == states
    for bad in (7, -1, [3, 3]):
        with pytest.raises(api.LPCNetError):
            b.active = bad
    assert b.active == 6
    b.copy_streams([], [])                                   # nothing to do
    b.copy_streams([0, 0], [4, 5])                           # one source, two destinations
    assert raw(b, 4) == states[0] and raw(b, 5) == states[0] and [raw(b, s) for s in range(4)] == states[:4]
    b.active = 0                                             # nothing is launched, every call returns
    pcm = b.synthesize(feats_for(range(8600, 8606), 2))
    assert not pcm.any() and [raw(b, s) for s in range(4)] == states[:4]
    b.close()


# ---------------------------------------------------------------------------------------------------------- 5. ordering
def test_enqueued_calls_keep_the_count_they_were_enqueued_with(blob_f32, hip_lib):
    import torch
    feats = feats_for(range(8700, 8706), 4)
    st = torch.cuda.current_stream().cuda_stream

    def run(sync):
        b = api.LPCNetBatch(6, blob_f32)
        d_f = torch.from_numpy(feats).cuda()
        p1 = torch.full((6, 2 * 160), SENTINEL, dtype=torch.int16, device="cuda")
        p2 = torch.full((6, 2 * 160), SENTINEL, dtype=torch.int16, device="cuda")
        d_f2 = d_f[:, 2:].contiguous()
        torch.cuda.synchronize()
        b.active = 5
        b.synthesize_device(d_f[:, :2].contiguous().data_ptr(), 36, p1.data_ptr(), 2, st)
        if sync:
            torch.cuda.synchronize(); b.sync()
        b.active = 3
        b.copy_streams([4], [1], st)
        if sync:
            torch.cuda.synchronize(); b.sync()
        b.synthesize_device(d_f2.data_ptr(), 36, p2.data_ptr(), 2, st)
        torch.cuda.synchronize(); b.sync()
        out = p1.cpu().numpy(), p2.cpu().numpy(), [raw(b, s) for s in range(6)]
        b.close()
        return out

    a1, a2, sa = run(True)
    b1, b2, sb = run(False)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2) and sa == sb
    assert (a1[5:] == SENTINEL).all() and (a1[:5] != SENTINEL).any(axis=1).all()      # the first call ran five streams ...
    assert (a2[3:] == SENTINEL).all() and (a2[:3] != SENTINEL).any(axis=1).all()      # ... the second three
    want = oracle_run(blob_f32, np.concatenate([feats[[4], :2], feats[[1], 2:]], axis=1))[0]      # slot 1 carries on as stream 4
    assert np.array_equal(a2[1], want[0, 320:])


# ---------------------------------------------------------------------------------------------------------- 6. shards
def test_two_shards_on_one_device(blob_f32, hip_lib):
    import torch
    feats = feats_for(range(8800, 8812), 4)
    u = api.LPCNetBatch(12, blob_f32)
    want = u.synthesize(feats).reshape(12, 4, 160)
    b = api.LPCNetBatch(12, blob_f32, devices=[0, 0])
    assert [(f, c) for f, c, _ in b.shards] == [(0, 6), (6, 6)] and b.active == [6, 6]
    with pytest.raises(api.LPCNetError):
        b.active = [2, 7]
    with pytest.raises(api.LPCNetError):
        b.active = 5                                         # one count per shard
    b.active = [2, 5]
    assert b.active == [2, 5] and b.active_streams == 7
    live = [0, 1, 6, 7, 8, 9, 10]
    p = b.synthesize(feats[:, :1], preload_pcm=np.full((12, 160), SENTINEL, np.int16), preload=0)
    assert np.array_equal(p[live], want[live, 0]) and (np.delete(p, live, axis=0) == SENTINEL).all()
    # the _shard device calls: a shard's arrays are [count_k][...], its active rows lead
    for k, (first, act) in enumerate(((0, 2), (6, 5))):
        d_f = torch.from_numpy(feats[first:first + 6, 1:2].copy()).cuda()
        d_p = torch.full((6, 160), SENTINEL, dtype=torch.int16, device="cuda")
        b.synthesize_device_shard(k, d_f.data_ptr(), 36, d_p.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize(); b.sync()
        got = d_p.cpu().numpy()
        assert np.array_equal(got[:act], want[first:first + act, 1]) and (got[act:] == SENTINEL).all()
    # one list: stream 7 -> slot 2 across the shards, stream 6 -> slot 11 inside the second
    b.copy_streams([7, 6], [2, 11])
    assert raw(b, 2) == raw(b, 7) and raw(b, 11) == raw(b, 6)
    b.active = [3, 6]
    rows = [0, 1, 7, 3, 4, 5, 6, 7, 8, 9, 10, 6]
    p = b.synthesize(feats[rows, 2:]).reshape(12, 2, 160)
    for slot in (0, 1, 2, 6, 7, 8, 9, 10, 11):
        assert np.array_equal(p[slot], want[rows[slot], 2:]), slot
        assert raw(b, slot) == raw(u, rows[slot])
    assert not p[3:6].any()
    u.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 7. FAST
@pytest.mark.parametrize("two_group,active", [(False, 5), (True, 13)], ids=["table-5of16", "two-group-13of16"])
def test_fast_output_is_that_of_a_batch_of_the_active_count(two_group, active, blob_f32, hip_lib):
    feats = feats_for(range(8900, 8916), T3)

    def make(n):
        b = api.LPCNetBatch(n, blob_f32)
        if two_group:
            b.fast_two_group = True
        b.set_fast(True)
        if two_group:
            b.streams_per_workgroup = 8
        return b

    b, small = make(16), make(active)
    b.active = active
    got = b.synthesize(feats)
    assert np.array_equal(got[:active], small.synthesize(feats[:active])) and not got[active:].any()
    assert all(raw(b, s) == raw(small, s) for s in range(active))
    b.close(); small.close()
