"""Long and wide GPU parity runs (the exposure of the barrier-free hand-off inside a workgroup and of the
chunked frame loop has to be comparable to the benchmark's, not 10^4 samples), plus the behaviour added in round 2:
the process-default model, lpcnet_synthesize with N > 160, device release / re-creation, ordering across caller
streams, and batches sharded over several devices by the C library itself.

Every stream has its OWN seeded feature file and is compared bit for bit (tolerance 0) with the plain-C oracle, which
runs on the host cores in a process pool (oracle.orc.synthesize_many)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lpcnet_amd import api, synth
from oracle import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def distinct_feats(first_seed, n, T):
    return np.stack([synth.make_features(first_seed + s, T) for s in range(n)])


def first_mismatch(got, want):
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else (int(bad[0][0]), int(bad[0][1]) // 160, int(bad[0][1]) % 160, int((got != want).any(axis=1).sum()))


@pytest.mark.parametrize("flavour,n,T,S", [("float", 256, 110, 4), ("float", 256, 30, 2), ("int8", 256, 40, 4)],
                         ids=["f32-256x110-S4", "f32-256x30-S2", "int8-256x40-S4"])
def test_256_distinct_streams_against_oracle(flavour, n, T, S, hip_lib):
    """256 distinct feature files, >= 100-frame chunk boundary crossed (T = 110), every stream checked."""
    blob = synth.blob_bytes(synth.make_model(flavour=flavour))
    feats = distinct_feats(30000, n, T)
    want = orc.synthesize_many(blob, feats)
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = S
    got = b.synthesize(feats)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    b.close()


@pytest.mark.parametrize("n,S", [(600, 2), (300, 1)], ids=["S2", "S1"])
def test_int8_two_workgroups_per_cu_variants(n, S, blob_i8, hip_lib, monkeypatch):
    """more workgroups than CUs: the int8 engine switches to its 128-VGPR variants (two workgroups per CU).  Same
    arithmetic, other register allocation: bit-exact against the oracle; FAST results equal the one-workgroup variant's."""
    T = 6
    feats = distinct_feats(70000, n, T)
    want = orc.synthesize_many(blob_i8, feats)
    b = api.LPCNetBatch(n, blob_i8)
    b.streams_per_workgroup = S
    got = b.synthesize(feats)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    b.reset()
    b.set_fast(True)
    b.streams_per_workgroup = S
    fast_packed = b.synthesize(feats)
    b.close()
    monkeypatch.setenv("LPCNET_HIP_PACK2", "0")
    b = api.LPCNetBatch(n, blob_i8)
    b.set_fast(True)
    b.streams_per_workgroup = S
    assert np.array_equal(b.synthesize(feats), fast_packed)
    b.close()


def test_1024_distinct_streams_full_occupancy(blob_f32, hip_lib):
    """BASELINE config 2 shape: 1024 DISTINCT streams, one workgroup of four per CU, all 1024 compared with the oracle."""
    n, T = 1024, 24
    feats = distinct_feats(40000, n, T)
    want = orc.synthesize_many(blob_f32, feats)
    b = api.LPCNetBatch(n, blob_f32)
    assert b.streams_per_workgroup == 4
    got = b.synthesize(feats)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    # a second pass continues every stream (state carried on the device), still exact
    more = distinct_feats(50000, n, 6)
    want2 = orc.synthesize_many(blob_f32, np.concatenate([feats, more], axis=1))[:, T * 160:]
    got2 = b.synthesize(more)
    assert first_mismatch(got2, want2) is None, first_mismatch(got2, want2)
    b.close()


def test_2048_distinct_float_streams_two_rounds_of_workgroups(blob_f32, hip_lib):
    """more workgroups than CUs for the float kernel: 2048 distinct streams at S = 4 = 512 workgroups on 256 CUs,
    a second round of workgroups on every CU; every stream compared with the oracle"""
    n, T = 2048, 12
    feats = distinct_feats(90000, n, T)
    want = orc.synthesize_many(blob_f32, feats)
    b = api.LPCNetBatch(n, blob_f32)
    b.streams_per_workgroup = 4
    got = b.synthesize(feats)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    b.close()


@pytest.mark.parametrize("flavour", ["float", "int8"])
def test_soak_1024_streams_two_seconds(flavour, hip_lib):
    """3.2e7 samples through the barrier-free index hand-off at full occupancy: 1024 distinct streams x 200 frames in one
    call (two 100-frame chunks); 64 streams spread over the workgroups (every position inside a workgroup) against the oracle"""
    blob = synth.blob_bytes(synth.make_model(flavour=flavour))
    n, T = 1024, 200
    feats = distinct_feats(80000, n, T)
    pick = np.array([(i * 16 + (i % 4)) % n for i in range(64)])
    want = orc.synthesize_many(blob, feats[pick])
    b = api.LPCNetBatch(n, blob)
    got = b.synthesize(feats)
    assert first_mismatch(got[pick], want) is None, first_mismatch(got[pick], want)
    assert np.all(np.abs(got.astype(np.int32)).max(axis=1) > 0)
    b.close()


def test_ten_second_files_past_frame_count_saturation(blob_f32, hip_lib):
    """1010 frames per stream: frame_count saturates at 1000 (src/lpcnet.c:119), ten 100-frame chunks + a partial one."""
    n, T = 4, 1010
    feats = distinct_feats(60000, n, T)
    want = orc.synthesize_many(blob_f32, feats)
    b = api.LPCNetBatch(n, blob_f32)
    b.streams_per_workgroup = 4
    got = b.synthesize(feats)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    assert b.get_state(0).frame_count == 1000
    b.close()


def test_synthesize_more_than_160_samples_per_call(blob_f32, hip_lib):
    """lpcnet_synthesize(st, f, out, N) for N > 160: one frame-network step, then N samples (src/lpcnet.c:235-281)."""
    f = synth.make_features(7100, 8)
    om = orc.OracleModel(blob_f32)
    o = om.new_state()
    st = api.LPCNetState(blob_f32)
    for t, n in enumerate((160, 400, 161, 57, 320, 160)):
        want = np.zeros(n, np.int16)
        o.L.orc_synthesize(o.p, np.ascontiguousarray(f[t, :20]), want, n, 0)
        assert np.array_equal(st.synthesize(f[t], n), want), (t, n)
    # teacher forcing across the 160-sample pieces (preload 200 of 300)
    forced = ((np.arange(200) * 53) % 3000 - 1500).astype(np.int16)
    want = np.zeros(300, np.int16); want[:200] = forced
    o.L.orc_synthesize(o.p, np.ascontiguousarray(f[6, :20]), want, 300, 200)
    out = np.zeros(300, np.int16); out[:200] = forced
    st.L.lpcnet_synthesize_impl(st.p, np.ascontiguousarray(f[6, :20]), out, 300, 200)
    assert np.array_equal(out, want)


def test_default_model_and_release(blob_f32, golden, hip_lib):
    """A state that never saw lpcnet_load_model runs on the process-default model (the reference binds its compiled-in
    model in lpcnet_init); lpcnet_hip_shutdown() releases the device side without invalidating bound states."""
    T = 10
    f = synth.make_features(1000, int(golden["n_frames"]))[:T]
    api.set_default_model(blob_f32)
    st = api.LPCNetState()                                   # no load_model
    first = np.concatenate([st.synthesize(f[t]) for t in range(4)])
    api.shutdown()                                           # device buffers, engine and stream are gone ...
    rest = np.concatenate([st.synthesize(f[t]) for t in range(4, T)])     # ... and come back on demand
    assert np.array_equal(np.concatenate([first, rest]), golden["pcm_gf_1000"][:T * 160])
    # two states interleaved on one model: the device-resident copy follows whichever state comes next
    a, b = api.LPCNetState(blob_f32), api.LPCNetState(blob_f32)
    fa, fb = synth.make_features(1001, 60)[:6], synth.make_features(1002, 60)[:6]
    pa, pb = [], []
    for t in range(6):
        pa.append(a.synthesize(fa[t]))
        pb.append(b.synthesize(fb[t]))
    assert np.array_equal(np.concatenate(pa), golden["pcm_gf_1001"][:960]) and np.array_equal(np.concatenate(pb), golden["pcm_gf_1002"][:960])


def test_default_model_from_file_in_a_fresh_process(tmp_path, blob_f32, golden, hip_lib):
    """./weights_blob.bin (the file name the reference's demo hard-codes) is picked up without any explicit call."""
    d = str(tmp_path)
    open(os.path.join(d, "weights_blob.bin"), "wb").write(blob_f32)
    code = ("import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from lpcnet_amd import api, synth\n"
            "st = api.LPCNetState()\n"
            "f = synth.make_features(1000, 60)\n"
            "np.concatenate([st.synthesize(f[t]) for t in range(5)]).tofile('out.pcm')\n" % ROOT)
    subprocess.check_call([sys.executable, "-c", code], cwd=d, timeout=600)
    assert np.array_equal(np.fromfile(os.path.join(d, "out.pcm"), np.int16), golden["pcm_gf_1000"][:800])


def test_calls_on_different_caller_streams_are_ordered(blob_f32, hip_lib):
    """Two device-pointer calls on two different non-blocking streams with no synchronisation in between, then
    lpcnet_batch_sync(): the second call continues the first one's state, and sync covers both streams."""
    import torch
    n, T = 8, 6
    feats = distinct_feats(7200, n, 2 * T)
    want = orc.synthesize_many(blob_f32, feats, workers=4)
    b = api.LPCNetBatch(n, blob_f32)
    d_f1 = torch.from_numpy(np.ascontiguousarray(feats[:, :T])).cuda()
    d_f2 = torch.from_numpy(np.ascontiguousarray(feats[:, T:])).cuda()
    d_p1 = torch.zeros((n, T * 160), dtype=torch.int16, device="cuda")
    d_p2 = torch.zeros((n, T * 160), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    b.synthesize_device(d_f1.data_ptr(), 36, d_p1.data_ptr(), T, s1.cuda_stream)
    b.synthesize_device(d_f2.data_ptr(), 36, d_p2.data_ptr(), T, s2.cuda_stream)
    b.sync()                                                 # (no torch synchronisation: the library's own)
    st = b.get_state(0)
    got = np.concatenate([d_p1.cpu().numpy(), d_p2.cpu().numpy()], axis=1)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    assert st.frame_count == 2 * T
    b.close()


def test_sharded_batch_in_c(blob_f32, golden, hip_lib):
    """lpcnet_batch_create_sharded: contiguous blocks of streams on several devices (here: as many shards as the box has
    GPUs, at least two -- a device may carry several shards), one host thread per shard, no exchange."""
    import torch
    ndev = torch.cuda.device_count()
    devices = list(range(ndev)) if ndev >= 2 else [0, 0, 0]
    n, T = 4 * len(devices) + 1, 7                           # ragged: the first shard gets one stream more
    feats = distinct_feats(7300, n, T)
    want = orc.synthesize_many(blob_f32, feats, workers=4)
    b = api.LPCNetBatch(n, blob_f32, devices=devices)
    sh = b.shards
    assert len(sh) == len(devices) and sh[0] == (0, 5, devices[0]) and sum(c for _, c, _ in sh) == n
    assert [f for f, _, _ in sh] == list(np.cumsum([0] + [c for _, c, _ in sh])[:-1])
    got = b.synthesize(feats)
    assert first_mismatch(got, want) is None
    one = api.LPCNetBatch(n, blob_f32)                       # the same on one device
    assert np.array_equal(one.synthesize(feats), got)
    # per-stream calls address the right shard: reset across a shard boundary, state export from the last shard
    b.reset(3, 4)
    again = b.synthesize(feats)
    cont = orc.synthesize_many(blob_f32, np.concatenate([feats, feats], axis=1), workers=4)[:, T * 160:]
    for s in range(n):
        assert np.array_equal(again[s], want[s] if 3 <= s < 7 else cont[s]), s
    st = api.LPCNetState(blob_f32)
    assert hip_lib.lpcnet_batch_export_state(b.p, n - 1, st.p) == 0
    s_one = one.get_state(n - 1)
    one.reset(0, n)
    # codec path over shards
    api.set_codebooks(*synth.make_codebooks(5))
    pk = np.stack([golden["packets"]] * n)
    b.reset()
    out = b.decode(pk)
    for s in range(n):
        assert np.array_equal(out[s], golden["packet_pcm_gf"].reshape(-1))
    # device pointers belong to one shard
    d_f = torch.from_numpy(np.ascontiguousarray(feats[sh[1][0]:sh[1][0] + sh[1][1]])).to(f"cuda:{sh[1][2]}")
    d_p = torch.zeros((sh[1][1], T * 160), dtype=torch.int16, device=f"cuda:{sh[1][2]}")
    with pytest.raises(api.LPCNetError):
        b.synthesize_device(d_f.data_ptr(), 36, d_p.data_ptr(), T)
    b.reset()
    b.synthesize_device_shard(1, d_f.data_ptr(), 36, d_p.data_ptr(), T)
    b.sync()
    assert np.array_equal(d_p.cpu().numpy(), want[sh[1][0]:sh[1][0] + sh[1][1]])
    assert s_one.frame_count == T
    b.close(); one.close()


def test_sharded_batch_calls_that_run_shard_after_shard(blob_f32, hip_lib):
    """The host-pointer calls whose shards run in turn hand every shard its own part of the caller's arrays: 5 streams as shards of 3 and 2
    on one device, 3 frames (two start-up frames and the first live one), bit for bit against the plain-C oracle.  The per-stream step with
    N = 40 on every stream against orc_synthesize with N; the frame network and the sample loop as two calls per frame against synthesize."""
    n, T, N = 5, 3, 40
    feats = distinct_feats(7400, n, T)
    om = orc.OracleModel(blob_f32)
    b = api.LPCNetBatch(n, blob_f32, devices=[0, 0])
    assert b.shards == [(0, 3, 0), (3, 2, 0)]
    ost = [om.new_state() for _ in range(n)]
    for t in range(T):
        got = b.synthesize_step(np.ascontiguousarray(feats[:, t]), np.zeros((n, 160), np.int16), [N] * n, [0] * n, [1] * n)
        for s in range(n):
            ref = np.zeros(160, np.int16)
            ost[s].L.orc_synthesize(ost[s].p, np.ascontiguousarray(feats[s, t, :20]), ref, N, 0)
            assert np.array_equal(got[s, :N], ref[:N]), (t, s)
    assert got[:, :N].any(axis=1).all()                      # (the third frame is live on every stream)
    b.reset()
    want = np.stack([om.new_state().synthesize(feats[s]) for s in range(n)])
    for t in range(T):
        ca, cb, lp = b.run_frames(np.ascontiguousarray(feats[:, t:t + 1]))
        assert np.array_equal(b.run_tail(ca, cb, lp), want[:, t * 160:(t + 1) * 160]), t
    assert want[:, 2 * 160:].any(axis=1).all()
    b.close()


@pytest.mark.parametrize("kw,n", [(dict(), 1024), (dict(densities=(0.07, 0.07, 0.25)), 1024), (dict(flavour="int8"), 1024), (dict(), 2560)],
                         ids=["default", "denseA", "int8", "default2560"])
def test_streams_per_workgroup_is_measured_not_looked_up(kw, n, hip_lib):
    """the streams-per-workgroup choice must come from THIS model (a denser GRU-A runs another item-count
    variant with other step times): the engine times S = 1, 2, 4 (8) on the batch itself before its first run.  The chosen
    value has to be (within noise) the fastest when each is pinned, the states must be untouched by the
    measurement (bit-exact output afterwards), and a pinned value must stay pinned.  The call that measures runs on the
    measured value itself, not on the table's (a one-shot user never makes a second call): its kernel time is a pinned batch's at
    the chosen value -- and where the table says otherwise (2560 float streams: 320 workgroups of eight against 640 of four, two rounds
    against three, which the table's step times put the other way round than this GPU) nearer to that than to the table's."""
    blob = synth.blob_bytes(synth.make_model(**kw))
    T = 6
    feats = distinct_feats(95000, n, T)
    auto = api.LPCNetBatch(n, blob)
    table = auto.streams_per_workgroup                       # (before the first run: the table's value)
    auto.enable_timing(True)
    pcm_auto = auto.synthesize(feats)
    t_first = auto.last_timing()[0]
    chosen = auto.streams_per_workgroup
    auto.close()
    times = {}
    for S in sorted({1, 2, 4, table, chosen}):
        b = api.LPCNetBatch(n, blob)
        b.streams_per_workgroup = S
        b.enable_timing(True)
        b.synthesize(feats)                                  # warm-up
        best = None
        for _ in range(3):                                   # best of three: a single timing on a shared GPU is a coin flip
            b.reset()
            out = b.synthesize(feats)
            t = b.last_timing()[0]
            best = t if best is None else min(best, t)
        times[S] = best
        assert b.streams_per_workgroup == S
        if S == chosen:
            assert np.array_equal(out, pcm_auto)             # the auto-tuned batch produced exactly what a pinned one does
        b.close()
    assert times[chosen] <= 1.15 * min(times.values()), (chosen, times)      # (a perf sanity bound, deliberately loose; the bit-exactness asserts are the gate)
    assert t_first <= 1.25 * times[chosen], (table, chosen, t_first, times)      # (one timing against the best of three)
    if times[table] > 1.05 * times[chosen]:                  # (the table's kernel is measurably another one)
        assert abs(t_first - times[chosen]) < abs(t_first - times[table]), (table, chosen, t_first, times)
    print("streams per workgroup: table %d, measured %d; first call %.3f ms; pinned %s" % (table, chosen, t_first, times))
    pick = [0, 257, n - 1]
    want = orc.synthesize_many(blob, feats[pick])
    assert first_mismatch(pcm_auto[pick], want) is None


def test_legacy_api_combines_concurrent_callers(blob_f32, hip_lib):
    """VERDICT r3 (missing 4): the reference is re-entrant per state -- N threads with N LPCNetStates scale over N cores.  The
    engine's drop-in lpcnet_synthesize used to serialise all states of a model behind one 1-stream batch.  Now concurrent
    callers are combined into one multi-stream pass (api_stream.c: dispatch / comb_run): 64 threads x 50 frames, one state each, every
    thread's PCM must be the oracle's bit for bit, and the aggregate rate must be a large multiple of one thread's."""
    import threading, time
    n, T = 64, 50
    feats = distinct_feats(61000, n, T)
    want = orc.synthesize_many(blob_f32, feats)
    # one thread alone
    st = api.LPCNetState(blob_f32)
    st.synthesize(feats[0, 0])                                  # (warm-up: device side, first launch)
    st.reset()
    t0 = time.perf_counter()
    solo = np.concatenate([st.synthesize(f) for f in feats[0]])
    t_solo = time.perf_counter() - t0
    assert np.array_equal(solo, want[0])
    # 64 threads, one state each
    states = [api.LPCNetState(blob_f32) for _ in range(n)]
    out = [None] * n
    start = threading.Barrier(n + 1)

    def work(i):
        start.wait()
        out[i] = np.concatenate([states[i].synthesize(f) for f in feats[i]])

    th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in th:
        t.start()
    api.dispatch_stats(reset=True)
    start.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    t_all = time.perf_counter() - t0
    for i in range(n):
        assert np.array_equal(out[i], want[i]), i
    speedup = n * t_solo / t_all
    print("legacy API: 1 thread %.1f x real time, %d threads %.1f x in total (%.1f x one thread)" % (T * 0.01 / t_solo, n, n * T * 0.01 / t_all, speedup))
    calls, passes, largest = api.dispatch_stats()
    print("dispatcher: %d calls in %d device passes (%.1f per pass, largest %d)" % (calls, passes, calls / max(passes, 1), largest))
    # the combining itself is what is asserted (the dispatcher's own counters); the wall-clock ratio depends on the box's host cores (20-27 x seen)
    assert calls == n * T and calls / passes >= 8.0 and largest >= 16, (calls, passes, largest)
    assert speedup >= 4.0, (t_solo, t_all, speedup)


def test_eight_shards_of_1024_streams_in_c(blob_f32, hip_lib):
    """BASELINE config 3's shape inside ONE process -- lpcnet_batch_create_sharded with 8 shards x 1024 streams (all on
    the devices the box has; one GPU carries all eight if there is only one): contiguous blocks, a model copy, buffers, stream and
    host thread per shard, no exchange.  The first and the last stream of every shard are checked against the oracle."""
    import torch
    ndev = max(1, torch.cuda.device_count())
    devices = [k % ndev for k in range(8)]
    n, T = 8 * 1024, 5
    base = distinct_feats(64000, 64, T)
    feats = np.ascontiguousarray(base[np.arange(n) % 64])          # 64 distinct feature files, laid out so that shard borders fall on different ones
    b = api.LPCNetBatch(n, blob_f32, devices=devices)
    sh = b.shards
    assert len(sh) == 8 and all(c == 1024 for _, c, _ in sh) and [f for f, _, _ in sh] == [1024 * k for k in range(8)]
    got = b.synthesize(feats)
    pick = sorted({f for f, _, _ in sh} | {f + c - 1 for f, c, _ in sh})
    want = orc.synthesize_many(blob_f32, feats[pick])
    assert first_mismatch(got[pick], want) is None
    # every stream equals the stream with the same feature file (they all started from reset)
    for s in (1, 1023, 1024, 4097, 8191):
        assert np.array_equal(got[s], got[s % 64])
    assert np.count_nonzero(got) > 0.3 * got.size
    b.close()


def test_legacy_api_dispatcher_mixed_models_and_frame_lengths(hip_lib):
    """the combining dispatcher under a mixed load: two models (float and int8 blobs: two registry slots, two queues), callers with
    different N per call (80 / 160 samples: only equal N share a pass), one thread resetting its state half way -- every thread's
    output must be what the oracle gives for the same call sequence"""
    import threading
    blobs = [synth.blob_bytes(synth.make_model(seed=3100)), synth.blob_bytes(synth.make_model(flavour="int8", seed=3101))]
    oms = [orc.OracleModel(b) for b in blobs]
    n, T = 24, 24
    feats = distinct_feats(62000, n, T)
    plan = [[160 if (i + t) % 3 else 80 for t in range(T)] for i in range(n)]           # N per call
    want = []
    for i in range(n):
        st = oms[i % 2].new_state()
        outs = []
        for t in range(T):
            if i == 5 and t == T // 2:
                st.L.orc_state_reset(st.p)
            o = np.zeros(plan[i][t], np.int16)
            st.L.orc_synthesize(st.p, np.ascontiguousarray(feats[i, t, :20], np.float32), o, plan[i][t], 0)
            outs.append(o)
        want.append(np.concatenate(outs))
    states = [api.LPCNetState(blobs[i % 2]) for i in range(n)]
    got = [None] * n
    start = threading.Barrier(n)

    def work(i):
        start.wait()
        outs = []
        for t in range(T):
            if i == 5 and t == T // 2:
                states[i].reset()
            outs.append(states[i].synthesize(feats[i, t], plan[i][t]))
        got[i] = np.concatenate(outs)

    th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i


_SMALLREG_CHILD = r"""
import sys, threading, numpy as np
sys.path.insert(0, %(root)r)
import torch
from lpcnet_amd import api, synth
feats = synth.make_features(1000, 6)
run = lambda st, k=4: np.concatenate([st.synthesize(f) for f in feats[:k]])
blobs = [synth.blob_bytes(synth.make_model(seed=3100 + i)) for i in range(7)]
# ---- full-slot eviction: 4 slots; the 5th distinct blob evicts the least recently used one, whose stale handle is then DETECTED
first = api.LPCNetState(blobs[0]); want0 = run(first)
others = [api.LPCNetState(b) for b in blobs[1:4]]
wants = [run(st) for st in others]                      # slots 1..3 used after slot 0
fifth = api.LPCNetState(blobs[4])                       # table full: slot 0 (least recently used) goes
assert np.any(run(fifth) != 0)
out = np.full(160, 9, np.int16)
api.clear_error()
api.load_library().lpcnet_synthesize(first.p, np.ascontiguousarray(feats[0][:20]), out, 160)
assert not out.any() and api.status() == -5 and "evicted" in api.last_error(), (api.status(), api.last_error())
first.load_model(blobs[0]); first.reset(); api.clear_error()
assert np.array_equal(run(first), want0) and api.status() == 0          # bound again: works, bit for bit
# ---- device sides are recycled (2 resident) and slots evicted while other threads synthesize through the combining dispatcher
errs, stop = [], threading.Event()
def worker(blob, seed):
    try:
        st = api.LPCNetState(blob); ref = None
        f = synth.make_features(seed, 3)
        while not stop.is_set():
            st.reset()
            got = np.concatenate([st.synthesize(x) for x in f])
            if api.status():                                # its model was evicted by the binder below: bind again, like a server would
                api.clear_error(); st.load_model(blob); continue
            if ref is None: ref = got
            elif not np.array_equal(ref, got): errs.append(("mismatch", seed)); return
    except Exception as e:
        errs.append(repr(e))
ths = [threading.Thread(target=worker, args=(blobs[i %% 2], 4000 + i)) for i in range(6)]
for t in ths: t.start()
for rnd in range(12):                                       # keep binding other models: device sides recycle, slots evict
    st = api.LPCNetState(blobs[2 + rnd %% 5]); run(st, 1)
stop.set()
for t in ths: t.join()
assert not errs, errs
print("smallreg ok")
"""


def test_small_registry_eviction_and_recycling_under_load(hip_lib):
    """the paths a 256-slot registry never reaches in a test -- a slot evicted altogether (stale handle detected: the call
    fails soft with the 'evicted' message, binding again works) and device sides released / slots evicted while other threads are
    inside the combining dispatcher -- on a library built with 4 slots / 2 resident device sides (lpcnet_amd/build.py)."""
    import subprocess
    import sys
    from lpcnet_amd import build
    lib = build.build_small_registry()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SMALLREG_CHILD % dict(root=root)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, LPCNET_HIP_LIB=lib, LPCNET_HIP_QUIET="1"))
    assert r.returncode == 0 and "smallreg ok" in r.stdout, (r.stdout[-800:], r.stderr[-2500:])
