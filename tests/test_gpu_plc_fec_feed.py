"""The batched FEC feed (lpcnet_batch_plc_fec_feed*: every stream's lpcnet_plc_fec_clear / lpcnet_plc_fec_add traffic in one call and one launch)
against the per-stream calls it replaces and against the reference (tests/golden/golden_plc_fec_v1.npz, made by tests/tools/make_golden_plc_fec.py
from the reference's generic-C builds driven stream by stream).  One 60-step script of five streams (tests/tools/plc_fec_script.py); all
comparisons on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_fec_script as fs  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

N, T = fs.N, fs.T
FILL, KEEP, READ, SKIP = 4, 5, 6, 7          # columns of lpcn_plc_ctl, the first 9 ints of a stream's PLC state record


@pytest.fixture(scope="module")
def sc():
    return fs.script()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_fec_v1.npz"))


@pytest.fixture(scope="module")
def blobs(gold):
    b = [synth.blob_bytes(plc_synth.make_model_with_plc()), synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))]
    assert [zlib.crc32(x) for x in b] == gold["blob_crc"].tolist()
    return b


def frame_of(sc, t, streams=slice(None)):
    lost = np.ascontiguousarray(sc["lost"][t, streams])
    frame = np.ascontiguousarray(sc["pcm"][streams, t])
    frame[lost != 0] = 0
    return frame, lost


def ctl_of(b, s):
    return np.frombuffer(b.get_plc_state(s)[:36], np.int32)


def run_feed(b, sc):
    """the script through one plc_fec_feed per step -> PCM [N][T][160], dropped [T][N], every stream's state at the end"""
    out = np.zeros((N, T, 160), np.int16)
    dropped = np.zeros((T, N), np.int32)
    for t in range(T):
        r0, r1 = fs.step_rows(sc, t)
        dropped[t] = b.plc_fec_feed(sc["vec"][r0:r1], sc["count"][t], sc["skip"][t], sc["clear"][t])
        out[:, t] = b.plc_step(*frame_of(sc, t))
    return out, dropped, [b.get_plc_state(s) for s in range(N)]


def run_per_stream(b, sc):
    """the same script through plc_fec_clear / plc_fec_add, stream by stream -> PCM, the 1-returns per step and stream, the states"""
    out = np.zeros((N, T, 160), np.int16)
    full = np.zeros((T, N), np.int32)
    for t in range(T):
        row = fs.step_rows(sc, t)[0]
        for s in range(N):
            if sc["clear"][t, s]:
                b.plc_fec_clear(s)
            for _ in range(int(sc["skip"][t, s])):
                assert b.plc_fec_add(s, None) == 0
            for _ in range(int(sc["count"][t, s])):
                full[t, s] += b.plc_fec_add(s, sc["vec"][row])
                row += 1
        out[:, t] = b.plc_step(*frame_of(sc, t))
    return out, full, [b.get_plc_state(s) for s in range(N)]


@pytest.fixture(scope="module")
def host_form(sc, blobs, hip_lib):
    """the host-form run of the script per (options, int8), made once and shared"""
    made = {}

    def get(options, i8=0):
        if (options, i8) not in made:
            b = api.LPCNetBatch(N, blobs[i8])
            b.plc_enable(options)
            made[(options, i8)] = run_feed(b, sc)
            b.close()
        return made[(options, i8)]
    return get


def planned(sc, options):
    """the script through the two host planners alone -> per step the feed's records and dropped counts and the ring positions before it; the final ctl"""
    ctl = np.zeros((N, 9), np.int32)
    ctl[:, 0] = 400
    steps = []
    for t in range(T):
        before = ctl.copy()
        rec, dropped = api.plc_fec_feed_plan(ctl, sc["count"][t], sc["skip"][t], sc["clear"][t])
        steps.append((before, rec, dropped))
        api.plc_plan(options, ctl, sc["lost"][t])
    return steps, ctl


def assert_script_reaches_every_case(sc, steps):
    seen = dict(count0_beside_fed=False, three_at_once=False, skips=False, clear_then_vectors=False, compaction_mid_list=False, full_ring_keep0_drops=False)
    fed = np.zeros(N, np.int64)
    for t, (before, rec, dropped) in enumerate(steps):
        count, skip, clear = sc["count"][t], sc["skip"][t], sc["clear"][t]
        fed += count
        by_stream = {int(r[0]): r for r in rec}
        seen["count0_beside_fed"] |= bool((count == 0).any() and len(rec) > 0 and not set(np.flatnonzero(count == 0)) & set(by_stream))
        seen["skips"] |= bool((skip > 0).any())
        for s, r in by_stream.items():
            seen["three_at_once"] |= bool(count[s] == 3 and r[2] + r[6] == 3)
            seen["clear_then_vectors"] |= bool(clear[s] and before[s, FILL] > 0 and r[3] == 0 and r[2] == count[s])
            seen["compaction_mid_list"] |= bool(before[s, FILL] == 98 and before[s, KEEP] > 0 and count[s] == 5 and tuple(r[2:]) == (2, 98, before[s, KEEP], 100 - before[s, KEEP], 3, 100 - before[s, KEEP]))
        for s in np.flatnonzero(dropped):
            seen["full_ring_keep0_drops"] |= bool(before[s, KEEP] == 0 and not clear[s] and fed[s] > 100 and not sc["lost"][:t + 1, s].any())
    assert all(seen.values()), seen


@pytest.mark.parametrize("options", [api.PLC_CODEC, api.PLC_CAUSAL | api.PLC_DC_FILTER])
def test_one_feed_per_step_equals_the_per_stream_calls(options, sc, blobs, host_form):
    steps, ctl = planned(sc, options)
    assert_script_reaches_every_case(sc, steps)
    b = api.LPCNetBatch(N, blobs[0])
    b.plc_enable(options)
    want, full, want_state = run_per_stream(b, sc)
    b.close()
    got, dropped, got_state = host_form(options)
    for t in range(T):
        assert np.array_equal(got[:, t], want[:, t]), (t, np.argwhere(got[:, t] != want[:, t])[:4].tolist())
    assert np.array_equal(dropped, full) and dropped.sum() > 20
    assert np.array_equal(dropped, np.stack([s[2] for s in steps]))
    for s in range(N):
        assert got_state[s] == want_state[s], s
        assert np.array_equal(np.frombuffer(got_state[s][:36], np.int32), ctl[s]), s
    lost = sc["lost"].T.astype(bool)
    assert (got[lost] != 0).mean() > 0.5                  # the concealment is not silence


@pytest.mark.parametrize("case", range(3))
def test_feed_equals_the_reference(case, gold, sc, host_form):
    for k in ("lost", "count", "skip", "clear", "vec"):
        assert np.array_equal(gold[k], sc[k]), k          # the fixture was made from this script
    assert np.array_equal(gold["pcm_in"], sc["pcm"])
    options, i8 = (int(x) for x in gold["cases"][case])
    got = host_form(options, i8)[0]
    bad = np.argwhere(got != gold["pcm_out"][case])
    assert bad.size == 0, "options %d int8 %d: first differing (stream, frame, sample) %s of %d" % (options, i8, bad[:4].tolist(), len(bad))


def test_device_form_on_a_caller_stream_and_capture_refusal(sc, blobs, host_form):
    import torch
    dev = torch.device("cuda:0")
    want, want_dropped, want_state = host_form(api.PLC_CODEC)
    b = api.LPCNetBatch(N, blobs[0])
    b.plc_enable(api.PLC_CODEC)
    b.tune()
    vec = torch.from_numpy(sc["vec"]).to(dev)
    d = torch.zeros((N, 160), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    out = np.zeros((N, T, 160), np.int16)
    dropped = np.zeros((T, N), np.int32)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for t in range(T):
            frame, lost = frame_of(sc, t)
            d.copy_(torch.from_numpy(frame))
            r0 = fs.step_rows(sc, t)[0]
            dropped[t] = b.plc_fec_feed_device(vec.data_ptr() + r0 * 80, sc["count"][t], sc["skip"][t], sc["clear"][t], hip_stream=s.cuda_stream)
            b.plc_step_device(d.data_ptr(), lost, s.cuda_stream)          # (nothing waits between the feed and the step)
            out[:, t] = d.cpu().numpy()
    assert np.array_equal(out, want) and np.array_equal(dropped, want_dropped)
    assert [b.get_plc_state(i) for i in range(N)] == want_state
    before = [b.get_plc_state(i) for i in range(N)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.plc_fec_feed_device(vec.data_ptr(), [1] * N, hip_stream=cs)
        d.add_(0)                                         # (the capture stays usable and is not empty)
    b.sync()
    assert [b.get_plc_state(i) for i in range(N)] == before
    b.close()


def test_two_unequal_shards_equal_the_unsharded_batch(sc, blobs, host_form):
    import torch
    want, want_dropped, want_state = host_form(api.PLC_CODEC)
    b = api.LPCNetBatch(N, blobs[0], devices=[0, 0])
    assert [x[:2] for x in b.shards] == [(0, 3), (3, 2)]
    b.plc_enable(api.PLC_CODEC)
    got, dropped, state = run_feed(b, sc)
    b.close()
    assert np.array_equal(got, want) and np.array_equal(dropped, want_dropped) and state == want_state
    # the device form shard by shard: each shard's streams alone, in arrays and in packing
    b = api.LPCNetBatch(N, blobs[0], devices=[0, 0])
    b.plc_enable(api.PLC_CODEC)
    b.tune()
    dev = torch.device("cuda:0")
    vec = torch.from_numpy(sc["vec"]).to(dev)
    d = torch.zeros((N, 160), dtype=torch.int16, device=dev)
    out = np.zeros((N, T, 160), np.int16)
    dropped = np.zeros((T, N), np.int32)
    torch.cuda.synchronize()
    for t in range(T):
        frame, lost = frame_of(sc, t)
        d.copy_(torch.from_numpy(frame))
        torch.cuda.synchronize()
        for k, (first, cnt, _) in enumerate(b.shards):
            sl = slice(first, first + cnt)
            r0 = fs.step_rows(sc, t)[0] + int(sc["count"][t, :first].sum())
            dropped[t, sl] = b.plc_fec_feed_device(vec.data_ptr() + r0 * 80, sc["count"][t, sl], sc["skip"][t, sl], sc["clear"][t, sl], shard=k)
            b.plc_step_device(d[sl].data_ptr(), lost[sl], shard=k)
        b.sync()
        out[:, t] = d.cpu().numpy()
    assert np.array_equal(out, want) and np.array_equal(dropped, want_dropped)
    with pytest.raises(api.LPCNetError, match=r"\(-4\).*shard"):
        b.plc_fec_feed_device(vec.data_ptr(), [1] * N)
    b.close()


def test_errors_leave_the_rings_alone(sc, blobs, hip_lib):
    import torch
    one = np.zeros((1, 20), np.float32)
    b = api.LPCNetBatch(2, blobs[0])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.plc_fec_feed(one, [1, 0])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.plc_fec_feed_device(0, [0, 0])
    b.plc_enable(api.PLC_CODEC)
    assert not b.plc_fec_feed(sc["vec"][:3], [2, 1], [0, 4]).any()
    assert ctl_of(b, 0)[[FILL, SKIP]].tolist() == [2, 0] and ctl_of(b, 1)[[FILL, SKIP]].tolist() == [1, 4]
    before = [b.get_plc_state(i) for i in range(2)]
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.plc_fec_feed(one, [1, -1], [3, 3], [1, 1])
    d = torch.zeros((4, 20), dtype=torch.float32, device="cuda:0")
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.plc_fec_feed_device(d.data_ptr(), [1, -1], [3, 3], [1, 1])
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.plc_fec_feed_device(0, [1, 0])                  # vectors without a source
    assert [b.get_plc_state(i) for i in range(2)] == before
    # a feed without vectors is skips and clears alone; a list of per-stream arrays is packed for the caller
    assert not b.plc_fec_feed(np.zeros((0, 20), np.float32), [0, 0], [1, 0], [0, 1]).any()
    assert ctl_of(b, 0)[[FILL, SKIP]].tolist() == [2, 1] and ctl_of(b, 1)[[FILL, SKIP]].tolist() == [0, 0]
    assert not b.plc_fec_feed([sc["vec"][3:4], sc["vec"][4:6]], [1, 2]).any()
    assert b.get_plc_state(1).find(sc["vec"][4:6].tobytes()) > 0 and ctl_of(b, 1)[FILL] == 2
    b.close()
    b = api.LPCNetBatch(N, blobs[0], devices=[0, 0])
    b.plc_enable(api.PLC_CODEC)
    before = [b.get_plc_state(i) for i in range(N)]
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.plc_fec_feed(sc["vec"][:4], [1, 1, 1, 1, -1])    # refused for the whole batch before the first shard's rings change
    assert [b.get_plc_state(i) for i in range(N)] == before
    b.close()
