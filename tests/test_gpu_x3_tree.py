"""GPU tests of the two-stage sampling tree on the twelve-wave form of the two-group sample kernel (lpcnet_amd/csrc/sample_kernel_x3.hip.h; round 13):
stage 1 on each stream's chain wave behind GRU-B's gates, stage 2 as one packed pass of wave LPCN_X3_S2W behind its P1 segments.  Forced through
the C ABI (twelve_waves = 1, eight streams per workgroup) and compared with the plain-C oracle bit for bit -- PCM, GRU states, conv memories, LPC
history, last excitation, de-emphasis memory, frame count and RNG words -- and with the eight-wave form on the same inputs (PCM and the complete
state record).  What the cases are after:

  * 13, 5 and 1 streams: groups with fewer than four streams, whose unused stage-2 fields evaluate clamped copies;
  * a continued second call: the prefix cells are cleared at launch and the sequence numbers restart;
  * 1 and 40 samples per call: stage 2's poll and lead sit at the end of a P1 that a launch of one sample runs once per group;
  * a reset of one stream inside a group between two calls.

The packer offers forced dealings (LPCN_DEAL_FORCE_X2, tests/test_gpu_x2_slots.py) for the eight-wave image only, so there is no case that moves
every P1 item off the stage-2 wave of the twelve-wave image.  The oracle runs once per module; no test changes what it returned."""
import numpy as np
import pytest

from lpcnet_amd import api, synth
from oracle import orc

pytestmark = pytest.mark.gpu

NMAX, T1, T2 = 13, 3, 2


def batch(n, blob, twelve):
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = 8
    b.twelve_waves = twelve
    assert b.streams_per_workgroup == 8 and b.twelve_waves == twelve
    return b


def snapshot(st):
    return st.nnet_state() + st.signal_state()


def check_state(b, s, snap):
    c1, c2, ga, gb, ls, le, dm, fc, rng = snap
    st = b.get_state(s)
    assert np.array_equal(np.array(st.gru_a, np.float32), ga) and np.array_equal(np.array(st.gru_b, np.float32), gb), s
    assert np.array_equal(np.array(st.conv1_mem, np.float32), c1) and np.array_equal(np.array(st.conv2_mem, np.float32), c2), s
    assert np.array_equal(np.array(st.last_sig, np.float32), ls) and st.last_exc == le and st.frame_count == fc, s
    assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s


def same_records(b12, b8, n):
    for s in range(n):
        assert bytes(b12.get_state(s)) == bytes(b8.get_state(s)), s      # the complete record, RNG included


@pytest.fixture(scope="module")
def ref(blob_f32):
    """13 streams through the oracle: a call of 3 frames, then either a continued call of 2 frames or the same 2 frames from a fresh state"""
    om = orc.OracleModel(blob_f32)
    f1 = np.stack([synth.make_features(8300 + s, T1) for s in range(NMAX)])
    f2 = np.stack([synth.make_features(8400 + s, T2) for s in range(NMAX)])
    pcm1, snap1, pcm2, snap2, pcm2_fresh, snap2_fresh = [], [], [], [], [], []
    for s in range(NMAX):
        st = om.new_state()
        pcm1.append(st.synthesize(f1[s])); snap1.append(snapshot(st))
        pcm2.append(st.synthesize(f2[s])); snap2.append(snapshot(st))
        st = om.new_state()
        pcm2_fresh.append(st.synthesize(f2[s])); snap2_fresh.append(snapshot(st))
    out = dict(f1=f1, f2=f2, pcm1=np.stack(pcm1), pcm2=np.stack(pcm2), pcm2_fresh=np.stack(pcm2_fresh))
    for a in out.values():
        a.setflags(write=False)
    out.update(snap1=snap1, snap2=snap2, snap2_fresh=snap2_fresh)
    return out


@pytest.mark.parametrize("n", [8, 13, 5, 1])
def test_stream_counts_and_a_continued_call(n, ref, blob_f32, hip_lib):
    b12, b8 = batch(n, blob_f32, 1), batch(n, blob_f32, 0)
    for feats, pcm, snaps in ((ref["f1"], ref["pcm1"], ref["snap1"]), (ref["f2"], ref["pcm2"], ref["snap2"])):
        f = np.ascontiguousarray(feats[:n])
        got = b12.synthesize(f)
        assert np.array_equal(got, pcm[:n])
        for s in range(n):
            check_state(b12, s, snaps[s])
        assert np.array_equal(b8.synthesize(f), got)
        same_records(b12, b8, n)
    assert np.any(got != 0)                                  # (the continued call is past the start-up frames)
    b12.close(); b8.close()


@pytest.mark.parametrize("N", [1, 40])
def test_n_samples_per_call(N, ref, blob_f32, hip_lib):
    n, T = 13, 4
    feats = np.concatenate([ref["f1"], ref["f2"]], axis=1)[:n, :T]
    om = orc.OracleModel(blob_f32)
    sts = [om.new_state() for _ in range(n)]
    b12, b8 = batch(n, blob_f32, 1), batch(n, blob_f32, 0)
    for t in range(T):
        f = np.ascontiguousarray(feats[:, t])
        zero = np.zeros((n, 160), np.int16)
        got = b12.synthesize_step(f, zero, [N] * n, [0] * n, [1] * n)
        for s in range(n):
            want = np.zeros(160, np.int16)
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), want, N, 0)
            assert np.array_equal(got[s, :N], want[:N]), (t, s)
        assert np.array_equal(b8.synthesize_step(f, zero, [N] * n, [0] * n, [1] * n), got)
    for s in range(n):
        check_state(b12, s, snapshot(sts[s]))
    same_records(b12, b8, n)
    b12.close(); b8.close()


def test_reset_of_one_stream_inside_a_group_between_calls(ref, blob_f32, hip_lib):
    n, gone = 8, 5                                           # stream 1 of group 1
    b12, b8 = batch(n, blob_f32, 1), batch(n, blob_f32, 0)
    f1, f2 = np.ascontiguousarray(ref["f1"][:n]), np.ascontiguousarray(ref["f2"][:n])
    assert np.array_equal(b12.synthesize(f1), ref["pcm1"][:n])
    assert np.array_equal(b8.synthesize(f1), ref["pcm1"][:n])
    b12.reset(gone, 1); b8.reset(gone, 1)
    got = b12.synthesize(f2)
    for s in range(n):
        assert np.array_equal(got[s], (ref["pcm2_fresh"] if s == gone else ref["pcm2"])[s]), s
        check_state(b12, s, (ref["snap2_fresh"] if s == gone else ref["snap2"])[s])
    assert np.array_equal(b8.synthesize(f2), got)
    same_records(b12, b8, n)
    b12.close(); b8.close()
