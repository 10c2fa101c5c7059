"""GPU tests of the two-stage tree of the two-group sample kernel (lpcnet_amd/csrc/sample_kernel_x2.hip.h, tree_stages.h): each stream's chain wave
evaluates the tree's top five levels, walks them, evaluates the 7-node subtree under the node reached and hands the leader 8 bits.  Every case is
compared with the plain-C oracle bit for bit: PCM, GRU states, LPC history, last excitation, de-emphasis memory, frame count and RNG words."""
import numpy as np
import pytest

from lpcnet_amd import api, synth
from oracle import orc

pytestmark = pytest.mark.gpu


def feats_for(seeds, T):
    return np.stack([synth.make_features(s, T) for s in seeds])


def check_states(b, states, which):
    for s in which:
        st = b.get_state(s)
        c1, c2, ga, gb = states[s].nnet_state()
        ls, le, dm, fc, rng = states[s].signal_state()
        assert np.array_equal(np.array(st.gru_a, np.float32), ga) and np.array_equal(np.array(st.gru_b, np.float32), gb), s
        assert np.array_equal(np.array(st.conv1_mem, np.float32), c1) and np.array_equal(np.array(st.conv2_mem, np.float32), c2), s
        assert np.array_equal(np.array(st.last_sig, np.float32), ls) and st.last_exc == le and st.frame_count == fc, s
        assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s


def batch8(n, blob):
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = 8
    assert b.streams_per_workgroup == 8
    return b


@pytest.mark.parametrize("n", [8, 13, 5, 1])
def test_stream_counts_with_start_up_frames_and_a_continued_call(n, blob_f32, hip_lib):
    """full workgroup, partial second group, partial first group, one stream (the other seven lanes-of-streams are clamped copies); the first two
    frames of a fresh stream are start-up frames (not live: the tree runs, its value is ignored); a second call continues from the state written back"""
    T1, T2 = 6, 3
    f1, f2 = feats_for(range(8100, 8100 + n), T1), feats_for(range(8200, 8200 + n), T2)
    om = orc.OracleModel(blob_f32)
    sts = [om.new_state() for _ in range(n)]
    b = batch8(n, blob_f32)
    got = b.synthesize(f1)
    want = np.stack([sts[s].synthesize(f1[s]) for s in range(n)])
    assert np.array_equal(got, want)
    assert np.all(got[:, :320] == 0) and np.any(got[:, 320:] != 0)
    check_states(b, sts, range(n))
    got2 = b.synthesize(f2)
    want2 = np.stack([sts[s].synthesize(f2[s]) for s in range(n)])
    assert np.array_equal(got2, want2)
    check_states(b, sts, range(n))
    b.close()


@pytest.mark.parametrize("preload", [160, 40])
def test_teacher_forced_samples_ignore_the_walked_value(preload, blob_f32, hip_lib):
    """src/lpcnet.c:256-259: the first `preload` samples of a frame come from the caller; the tree of those samples runs and is not used"""
    n, T = 9, 8
    feats = feats_for(range(8300, 8300 + n), T)
    rng = np.random.RandomState(83)
    forced = (rng.randn(n, T * 160) * 900).astype(np.int16)
    om = orc.OracleModel(blob_f32)
    sts = [om.new_state() for _ in range(n)]
    want = np.zeros((n, T * 160), np.int16)
    for s in range(n):
        for t in range(T):
            frame = forced[s, t * 160:(t + 1) * 160].copy()
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), frame, 160, preload)
            want[s, t * 160:(t + 1) * 160] = frame
    b = batch8(n, blob_f32)
    got = b.synthesize(feats, preload_pcm=forced, preload=preload)
    assert np.array_equal(got, want)
    check_states(b, sts, range(n))
    b.close()


@pytest.mark.parametrize("N", [160, 40, 1])
def test_frame_lengths(N, blob_f32, hip_lib):
    """N samples per frame through the per-stream step call; N = 1: every sample is a frame boundary"""
    n, T = 9, 6
    feats = feats_for(range(8400, 8400 + n), T)
    om = orc.OracleModel(blob_f32)
    sts = [om.new_state() for _ in range(n)]
    b = batch8(n, blob_f32)
    for t in range(T):
        pcm = np.zeros((n, 160), np.int16)
        got = b.synthesize_step(np.ascontiguousarray(feats[:, t]), pcm, [N] * n, [0] * n, [1] * n)
        for s in range(n):
            ref = np.zeros(160, np.int16)
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), ref, N, 0)
            assert np.array_equal(got[s, :N], ref[:N]), (t, s)
    check_states(b, sts, range(n))
    b.close()


LONG_SEEDS, LONG_FRAMES = range(8500, 8516), 100


def level_coverage(excs):
    """per tree level (decision 0 = the highest bit of the excitation index): whether both halves were taken"""
    e = np.asarray(excs)
    return [(bool(np.any(((e >> (7 - lv)) & 1) == 0)), bool(np.any(((e >> (7 - lv)) & 1) == 1))) for lv in range(8)]


def test_long_run_reaches_both_halves_of_every_tree_level(blob_f32, hip_lib):
    """100 frames x 16 streams, one frame per call, the complete state compared after every tenth call and the last excitation after every call.  The
    excitations sampled at the frame ends (1568 of them, the oracle's values, which the engine's must equal) take both branches at every level of the
    tree, so each of the five bits that select the stage-2 subtree is exercised with both values.  (With these seeds on the synthetic model they fall
    into the four subtrees around the mu-law zero, 14..17 of 32; the extreme amplitudes are not reached.)"""
    n = len(LONG_SEEDS)
    feats = feats_for(LONG_SEEDS, LONG_FRAMES)
    om = orc.OracleModel(blob_f32)
    sts = [om.new_state() for _ in range(n)]
    b = batch8(n, blob_f32)
    excs = []
    for t in range(LONG_FRAMES):
        f = np.ascontiguousarray(feats[:, t:t + 1])
        got = b.synthesize(f)
        want = np.stack([sts[s].synthesize(f[s]) for s in range(n)])
        assert np.array_equal(got, want), t
        for s in range(n):
            le = sts[s].signal_state()[1]
            assert b.get_state(s).last_exc == le, (t, s)
            if t >= 2:
                excs.append(le)
        if t % 10 == 9:
            check_states(b, sts, range(n))
    assert all(lo and hi for lo, hi in level_coverage(excs)), level_coverage(excs)
    b.close()
