"""GPU tests of the packed stage 2 of the two-group sample kernel (lpcnet_amd/csrc/sample_kernel_x2.hip.h, round 9): each stream's chain wave
evaluates the tree's top five levels and publishes its five bits under the sample's sequence number; ONE row wave evaluates the last three levels
of the group's four streams in one pass (lane 16 f + l = local lane l of stream f) and hands the leader 8 bits per stream.  Every case is compared
with the plain-C oracle bit for bit: PCM, GRU states, LPC history, last excitation, de-emphasis memory, frame count and RNG words.

Every case is one GPU step: a child process of its own under its own time limit.  A child that ends on a signal or runs into its limit marks the
module: the cases behind it fail without starting anything on the GPU, and nothing is run a second time."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- the cases (run in the child)
def _feats_for(seeds, T):
    from lpcnet_amd import synth
    return np.stack([synth.make_features(s, T) for s in seeds])


def _check_states(b, states, which):
    for s in which:
        st = b.get_state(s)
        c1, c2, ga, gb = states[s].nnet_state()
        ls, le, dm, fc, rng = states[s].signal_state()
        assert np.array_equal(np.array(st.gru_a, np.float32), ga) and np.array_equal(np.array(st.gru_b, np.float32), gb), s
        assert np.array_equal(np.array(st.conv1_mem, np.float32), c1) and np.array_equal(np.array(st.conv2_mem, np.float32), c2), s
        assert np.array_equal(np.array(st.last_sig, np.float32), ls) and st.last_exc == le and st.frame_count == fc, s
        assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s


def _setup(n):
    from lpcnet_amd import api, synth
    from oracle import orc
    blob = synth.blob_bytes(synth.make_model(flavour="float"))
    om = orc.OracleModel(blob)
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = 8
    assert b.streams_per_workgroup == 8
    return b, om, [om.new_state() for _ in range(n)]


def case_streams(n):
    """8 / 16 / 13 / 5 / 1 streams: full, partial and empty fields in both groups (the fields of absent streams belong to clamped copies); the first
    two frames of a fresh stream are start-up frames (the tree runs, its value is ignored); a second call continues from the state written back --
    the sequence numbers of a launch start over, the prefix cells are cleared"""
    n = int(n)
    T1, T2 = 6, 3
    f1, f2 = _feats_for(range(9100, 9100 + n), T1), _feats_for(range(9200, 9200 + n), T2)
    b, om, sts = _setup(n)
    got = b.synthesize(f1)
    assert np.array_equal(got, np.stack([sts[s].synthesize(f1[s]) for s in range(n)]))
    assert np.all(got[:, :320] == 0) and np.any(got[:, 320:] != 0)
    _check_states(b, sts, range(n))
    got2 = b.synthesize(f2)
    assert np.array_equal(got2, np.stack([sts[s].synthesize(f2[s]) for s in range(n)]))
    _check_states(b, sts, range(n))
    b.close()


def case_partial_resets():
    """streams of one group, and all of the other group, start over while their neighbours go on: live and start-up streams side by side in the
    fields of one pass"""
    n, T = 13, 5
    feats = _feats_for(range(9300, 9300 + n), T)
    b, om, sts = _setup(n)
    assert np.array_equal(b.synthesize(feats), np.stack([sts[s].synthesize(feats[s]) for s in range(n)]))
    b.reset(1, 2)                                           # streams 1, 2 of group 0
    b.reset(4, 4)                                           # all of group 1
    b.reset(10, 1)                                          # one stream of the second workgroup's group 0
    for s in (1, 2, 4, 5, 6, 7, 10):
        sts[s] = om.new_state()
    assert np.array_equal(b.synthesize(feats), np.stack([sts[s].synthesize(feats[s]) for s in range(n)]))
    _check_states(b, sts, range(n))
    b.close()


def case_frame_length(N):
    """N samples per frame through the per-stream step call; N = 1: every sample is a frame boundary"""
    N = int(N)
    n, T = 9, 6
    feats = _feats_for(range(9400, 9400 + n), T)
    b, om, sts = _setup(n)
    for t in range(T):
        pcm = np.zeros((n, 160), np.int16)
        got = b.synthesize_step(np.ascontiguousarray(feats[:, t]), pcm, [N] * n, [0] * n, [1] * n)
        for s in range(n):
            ref = np.zeros(160, np.int16)
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), ref, N, 0)
            assert np.array_equal(got[s, :N], ref[:N]), (t, s)
    _check_states(b, sts, range(n))
    b.close()


def case_teacher_forcing(preload):
    """src/lpcnet.c:256-259: the first `preload` samples of a frame come from the caller; the tree of those samples runs and is not used"""
    preload = int(preload)
    n, T = 9, 8
    feats = _feats_for(range(9500, 9500 + n), T)
    forced = (np.random.RandomState(95).randn(n, T * 160) * 900).astype(np.int16)
    b, om, sts = _setup(n)
    want = np.zeros((n, T * 160), np.int16)
    for s in range(n):
        for t in range(T):
            frame = forced[s, t * 160:(t + 1) * 160].copy()
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), frame, 160, preload)
            want[s, t * 160:(t + 1) * 160] = frame
    got = b.synthesize(feats, preload_pcm=forced, preload=preload)
    assert np.array_equal(got, want)
    _check_states(b, sts, range(n))
    b.close()


def case_long_run():
    """100 frames x 16 streams (two workgroups: every field of both groups carries a stream), one frame per call, the last excitation compared after
    every call and the complete state after every tenth.  The excitations at the frame ends are the oracle's, which the engine's must equal; PER FIELD
    (stream s sits in field s % 4) they take both branches at every level of the tree."""
    n, T = 16, 100
    feats = _feats_for(range(9600, 9600 + n), T)
    b, om, sts = _setup(n)
    excs = [[] for _ in range(4)]
    for t in range(T):
        f = np.ascontiguousarray(feats[:, t:t + 1])
        got = b.synthesize(f)
        assert np.array_equal(got, np.stack([sts[s].synthesize(f[s]) for s in range(n)])), t
        for s in range(n):
            le = sts[s].signal_state()[1]
            assert b.get_state(s).last_exc == le, (t, s)
            if t >= 2:
                excs[s % 4].append(le)
        if t % 10 == 9:
            _check_states(b, sts, range(n))
    for field in range(4):
        e = np.asarray(excs[field])
        cover = [(bool(np.any(((e >> (7 - lv)) & 1) == 0)), bool(np.any(((e >> (7 - lv)) & 1) == 1))) for lv in range(8)]
        assert all(lo and hi for lo, hi in cover), (field, cover)
    b.close()


# ---------------------------------------------------------------------------------------------------------- the parent: one child per step
_faulted = []      # the first step that ended on a signal or a time limit


def run_step(case, arg=None, limit=300):
    assert not _faulted, "not started: GPU step %s ended abnormally before this one" % _faulted[0]
    cmd = [sys.executable, os.path.abspath(__file__), case] + ([str(arg)] if arg is not None else [])
    try:
        r = subprocess.run(cmd, cwd=ROOT, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _faulted.append("%s %s (time limit of %d s)" % (case, arg, limit))
        pytest.fail("GPU step ran into its time limit: %s\n%s" % (_faulted[0], e.stdout or ""))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _faulted.append("%s %s (exit status %d)" % (case, arg, r.returncode))
    assert r.returncode == 0, "exit status %d\n%s" % (r.returncode, r.stdout[-4000:])


@pytest.mark.parametrize("n", [8, 16, 13, 5, 1])
def test_stream_counts_with_start_up_frames_and_a_continued_call(n, hip_lib):
    run_step("streams", n)


def test_partial_resets(hip_lib):
    run_step("partial_resets")


@pytest.mark.parametrize("N", [160, 40, 1])
def test_frame_lengths(N, hip_lib):
    run_step("frame_length", N)


@pytest.mark.parametrize("preload", [160, 40])
def test_teacher_forced_samples_ignore_the_walked_value(preload, hip_lib):
    run_step("teacher_forcing", preload)


def test_long_run_reaches_both_halves_of_every_tree_level_in_every_field(hip_lib):
    run_step("long_run", limit=600)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("ok")
