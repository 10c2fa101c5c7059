"""GPU tests of the two-group sample kernel's STREAMED variants (lpcnet_amd/csrc/sample_kernel_x2.hip.h, sample_x2w.hip): models of more than 32
GRU-A items per lane -- heavy-tailed, trained-like sparsity -- at eight streams per workgroup, behind a batch's opt-in switch
(LPCNetBatch.two_group_streaming, lpcnet_batch_set_two_group_streaming).  24 items of a lane stay in registers, the others are fetched from L2 every
sample with their block indices; the arithmetic is the four-stream kernel's, so every comparison is bit for bit, against the plain-C oracle.

A. four models on their own dealing: densities 0.07 / 0.07 / 0.25 (36 items per lane: the smallest variant, 48), skew 0.05 (46), skew 0.1 (65:
   variant 80, a chain wave of 40 items, heads that are streamed from their first item), skew 0.4 (96: the largest variant, a chain wave of 95
   items, a row wave whose P1 has no item and whose head has two).  13 streams (one full workgroup and one of 4 + 1), 4 frames and a continued call
   of 2: PCM, GRU-A / B states, LPC history, last excitation, de-emphasis memory, frame count and RNG words of every stream.
B. skew 0.1: frames of 1 / 7 / 159 samples, teacher forcing with 0 / 80 / 160 imposed samples, a partial reset of streams 2..5 (both groups of a
   workgroup) between calls, and a 9-stream PLC sequence whose groups launch at eight, against the same sequence with the switch off.
C. the switch: off by default (a pinned eight is refused), refused for int8 blobs and a block-sparse GRU-B matrix, a no-op on a model that has the
   ordinary image, FAST under a pinned eight runs at four, no twelve-wave form, no switching off under a pinned eight.

Every case is one GPU step: a child process of its own under its own time limit.  A child that ends on a signal or runs into its limit marks the
module: the cases behind it fail without starting anything on the GPU, and nothing is run a second time."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEW = dict(skew=0.1)
MODELS = {
    "densities_36_items": dict(densities=(0.07, 0.07, 0.25)),
    "skew005_46_items": dict(skew=0.05),
    "skew01_65_items": SKEW,
    "skew04_96_items": dict(skew=0.4),
}

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- the cases (run in the child)
def wide_batch(n, blob):
    """a batch with the switch on and eight streams per workgroup pinned"""
    from lpcnet_amd import api
    b = api.LPCNetBatch(n, blob)
    assert b.two_group_streaming is False
    b.two_group_streaming = True
    assert b.two_group_streaming is True
    b.streams_per_workgroup = 8
    assert b.streams_per_workgroup == 8
    return b


def check_states(b, sts):
    for s, ost in enumerate(sts):
        st = b.get_state(s)
        c1, c2, ga, gb = ost.nnet_state()
        ls, le, dm, fc, rng = ost.signal_state()
        assert np.array_equal(np.array(st.gru_a, np.float32), ga) and np.array_equal(np.array(st.gru_b, np.float32), gb), s
        assert np.array_equal(np.array(st.last_sig, np.float32), ls) and st.last_exc == le and st.frame_count == fc, s
        assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s


def case_parity(model_kw):
    from lpcnet_amd import api, synth
    from oracle import orc
    n = 13
    blob = synth.blob_bytes(synth.make_model(**model_kw))
    info = api.x2_wide_info(blob)
    assert info["fits"] == 1 and info["selftest"] == 0
    om = orc.OracleModel(blob)
    sts = [om.new_state() for _ in range(n)]
    b = wide_batch(n, blob)
    for seed, T in ((9700, 4), (9800, 2)):
        feats = np.stack([synth.make_features(seed + s, T) for s in range(n)])
        got = b.synthesize(feats)
        want = np.stack([sts[s].synthesize(feats[s]) for s in range(n)])
        bad = np.argwhere(got != want)
        assert bad.size == 0, "first differing (stream, sample) %s of %d" % (bad[:4].tolist(), len(bad))
        check_states(b, sts)
        assert b.streams_per_workgroup == 8
    assert np.any(got != 0)                                  # (the continued call is past the start-up frames)
    b.close()


def case_short_frames(N):
    """lpcnet_synthesize(st, features, out, N) for every stream (the per-stream step call with equal arguments: one group, one launch)"""
    from lpcnet_amd import synth
    from oracle import orc
    n, T = 9, 5
    blob = synth.blob_bytes(synth.make_model(**SKEW))
    om = orc.OracleModel(blob)
    sts = [om.new_state() for _ in range(n)]
    b = wide_batch(n, blob)
    feats = np.stack([synth.make_features(5300 + s, T) for s in range(n)])
    nonzero = False
    for t in range(T):
        got = b.synthesize_step(np.ascontiguousarray(feats[:, t]), np.zeros((n, 160), np.int16), [N] * n, [0] * n, [1] * n)
        assert b.last_groups()[:, 6].tolist() == [8]
        for s in range(n):
            ref = np.zeros(160, np.int16)
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), ref, N, 0)
            assert np.array_equal(got[s, :N], ref[:N]), (t, s)
        nonzero = nonzero or bool(np.any(got != 0))
    check_states(b, sts)
    assert nonzero
    b.close()


def case_teacher_forcing():
    """preload samples of every frame imposed (src/lpcnet.c:256-259): 0, half a frame, the whole frame; one batch, reset in between"""
    from lpcnet_amd import synth
    from oracle import orc
    n, T = 8, 4
    blob = synth.blob_bytes(synth.make_model(**SKEW))
    om = orc.OracleModel(blob)
    b = wide_batch(n, blob)
    feats = np.stack([synth.make_features(6100 + s, T) for s in range(n)])
    rng = np.random.default_rng(7)
    imposed = rng.integers(-9000, 9000, (n, T * 160)).astype(np.int16)
    for preload in (0, 80, 160):
        b.reset()
        pcm_in = np.zeros((n, T * 160), np.int16)
        for t in range(T):
            pcm_in[:, t * 160:t * 160 + preload] = imposed[:, t * 160:t * 160 + preload]
        got = b.synthesize(feats, preload_pcm=pcm_in, preload=preload)
        sts = [om.new_state() for _ in range(n)]
        for s in range(n):
            for t in range(T):
                ref = pcm_in[s, t * 160:(t + 1) * 160].copy()
                sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), ref, 160, preload)
                assert np.array_equal(got[s, t * 160:(t + 1) * 160], ref), (preload, s, t)
        check_states(b, sts)
        assert np.any(got != 0)
    b.close()


def case_partial_reset():
    """streams 2..5 -- two of each group of the workgroup -- start over between two calls; the others go on"""
    from lpcnet_amd import synth
    from oracle import orc
    n, T = 8, 4
    blob = synth.blob_bytes(synth.make_model(**SKEW))
    om = orc.OracleModel(blob)
    sts = [om.new_state() for _ in range(n)]
    b = wide_batch(n, blob)
    feats = np.stack([synth.make_features(5100 + s, T) for s in range(n)])
    first = b.synthesize(feats)
    assert np.array_equal(first, np.stack([sts[s].synthesize(feats[s]) for s in range(n)]))
    b.reset(2, 4)
    for s in range(2, 6):
        sts[s] = om.new_state()
    second = b.synthesize(feats)
    for s in range(n):
        assert np.array_equal(second[s], sts[s].synthesize(feats[s])), s
    check_states(b, sts)
    assert np.any(second[[0, 1, 6, 7]] != 0) and np.all(second[2:6, :320] == 0)
    b.close()


def case_plc():
    """nine streams through plc_step with losses: the compacted groups launch at eight under the group schedule, and the output is the one the
    batch gives with the switch off (the four-stream kernel)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import plc_model as pm
    import plc_synth
    from plc_run import run
    from lpcnet_amd import api, synth
    n, T = 9, 24
    blob = synth.blob_bytes(plc_synth.make_model_with_plc(flavour="float", **SKEW))
    pcm = np.stack([pm.stream_pcm(s, T) for s in range(n)])
    lost = pm.loss_patterns()[:n, :T].copy()
    lost[:, 10] = [1, 0, 1, 0, 1, 0, 1, 0, 1]                # (whatever the fixture's patterns do this early: a step with two groups)
    lost[:, 11] = 1
    outs = []
    for on in (False, True):
        b = api.LPCNetBatch(n, blob)
        b.plc_enable(api.PLC_CAUSAL)
        if on:
            b.two_group_streaming = True
            b.streams_per_workgroup = 8
        else:
            b.streams_per_workgroup = 4
        b.group_schedule = (1, 1)
        out, forms = [], set()
        for t in range(T):
            out.append(run(b, pcm, lost, t, t + 1))
            g = b.last_groups()
            assert all(S == b.group_form(cnt) for cnt, S in g[:, [2, 6]].tolist())      # (a step may have no group: nothing to synthesise yet)
            forms |= set(g[:, 6].tolist())
        assert forms == ({8} if on else {4}), forms
        outs.append(np.concatenate(out, axis=1))
        b.close()
    assert np.array_equal(outs[0], outs[1])
    assert np.any(outs[1][lost.astype(bool)] != 0) and np.any(outs[1][~lost.astype(bool)] != 0)


def case_switch(which):
    from lpcnet_amd import api, synth
    skew = synth.blob_bytes(synth.make_model(**SKEW))
    if which == "off_by_default":                            # today's behaviour: no two-group image, a pinned eight is refused
        b = api.LPCNetBatch(13, skew)
        assert b.two_group_streaming is False
        with pytest.raises(api.LPCNetError):
            b.streams_per_workgroup = 8
        assert b.streams_per_workgroup != 8 and b.group_form(13) != 8
    elif which in ("int8", "sparse_grub"):
        blob = synth.blob_bytes(synth.make_model(flavour="int8") if which == "int8" else synth.make_model(grub_density=0.5, seed=5))
        b = api.LPCNetBatch(13, blob)
        before = b.streams_per_workgroup
        with pytest.raises(api.LPCNetError) as e:
            b.two_group_streaming = True
        assert "two-group streaming" in str(e.value)
        assert b.two_group_streaming is False and b.streams_per_workgroup == before
        with pytest.raises(api.LPCNetError):
            b.streams_per_workgroup = 8
    elif which == "default_model_noop":
        b = api.LPCNetBatch(13, synth.blob_bytes(synth.make_model()))
        b.streams_per_workgroup = 8
        b.two_group_streaming = True                         # returns 0 and changes nothing
        assert b.two_group_streaming is False and b.streams_per_workgroup == 8
        b.two_group_streaming = False
        assert b.streams_per_workgroup == 8
    elif which == "fast_runs_at_four":
        b = wide_batch(13, skew)
        feats = np.stack([synth.make_features(100 + s, 3) for s in range(13)])
        exact = b.synthesize(feats)
        b.set_fast(True)
        assert b.streams_per_workgroup == 4 and b.two_group_streaming is True
        b.reset()
        fast = b.synthesize(feats)
        b.set_fast(False)
        assert b.streams_per_workgroup == 8
        b.reset()
        assert np.array_equal(b.synthesize(feats), exact)
        assert fast.shape == exact.shape and np.any(exact != 0)
    elif which == "no_twelve_waves":
        b = wide_batch(13, skew)
        assert b.twelve_waves == 0
        with pytest.raises(api.LPCNetError):
            b.twelve_waves = 1
        assert b.twelve_waves == 0 and b.streams_per_workgroup == 8
    elif which == "off_while_pinned":
        b = wide_batch(13, skew)
        with pytest.raises(api.LPCNetError):
            b.two_group_streaming = False
        assert b.two_group_streaming is True and b.streams_per_workgroup == 8
        b.streams_per_workgroup = 0                          # the engine's choice again: the cost table never picks eight for a wide image
        assert b.streams_per_workgroup != 8
        b.two_group_streaming = False
        assert b.two_group_streaming is False
        with pytest.raises(api.LPCNetError):
            b.streams_per_workgroup = 8
        b.two_group_streaming = True                         # (the image is kept: on again without another upload)
        b.streams_per_workgroup = 8
        assert b.streams_per_workgroup == 8
    else:
        raise AssertionError(which)
    b.close()


SWITCH = ["off_by_default", "int8", "sparse_grub", "default_model_noop", "fast_runs_at_four", "no_twelve_waves", "off_while_pinned"]
CHILD = {"parity": case_parity, "short_frames": case_short_frames, "teacher_forcing": case_teacher_forcing, "partial_reset": case_partial_reset,
         "plc": case_plc, "switch": case_switch}

# ---------------------------------------------------------------------------------------------------------- the parent
_faulted = []      # the first step that ended on a signal or a time limit


def run_step(case, arg=None, limit=300):
    assert not _faulted, "not started: GPU step %s ended abnormally before this one" % _faulted[0]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LPCN_DEAL") and k != "LPCNET_HIP_X2_STREAMED"}
    cmd = [sys.executable, os.path.abspath(__file__), case] + ([repr(arg)] if arg is not None else [])
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _faulted.append("%s %s (time limit of %d s)" % (case, arg, limit))
        pytest.fail("GPU step ran into its time limit: %s\n%s" % (_faulted[0], e.stdout or ""))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _faulted.append("%s %s (exit status %d)" % (case, arg, r.returncode))
    assert r.returncode == 0, "exit status %d\n%s" % (r.returncode, r.stdout[-4000:])


@pytest.mark.parametrize("name", list(MODELS))
def test_models_beyond_32_items_per_lane_against_the_oracle(name, hip_lib):
    run_step("parity", MODELS[name])


@pytest.mark.parametrize("N", [1, 7, 159])
def test_frames_of_n_samples(N, hip_lib):
    run_step("short_frames", N)


def test_teacher_forcing(hip_lib):
    run_step("teacher_forcing")


def test_partial_reset_in_both_groups_of_a_workgroup(hip_lib):
    run_step("partial_reset")


def test_plc_groups_launch_at_eight_and_match_the_four_stream_kernel(hip_lib):
    run_step("plc")


@pytest.mark.parametrize("which", SWITCH)
def test_the_switch(which, hip_lib):
    run_step("switch", which)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    CHILD[sys.argv[1]](*[eval(a) for a in sys.argv[2:]])
    print("ok")
