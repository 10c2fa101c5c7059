"""GPU parity tests of the twelve-wave form of the two-group sample kernel (lpcnet_amd/csrc/sample_kernel_x3.hip.h: eight float streams per workgroup on
three waves per SIMD, 16 items per lane, candidate slots cut head / tail), forced through the C ABI (twelve_waves = 1), against the plain-C oracle, the
reference-generated golden fixtures and the eight-wave form.  Same bar as tests/test_gpu_x2.py: PCM, GRU states, LPC history, RNG state bit for bit."""
import numpy as np
import pytest

from lpcnet_amd import api, synth
from oracle import orc

pytestmark = pytest.mark.gpu


def feats_for(seeds, T):
    return np.stack([synth.make_features(s, 60)[:T] if T <= 60 else synth.make_features(s, T) for s in seeds])


def batch12(n, blob):
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = 8
    b.twelve_waves = 1
    assert b.streams_per_workgroup == 8 and b.twelve_waves == 1
    return b


def check_states(b, states, which):
    for s in which:
        st = b.get_state(s)
        c1, c2, ga, gb = states[s].nnet_state()
        ls, le, dm, fc, rng = states[s].signal_state()
        assert np.array_equal(np.array(st.gru_a, np.float32), ga) and np.array_equal(np.array(st.gru_b, np.float32), gb), s
        assert np.array_equal(np.array(st.conv1_mem, np.float32), c1) and np.array_equal(np.array(st.conv2_mem, np.float32), c2), s
        assert np.array_equal(np.array(st.last_sig, np.float32), ls) and st.last_exc == le and st.frame_count == fc, s
        assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s


def oracle_states(blob, feats):
    om = orc.OracleModel(blob)
    pcm, states = [], []
    for f in feats:
        st = om.new_state()
        pcm.append(st.synthesize(f))
        states.append(st)
    return np.stack(pcm), states


@pytest.mark.parametrize("n", [8, 16, 13, 5, 1, 24])
def test_twelve_waves_match_the_oracle(n, blob_f32, hip_lib):
    T = 7
    feats = feats_for(range(2600, 2600 + n), T)
    want, states = oracle_states(blob_f32, feats)
    b = batch12(n, blob_f32)
    got = b.synthesize(feats)
    assert np.array_equal(got, want)
    check_states(b, states, range(n))
    b.close()


def test_golden_reference_pcm_on_twelve_waves(blob_f32, golden, hip_lib):
    T = int(golden["n_frames"])
    seeds = [1000 + s % 3 for s in range(8)]
    b = batch12(8, blob_f32)
    pcm = b.synthesize(feats_for(seeds, T))
    for s, seed in enumerate(seeds):
        assert np.array_equal(pcm[s], golden[f"pcm_gf_{seed}"]), s
        st = b.get_state(s)
        assert np.array_equal(np.array(st.gru_a, np.float32), golden[f"gru_a_gf_{seed}"])
        assert np.array_equal(np.array(st.gru_b, np.float32), golden[f"gru_b_gf_{seed}"])
    b.close()


def test_streaming_calls_and_chunks_equal_one_call_and_the_eight_wave_form(blob_f32, hip_lib):
    n, T = 11, 104
    feats = feats_for(range(4100, 4100 + n), T)
    b = batch12(n, blob_f32)
    whole = b.synthesize(feats)
    b.reset()
    parts = [b.synthesize(np.ascontiguousarray(feats[:, a:z])) for a, z in ((0, 1), (1, 2), (2, 3), (3, 50), (50, 104))]
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    b8 = api.LPCNetBatch(n, blob_f32)
    b8.streams_per_workgroup = 8
    b8.twelve_waves = 0
    assert b8.twelve_waves == 0
    assert np.array_equal(b8.synthesize(feats), whole)
    for s in range(n):
        assert bytes(b8.get_state(s)) == bytes(b.get_state(s)), s      # the complete record, RNG included
    b.close(); b8.close()


def test_partial_reset_across_the_groups(blob_f32, hip_lib):
    n, T = 8, 5
    feats = feats_for(range(5100, 5100 + n), T)
    b = batch12(n, blob_f32)
    first = b.synthesize(feats)
    b.reset(1, 2)
    b.reset(4, 4)
    second = b.synthesize(feats)
    om = orc.OracleModel(blob_f32)
    for s in range(n):
        st = om.new_state()
        assert np.array_equal(st.synthesize(feats[s]), first[s])
        if s in (1, 2, 4, 5, 6, 7):
            st = om.new_state()
        assert np.array_equal(st.synthesize(feats[s]), second[s]), s
    b.close()


def test_teacher_forcing(blob_f32, golden, hip_lib):
    f = np.repeat(synth.make_features(1000, 20)[None], 8, axis=0)
    b = batch12(8, blob_f32)
    forced = np.repeat(golden["forced_pcm_in"][None, :], 8, axis=0)
    out = b.synthesize(f, preload_pcm=forced, preload=160)
    want = forced.copy()
    want[:, :320] = 0
    assert np.array_equal(out, want)
    for s in (0, 3, 4, 7):
        st = b.get_state(s)
        assert np.array_equal(np.array(st.gru_a, np.float32), golden["forced_gru_a"])
        assert np.array_equal(np.array(st.gru_b, np.float32), golden["forced_gru_b"])
        assert np.array_equal(np.array(st.last_sig, np.float32), golden["forced_last_sig"])
        assert st.last_exc == int(golden["forced_last_exc"]) and np.array_equal(np.array(st.rng, np.uint32), golden["forced_rng"])
    b.reset()
    half_in = np.zeros((8, 20 * 160), np.int16)
    for t in range(20):
        half_in[:, t * 160:t * 160 + 80] = golden["forced_pcm_in"][t * 160:t * 160 + 80]
    half = b.synthesize(f, preload_pcm=half_in, preload=80)
    for s in range(8):
        assert np.array_equal(half[s], golden["half_forced_pcm"]), s
    b.close()


@pytest.mark.parametrize("N", [160, 40, 1])
def test_frames_of_n_samples(N, blob_f32, hip_lib):
    n, T = 9, 6
    feats = feats_for(range(5300, 5300 + n), T)
    om = orc.OracleModel(blob_f32)
    b = batch12(n, blob_f32)
    sts = [om.new_state() for _ in range(n)]
    for t in range(T):
        pcm = np.zeros((n, 160), np.int16)
        got = b.synthesize_step(np.ascontiguousarray(feats[:, t]), pcm, [N] * n, [0] * n, [1] * n)
        for s in range(n):
            ref = np.zeros(160, np.int16)
            sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, t, :20]), ref, N, 0)
            assert np.array_equal(got[s, :N], ref[:N]), (t, s)
    b.close()


@pytest.mark.parametrize("kw", [
    dict(densities=(0.03, 0.03, 0.12)),
    dict(densities=(0.045, 0.045, 0.18)),
    dict(shaped=False, densities=(0.04, 0.06, 0.15), seed=77),
    dict(off_grid=True),
], ids=["sparseA", "midA", "unshaped", "offgrid"])
def test_other_models_on_twelve_waves(kw, hip_lib):
    """other cuts: slots of <= 16 items whole on a head wave, lanes with fewer blocks than their slot's head"""
    blob = synth.blob_bytes(synth.make_model(**kw))
    assert api.x3_image_info(blob)[0] == 1
    n, T = 10, 6
    feats = feats_for(range(2700, 2700 + n), T)
    want, states = oracle_states(blob, feats)
    b = batch12(n, blob)
    got = b.synthesize(feats)
    assert np.array_equal(got, want), kw
    check_states(b, states, (0, 3, 4, 7, 9))
    b.close()


def test_models_without_the_image_refuse_the_forced_form_and_run_as_before(blob_i8, hip_lib):
    for blob in (blob_i8, synth.blob_bytes(synth.make_model(densities=(0.05, 0.05, 0.3)))):
        b = api.LPCNetBatch(8, blob)
        with pytest.raises(api.LPCNetError):
            b.twelve_waves = 1
        assert b.twelve_waves == 0
        b.close()
    blob = synth.blob_bytes(synth.make_model())
    feats = feats_for(range(2800, 2808), 5)
    b = batch12(8, blob)
    want = b.synthesize(feats)
    b.reset()
    b.set_fast(True)                                        # FAST has no two-group kernel in either form
    assert b.streams_per_workgroup == 4 and b.twelve_waves == 0
    b.set_fast(False)
    assert b.twelve_waves == 1
    b.reset()
    assert np.array_equal(b.synthesize(feats), want)
    b.close()


def test_table_value_stays_on_eight_waves(blob_f32, hip_lib):
    import os
    os.environ["LPCNET_HIP_NO_AUTOTUNE"] = "1"
    try:
        b = api.LPCNetBatch(2048, blob_f32)
        assert b.streams_per_workgroup == 8 and b.twelve_waves == 0
        b.close()
    finally:
        del os.environ["LPCNET_HIP_NO_AUTOTUNE"]


def test_2048_distinct_streams_over_two_calls(blob_f32, hip_lib):
    n, T = 2048, 6
    feats = np.stack([synth.make_features(7000 + s, 2 * T) for s in range(n)])
    b = batch12(n, blob_f32)
    a1 = b.synthesize(np.ascontiguousarray(feats[:, :T]))
    a2 = b.synthesize(np.ascontiguousarray(feats[:, T:]))
    got = np.concatenate([a1, a2], axis=1)
    pick = sorted(set(range(0, n, 16)) | set(range(0, 8)) | set(range(1016, 1024)) | set(range(2040, 2048)))
    want = orc.synthesize_many(blob_f32, np.ascontiguousarray(feats[pick]))
    assert np.array_equal(got[pick], want)
    assert (got != 0).mean() > 0.5
    b.close()
