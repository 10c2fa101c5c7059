"""GPU tests of the two-group sample kernel under FAST fp32 arithmetic (lpcnet_amd/csrc/sample_kernel_x2.hip.h with FAST = true, sample_x2f.hip;
a batch's opt-in: lpcnet_batch_set_fast_two_group / LPCNetBatch.fast_two_group).  GRU-A's items accumulate on the matrix pipe, the activations
are the hardware exp2 / rcp, the tree's terms are fused; the schedule, the leader and GRU-B's chains are PARITY's.  Protocol and constants of
the envelope test: tests/test_gpu_fast.py (forced_states is restated here with the opt-in)."""
import json
import os

import numpy as np
import pytest

from lpcnet_amd import api, synth

pytestmark = pytest.mark.gpu
ENVELOPE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simd_envelope_v1.json")))


def fast8_batch(n, blob, pin=True):
    """a batch on the two-group kernel with FAST arithmetic: eight pinned (or the table's choice), the opt-in, FAST = 1"""
    b = api.LPCNetBatch(n, blob)
    if pin:
        b.streams_per_workgroup = 8
    b.fast_two_group = True
    b.set_fast(True)
    return b


def raw(b, s):
    return bytes(b.get_state(s))


# ----------------------------------------------------------------------------------------------- 1: selection and switching
def test_selection_and_switching(blob_f32, blob_i8, hip_lib):
    n, T = 8, 5
    feats = np.stack([synth.make_features(7100 + s, T) for s in range(n)])
    b = api.LPCNetBatch(n, blob_f32)
    assert b.fast_two_group is False
    b.streams_per_workgroup = 8
    parity = b.synthesize(feats)
    b.reset()
    b.set_fast(True)
    assert b.streams_per_workgroup == 4                     # without the opt-in: as before
    b.fast_two_group = True
    assert b.fast_two_group is True and b.streams_per_workgroup == 8
    pcm = b.synthesize(feats)
    assert pcm.shape == parity.shape and np.all(pcm[:, :320] == 0) and np.any(pcm[:, 320:] != 0)
    assert np.all(np.abs(pcm[:, 320:].astype(np.int32)).max(axis=1) > 0)      # every stream of both groups is live
    b.set_fast(2)                                           # fp16 dual FC: not on this kernel
    assert b.streams_per_workgroup == 4
    b.set_fast(True)
    with pytest.raises(api.LPCNetError):                    # FAST on, eight pinned: the switch cannot go
        b.fast_two_group = False
    assert b.fast_two_group is True
    b.set_fast(False)
    assert b.streams_per_workgroup == 8
    b.reset()
    assert np.array_equal(b.synthesize(feats), parity)      # PARITY's bits, whatever the switch says
    b.fast_two_group = False                                # (PARITY active: nothing that runs depends on it)
    assert b.fast_two_group is False
    b.close()
    for blob in (blob_i8, synth.blob_bytes(synth.make_model(grub_density=0.5)), synth.blob_bytes(synth.make_model(densities=(0.07, 0.07, 0.25)))):
        b = api.LPCNetBatch(n, blob)
        with pytest.raises(api.LPCNetError):
            b.fast_two_group = True
        assert b.fast_two_group is False
        b.close()


# ----------------------------------------------------------------------------------------------- 2: teacher-forced envelope
def forced_states(blob, feats, pcm, fast):
    """tests/test_gpu_fast.py: forced_states at eight streams per workgroup, with the opt-in on the FAST batch"""
    n, T, _ = feats.shape
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = 8
    if fast:
        b.fast_two_group = True
    b.set_fast(fast)
    assert b.streams_per_workgroup == 8
    ga, gb = np.zeros((T, n, 384), np.float32), np.zeros((T, n, 16), np.float32)
    for t in range(T):
        b.synthesize(np.ascontiguousarray(feats[:, t:t + 1]), preload_pcm=np.ascontiguousarray(pcm[:, t * 160:(t + 1) * 160]), preload=160)
        for s in range(n):
            st = b.get_state(s)
            ga[t, s] = np.array(st.gru_a, np.float32)
            gb[t, s] = np.array(st.gru_b, np.float32)
    b.close()
    return ga, gb


MODELS = {"default": {}, "sparseA": dict(densities=(0.02, 0.02, 0.1))}
_forced_ref = {}


def forced_reference(model):
    """per model, once: the blob, 16 streams' features, PARITY's signal and its teacher-forced states (bit-exact whatever the batch size: the
    first 13 streams serve the 13-stream case)"""
    if model not in _forced_ref:
        blob = synth.blob_bytes(synth.make_model(flavour="float", **MODELS[model]))
        n, T = 16, 100
        feats = np.stack([synth.make_features(8800 + s, T) for s in range(n)])
        ref = api.LPCNetBatch(n, blob)
        pcm = ref.synthesize(feats)
        ref.close()
        ga_p, gb_p = forced_states(blob, feats, pcm, False)
        for a in (feats, pcm, ga_p, gb_p):
            a.setflags(write=False)
        _forced_ref[model] = (blob, feats, pcm, ga_p, gb_p)
    return _forced_ref[model]


@pytest.mark.parametrize("n", [16, 13])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_fast_two_group_teacher_forced_inside_reference_simd_envelope(model, n, hip_lib):
    """16 streams = two full workgroups; 13 = the second workgroup has group X full and one stream in group Y.  The sparser model is another
    items-per-lane instantiation.  Bounds: those of tests/test_gpu_fast.py for float blobs."""
    env = ENVELOPE["float"]
    p99_a, worst_a, worst_b = env["gru_a"]["p99"], env["gru_a"]["worst"], env["gru_b"]["worst"]
    blob, feats, pcm, ga_p, gb_p = forced_reference(model)
    T = feats.shape[1]
    feats, pcm, ga_p, gb_p = np.ascontiguousarray(feats[:n]), np.ascontiguousarray(pcm[:n]), ga_p[:, :n], gb_p[:, :n]
    ga_f, gb_f = forced_states(blob, feats, pcm, True)
    live = slice(3, T)
    da = np.abs(ga_f - ga_p)[live].max(axis=2).reshape(-1)
    db = np.abs(gb_f - gb_p)[live].max(axis=2).reshape(-1)
    print("FAST two-group, %s, n = %d: gru_a p99 %.3g max %.3g (envelope p99 %.3g worst %.3g), gru_b max %.3g (worst %.3g)"
          % (model, n, np.percentile(da, 99), da.max(), p99_a, worst_a, db.max(), worst_b))
    assert np.abs(ga_p[live]).max() > 0.3
    slack = 1.25
    assert np.percentile(da, 99) <= slack * p99_a and da.max() <= slack * worst_a, (np.percentile(da, 99), da.max(), env)
    assert db.max() <= slack * worst_b, (db.max(), env)
    assert da.max() <= 0.1 * p99_a
    b = fast8_batch(n, blob)
    out = b.synthesize(feats, preload_pcm=pcm, preload=160)
    assert b.streams_per_workgroup == 8
    assert np.array_equal(out[:, 320:], pcm[:, 320:]) and np.all(out[:, :320] == 0)
    b.close()


# ----------------------------------------------------------------------------------------------- 3: the sampler
SAMPLER_SEED0 = 7300         # features of stream s: synth.make_features(SAMPLER_SEED0 + s, 7)


def seventh_frame(blob, states, feats7, mode):
    """frame 7, free-running, of a batch loaded with `states`: mode "parity", "fast4" (the four-stream FAST kernel) or "fast8" (the two-group one)"""
    n = len(states)
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = 8 if mode == "fast8" else 4
    if mode == "fast8":
        b.fast_two_group = True
    b.set_fast(mode != "parity")
    assert b.streams_per_workgroup == (8 if mode == "fast8" else 4)
    for s in range(n):
        b.set_state(s, states[s])
    out = b.synthesize(feats7)
    b.close()
    return out


def sampler_runs(blob, seed0, n=16):
    feats = np.stack([synth.make_features(seed0 + s, 7) for s in range(n)])
    b = api.LPCNetBatch(n, blob)
    b.synthesize(np.ascontiguousarray(feats[:, :6]))
    states = [b.get_state(s) for s in range(n)]
    want = b.synthesize(np.ascontiguousarray(feats[:, 6:7]))      # PARITY, carried on
    b.close()
    f7 = np.ascontiguousarray(feats[:, 6:7])
    return want, {m: seventh_frame(blob, states, f7, m) for m in ("parity", "fast4", "fast8")}


def streams_that_differ(a, ref, k=32):
    return int(np.any(a[:, :k] != ref[:, :k], axis=1).sum())


def test_fast_two_group_sampler_follows_parity_from_identical_states(blob_f32, hip_lib):
    """Teacher forcing overrides the tree's decisions; this case runs free.  16 streams, 6 PARITY frames, then frame 7 from those raw states on PARITY,
    on FAST at four (the existing kernel, the yardstick) and on FAST at eight.  From identical states a FAST kernel leaves PARITY's samples only
    where a logit lies within rounding of its threshold: at most 1 of the 16 streams may differ anywhere in the first 32 samples, for both kernels.
    Seeds: features synth.make_features(7300 + s, 7) for stream s.  Observed on an MI355X: 0 of 16 streams differ on the four-stream FAST kernel and
    0 of 16 on the two-group one; the same 0 / 0 for the seed bases 7400, 7600, 7700, 7800, 7900, 8000 and 8100 (FAST's states sit ~5e-6 from
    PARITY's, so a flipped decision within 32 samples is rare; a broken tree differs on every stream)."""
    want, got = sampler_runs(blob_f32, SAMPLER_SEED0)
    assert np.array_equal(got["parity"], want) and np.any(want != 0)      # the raw state carries everything
    d4, d8 = streams_that_differ(got["fast4"], want), streams_that_differ(got["fast8"], want)
    print("streams of 16 that leave PARITY within 32 samples: FAST at four %d, FAST at eight %d" % (d4, d8))
    assert d4 <= 1, d4
    assert d8 <= 1, d8


# ----------------------------------------------------------------------------------------------- 4: determinism and state carry
def test_fast_two_group_determinism_and_state_carry(blob_f32, hip_lib):
    n, T = 13, 7
    feats = np.stack([synth.make_features(7500 + s, T) for s in range(n)])
    outs, states = [], []
    for split in ((7,), (3, 4), (1,) * 7):
        b = fast8_batch(n, blob_f32)
        parts, t = [], 0
        for k in split:
            parts.append(b.synthesize(np.ascontiguousarray(feats[:, t:t + k])))
            t += k
        assert b.streams_per_workgroup == 8
        outs.append(np.concatenate(parts, axis=1))
        states.append([raw(b, s) for s in range(n)])
        if split == (7,):
            # a partial reset across the two groups of the first workgroup and into the second, then four frames (two of them start-up frames):
            # those streams equal a fresh batch, the others carry on
            b.reset(first=3, count=6)
            again = b.synthesize(np.ascontiguousarray(feats[:, :4]))
            again_states = [raw(b, s) for s in range(3, 9)]
        b.close()
    assert np.any(outs[0][:, 320:] != 0)
    for o, st in zip(outs[1:], states[1:]):
        assert np.array_equal(o, outs[0])
        assert st == states[0]
    fresh = fast8_batch(n, blob_f32)
    want = fresh.synthesize(np.ascontiguousarray(feats[:, :4]))
    assert np.array_equal(again[3:9], want[3:9]) and np.any(want[3:9, 320:] != 0)
    assert again_states == [raw(fresh, s) for s in range(3, 9)]
    fresh.close()


# ----------------------------------------------------------------------------------------------- 5: no dependence on timing
def test_fast_two_group_choice_does_not_depend_on_timing(blob_f32, hip_lib):
    """FAST is never measured: with the opt-in the table picks eight where PARITY gets eight (2 048 streams: eight per CU), four at 1 024, and
    without the opt-in what it always picked"""
    n, T = 2048, 3
    feats = np.stack([synth.make_features(9300 + (s % 16), T) for s in range(n)])
    outs, spw = [], []
    for tuned in (False, True, False):
        b = fast8_batch(n, blob_f32, pin=False)
        if tuned:
            b.tune()
        outs.append(b.synthesize(feats))
        spw.append(b.streams_per_workgroup)
        b.close()
    assert spw == [8, 8, 8], spw
    assert np.any(outs[0][:, 320:] != 0)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    b = fast8_batch(1024, blob_f32, pin=False)
    assert b.streams_per_workgroup == 4
    b.close()
    b = api.LPCNetBatch(n, blob_f32)
    b.set_fast(True)
    assert b.streams_per_workgroup == 4                     # (the FAST table's value at eight streams per CU, as before)
    b.close()
