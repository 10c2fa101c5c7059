"""GPU parity of the sample loop at FULL SCALE: the loud input families of tests/tools/loud_inputs.py (PCM clip on both rails,
both clamps of the mu-law conversion at its three call sites, all 256 rows of the three embedding tables, an LPC history of
several 10^4 with alternating signs -- counted by tests/test_loud_census.py) through every form of the sample kernel.

Same bar as tests/test_gpu_parity.py: tolerance 0 on PCM (including the imposed samples, which must come back untouched),
gru_a, gru_b, last_sig, last_exc, deemph_mem, rng and frame_count.  Expected values: tests/golden/golden_loud_v1.npz (the compiled
reference's own output, float and int8 builds) for the two default blobs, the plain-C oracle (tied to that fixture by
tests/test_loud_golden.py) for the other models and for call patterns the fixture does not hold (short frames, skipped streams).

Families of one group share their per-frame preload counts, so a group fills one batch; every group runs in two arrangements
of its families over the stream slots, so that every row of a workgroup -- and both groups of the two-group kernel -- carries a
clipping stream at least once (the groups p160 and p160_0 impose or follow a loud signal without clipping)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import loud_inputs  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402
from oracle import orc  # noqa: E402

pytestmark = pytest.mark.gpu

T, FRAME = loud_inputs.T, loud_inputs.FRAME
GROUPS = loud_inputs.groups()
FAMS = loud_inputs.by_name()
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_loud_v1.npz"))

# model name -> (make_model arguments, fixture flavour or None)
MODELS = {
    "f32": (dict(flavour="float"), "f"),
    "int8": (dict(flavour="int8"), "i"),
    "streamed": (dict(densities=(0.1, 0.1, 0.35)), None),          # GRU-A items past the 28th streamed from L2
    "sparseB": (dict(grub_density=0.5), None),                      # block-sparse GRU-B input matrix (indexed path)
}
# form name -> (model, streams per workgroup, twelve waves, stream counts)
FORMS = {
    "f32-S1": ("f32", 1, 0, (8,)), "f32-S2": ("f32", 2, 0, (8,)), "f32-S4": ("f32", 4, 0, (8,)),
    "f32-S8": ("f32", 8, 0, (8, 13)), "f32-12waves": ("f32", 8, 1, (8, 13)),
    "int8-S1": ("int8", 1, 0, (8,)), "int8-S2": ("int8", 2, 0, (8,)), "int8-S4": ("int8", 4, 0, (8,)),
    "streamed-S4": ("streamed", 4, 0, (8,)), "sparseB-S4": ("sparseB", 4, 0, (8,)),
}
_cache = {}


def model(name):
    """-> (blob, expected: family name -> (pcm, state dict), conditioning of the tail families)"""
    if name not in _cache:
        kw, fl = MODELS[name]
        blob = synth.blob_bytes(synth.make_model(**kw))
        om = orc.OracleModel(blob)
        want = {}
        for f in FAMS.values():
            if fl is None:
                want[f.name] = loud_inputs.run_oracle(om, f)[:2]
            else:
                st = {k: GOLDEN[f"{k}_{fl}_{f.name}"] for k in loud_inputs.STATE_KEYS}
                want[f.name] = (GOLDEN[f"pcm_{fl}_{f.name}"], dict(st, frame_count=T))
        prods = {f.name: loud_inputs.tail_products(om, f)[:2] for f in FAMS.values() if f.tail}
        _cache[name] = (blob, want, prods)
    return _cache[name]


arrangements = loud_inputs.arrangements


def make_batch(blob, n, S, twelve=0):
    b = api.LPCNetBatch(n, blob)
    b.streams_per_workgroup = S
    if S == 8:
        b.twelve_waves = twelve
        assert b.twelve_waves == twelve
    assert b.streams_per_workgroup == S
    return b


def run_slots(b, slots, prods, frames=(0, T)):
    """frames [a, z) of one family per stream slot (all of one group) through the batch calls: one call per run of frames with one preload count"""
    a0, z0 = frames
    forced = np.stack([f.forced for f in slots])
    if slots[0].tail:
        if a0 == 0:
            for s in range(len(slots)):
                st = b.get_state(s)
                st.frame_count = T                                 # (the oracle and the reference ran the frame network T times before the tail calls)
                b.set_state(s, st)
        ca = np.stack([prods[f.name][0][a0:z0] for f in slots])
        cb = np.stack([prods[f.name][1][a0:z0] for f in slots])
        lpc = np.stack([np.tile(f.lpc, (z0 - a0, 1)) for f in slots])
        return b.run_tail(ca, cb, lpc, preload_pcm=forced[:, a0 * FRAME:z0 * FRAME], preload=slots[0].preload[0])
    feats = np.stack([f.features for f in slots])
    out = []
    for a, z, pre in slots[0].segments():
        a, z = max(a, a0), min(z, z0)
        if a >= z:
            continue
        ff = np.ascontiguousarray(feats[:, a:z])
        out.append(b.synthesize(ff, preload_pcm=forced[:, a * FRAME:z * FRAME], preload=pre) if pre else b.synthesize(ff))
    return np.concatenate(out, axis=1)


def check_state(st, want, tag):
    assert np.array_equal(np.array(st.gru_a, np.float32).view(np.uint32), want["gru_a"].view(np.uint32)), tag
    assert np.array_equal(np.array(st.gru_b, np.float32).view(np.uint32), want["gru_b"].view(np.uint32)), tag
    assert np.array_equal(np.array(st.last_sig, np.float32).view(np.uint32), want["last_sig"].view(np.uint32)), tag
    assert st.last_exc == int(want["last_exc"]) and np.float32(st.deemph_mem) == np.float32(want["deemph_mem"]), tag
    assert np.array_equal(np.array(st.rng, np.uint32), want["rng"]) and st.frame_count == want["frame_count"], tag


def check_slots(b, got, slots, want, tag):
    for s, f in enumerate(slots):
        pcm, st = want[f.name]
        bad = np.nonzero(got[s] != pcm)[0]
        assert bad.size == 0, (tag, s, f.name, "first differing sample", int(bad[0]), int(got[s][bad[0]]), int(pcm[bad[0]]))
        check_state(b.get_state(s), st, (tag, s, f.name))


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("form", list(FORMS))
def test_loud_families_on_every_form_of_the_sample_kernel(form, group, hip_lib):
    mname, S, twelve, counts = FORMS[form]
    blob, want, prods = model(mname)
    for n in counts:                                               # (13 at eight streams per workgroup: a loud stream next to dead rows)
        for k, slots in enumerate(arrangements(group, n)):
            b = make_batch(blob, n, S, twelve)
            got = run_slots(b, slots, prods)
            check_slots(b, got, slots, want, (form, group, n, k))
            b.close()


@pytest.mark.parametrize("S", [4, 8])
def test_step_call_with_a_different_family_preload_and_length_per_stream(S, blob_f32, hip_lib):
    """lpcnet_batch_synthesize_step: every stream of one call another family, its own n_samples (160, 40, 1) and preload, some streams skipped
    in some calls, one stream imposed digital silence: loud, silent and skipped streams share a workgroup.  Expected: the oracle driven
    alone with the same calls (the fixture holds whole frames only)."""
    fams = [f for f in loud_inputs.families() if not f.tail]
    silent = loud_inputs.Family("silent160", "p160", 50, np.zeros(T * FRAME, np.int16), tuple([160] * T))
    fams = fams[:5] + [silent] + fams[5:]
    n = len(fams)
    assert n == 12
    om = orc.OracleModel(blob_f32)
    ost = [om.new_state() for _ in range(n)]
    b = make_batch(blob_f32, n, S)
    ns = np.array([(160, 40, 1)[(s + s // 3) % 3] for s in range(n)], np.int32)
    feats = np.stack([f.features for f in fams])
    for t in range(T):
        mode = np.array([0 if t >= 3 and (t + s) % 5 == 4 else 1 for s in range(n)], np.int32)
        pre = np.array([min(f.preload[t], k) for f, k in zip(fams, ns)], np.int32)
        pcm_in = np.stack([f.forced[t * FRAME:(t + 1) * FRAME] for f in fams])
        want = pcm_in.copy()
        for s in range(n):
            if mode[s]:
                ost[s].L.orc_synthesize(ost[s].p, np.ascontiguousarray(feats[s, t, :20]), want[s], int(ns[s]), int(pre[s]))
        got = b.synthesize_step(np.ascontiguousarray(feats[:, t]), pcm_in, ns, pre, mode)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (S, t, bad[:4].tolist())
    for s in range(n):
        st = _oracle_state(ost[s])
        check_state(b.get_state(s), st, (S, s, fams[s].name))
    b.close()


def _oracle_state(o):
    return loud_inputs._pack_state(o.nnet_state(), o.signal_state())


def test_single_stream_c_api_with_forced_full_scale_pcm(hip_lib):
    """lpcnet_synthesize_impl of the C API (what the PLC drives), frame by frame, on the full-scale alternation"""
    blob, want, _ = model("f32")
    for name in ("alt80", "noise40a"):
        f = FAMS[name]
        st = api.LPCNetState(blob)
        feats = f.features
        pcm = np.concatenate([st.synthesize_impl(feats[t], FRAME, f.forced[t * FRAME:t * FRAME + f.preload[t]]) for t in range(T)])
        assert np.array_equal(pcm, want[name][0]), name
        rec = api.StreamState.from_buffer_copy(st.raw_bytes()[8:8 + C.sizeof(api.StreamState)])
        check_state(rec, want[name][1], name)


@pytest.mark.parametrize("form", ["f32-S4", "f32-S8", "f32-12waves", "int8-S4"])
def test_calls_split_inside_a_loud_stretch_equal_one_call(form, hip_lib):
    """state carried across a call boundary in the middle of the loud signal: the batch calls split at frames 7 and 8, and -- through the
    step call, whose frame step / tail step pair cuts a frame anywhere -- every stream split directly after one of its clipped samples"""
    mname, S, twelve, _ = FORMS[form]
    blob, want, prods = model(mname)
    n = 8
    for group in ("p80", "p40", "tail16"):
        slots = arrangements(group, n)[1]
        b = make_batch(blob, n, S, twelve)
        got = np.concatenate([run_slots(b, slots, prods, fr) for fr in ((0, 7), (7, 8), (8, T))], axis=1)
        check_slots(b, got, slots, want, (form, group, "frames"))
        b.close()
    slots = arrangements("p80", n)[0]
    b = make_batch(blob, n, S, twelve)
    feats = np.stack([f.features for f in slots])
    got = np.stack([f.forced for f in slots]).copy()
    cuts = []                                                       # per stream: (frame, samples of the frame step); the rest is the tail step
    for f in slots:                                                 # its first clipped free-running sample from frame 5 on; none (the quiet stream): frame 9, sample 100
        pcm = want[f.name][0].astype(np.int32)
        hit = [(t, i) for t in range(5, T) for i in range(f.preload[t], FRAME - 1) if abs(pcm[t * FRAME + i]) == 32767]
        cuts.append((hit[0][0], hit[0][1] + 1) if hit else (9, 101))
    assert sum(abs(int(want[f.name][0][t * FRAME + k - 1])) == 32767 for f, (t, k) in zip(slots, cuts)) >= 4
    for t in range(T):
        frame = got[:, t * FRAME:(t + 1) * FRAME]
        pre = np.array([f.preload[t] for f in slots], np.int32)
        k = np.array([ck if ct == t else FRAME for ct, ck in cuts], np.int32)
        assert (pre <= k).all()
        head = b.synthesize_step(np.ascontiguousarray(feats[:, t]), frame, k, pre, np.ones(n, np.int32))
        rest = np.zeros((n, FRAME), np.int16)
        for s in range(n):
            frame[s, :k[s]] = head[s, :k[s]]
            rest[s, :FRAME - k[s]] = frame[s, k[s]:]
        if (k < FRAME).any():
            tail = b.synthesize_step(np.ascontiguousarray(feats[:, t]), rest, np.maximum(FRAME - k, 1), np.zeros(n, np.int32), np.where(k < FRAME, 2, 0).astype(np.int32))
            for s in range(n):
                frame[s, k[s]:] = tail[s, :FRAME - k[s]]
    check_slots(b, got, slots, want, (form, "p80", "cut behind a clipped sample"))
    b.close()
