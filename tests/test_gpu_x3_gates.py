"""GPU tests of stage 1 of the sampling tree on the helper waves of the twelve-wave form of the two-group sample kernel
(lpcnet_amd/csrc/sample_kernel_x3.hip.h; round 14): a chain wave runs GRU-B's chain and gates, stores the new state under the live-mask guard, publishes
the sample's sequence number in a word of its own behind those stores and goes on to its P1 items; the stream's helper wave -- a row wave,
LPCN_X3_HELPERS -- fetches the tree's top rows, polls that word, walks stage 1 on the stored state and publishes the prefix for the stage-2 wave, behind
its own P1 segments; a wave without P1 items skips the P1 block.  Forced through the C ABI (twelve_waves = 1, eight streams per workgroup) and compared
with the plain-C oracle bit for bit -- PCM, GRU states, conv memories, LPC history, last excitation, de-emphasis memory, frame count and RNG words --
and with the eight-wave form on the same inputs (PCM and the complete state record).  What the cases are after:

  * 8, 13, 5 and 1 streams x 3 frames from reset: in the two silent start-up frames the guarded store keeps the old state and the helper walks stage 1
    on it; groups with fewer than four streams, whose chain waves run clamped copies that still publish;
  * a continued second call: the sequence words are cleared at launch and the sequence numbers restart;
  * 1 and 40 samples per call: a launch of one sample has a single chain half-step per group, nothing may poll for a word nobody publishes;
  * a reset of one stream inside a group between two calls;
  * two models whose image puts P1 items on a helper wave (the helper block sits behind the close of those), asserted on the host through
    api.x3_image_info; the benchmark model's image leaves the helper waves' P1 empty, asserted too.

The oracle runs once per module; no test changes what it returned."""
import os
import re

import numpy as np
import pytest

from lpcnet_amd import api, synth
from oracle import orc

pytestmark = pytest.mark.gpu

NMAX, T1, T2 = 13, 3, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def helper_waves():
    """the kernel's compile-time map: nibble s of LPCN_X3_HELPERS is the helper wave of stream s of a group"""
    src = open(os.path.join(ROOT, "lpcnet_amd", "csrc", "sample_kernel_x3.hip.h")).read()
    m = re.search(r"#\s*define\s+LPCN_X3_HELPERS\s+\(?\s*(0[xX][0-9A-Fa-f]+|\d+)[uUlL]*", src)
    assert m, "LPCN_X3_HELPERS is no longer a plain integer literal"
    v = int(m.group(1), 0)
    waves = [(v >> (4 * s)) & 15 for s in range(4)]
    assert v < (1 << 16) and len(set(waves)) == 4 and all(4 <= w < 12 for w in waves)      # four row waves (the kernel's static_assert keeps the leader's and the stage-2 wave out)
    return waves


def p1_items(blob):
    """P1 items per wave of the blob's twelve-wave image (segments 1..4)"""
    have, desc, rows, st = api.x3_image_info(blob)
    assert have == 1 and st == 0
    return desc[:, 1:, 2].sum(axis=1)


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
    """13 streams through the oracle: a call of 3 frames from reset, then either a continued call of 2 frames or the same 2 frames from a fresh state"""
    om = orc.OracleModel(blob_f32)
    f1 = np.stack([synth.make_features(9300 + s, T1) for s in range(NMAX)])
    f2 = np.stack([synth.make_features(9400 + s, T2) for s in range(NMAX)])
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
def test_stream_counts_from_reset_and_a_continued_call(n, ref, blob_f32, hip_lib):
    b12, b8 = batch(n, blob_f32, 1), batch(n, blob_f32, 0)
    for feats, pcm, snaps in ((ref["f1"], ref["pcm1"], ref["snap1"]), (ref["f2"], ref["pcm2"], ref["snap2"])):
        f = np.ascontiguousarray(feats[:n])
        got = b12.synthesize(f)
        assert np.array_equal(got, pcm[:n])
        for s in range(n):
            check_state(b12, s, snaps[s])
        assert np.array_equal(b8.synthesize(f), got)
        same_records(b12, b8, n)
    assert np.all(ref["pcm1"][:n, :320] == 0)                # the two silent start-up frames: the helper walks stage 1 on a state the guarded store has kept
    assert np.any(got != 0)                                  # (the continued call is past them)
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
    n, gone = 8, 6                                           # stream 2 of group 1
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


def test_benchmark_model_leaves_the_helper_waves_p1_empty(blob_f32, hip_lib):
    items = p1_items(blob_f32)
    assert all(items[w] == 0 for w in helper_waves()), items.tolist()


@pytest.mark.parametrize("densities", [(0.08, 0.08, 0.08), (0.08, 0.08, 0.12)], ids=["wave5", "wave8"])
def test_model_with_p1_items_on_a_helper_wave(densities, hip_lib):
    """The models tests/test_gpu_x3.py runs (sparseA, midA, unshaped, offgrid) leave every head wave but the free wave 9 without P1 items, as the
    benchmark model does: the packer fills waves 0..3, 9 and 4 first.  Denser update / reset rows overflow onto the head waves -- 5 P1 items on wave 5
    or on wave 8 here -- so that a helper wave runs P1 segments in front of the helper block."""
    blob = synth.blob_bytes(synth.make_model(densities=densities))
    items = p1_items(blob)
    assert any(items[w] > 0 for w in helper_waves()), items.tolist()
    n, T = 13, 3
    feats = np.stack([synth.make_features(9500 + s, T) for s in range(n)])
    om = orc.OracleModel(blob)
    b12, b8 = batch(n, blob, 1), batch(n, blob, 0)
    sts = [om.new_state() for _ in range(n)]
    want = np.stack([sts[s].synthesize(feats[s]) for s in range(n)])
    got = b12.synthesize(feats)
    assert np.array_equal(got, want)
    for s in range(n):
        check_state(b12, s, snapshot(sts[s]))
    assert np.array_equal(b8.synthesize(feats), got)
    same_records(b12, b8, n)
    assert np.any(got != 0)
    b12.close(); b8.close()
