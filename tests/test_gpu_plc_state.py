"""The state of a PLC stream on the device against the reference's LPCNetPLCState (tests/golden/golden_plc_state_v1.npz, recorded from the
compiled reference by tests/tools/make_golden_plc_state.py), in both directions through the one translator tests/tools/plc_state_map.py:

  export     every replay on the device, stopped at the fixture's checkpoints: what get_plc_state, get_raw_state and get_analysis_state return
             for every stream is, field by field over its live extent, what the reference holds (CRC-32 per field), and the host half is the
             reference's nine ints;
  import     the reference's snapshot set into one slot of a fresh batch of eight whose other slots run replays of their own: the next 20 frames
             are the reference's, sample for sample; the neighbours' output is what it is without the import;
  round trip the device's own export at every snapshot's control state, imported into another batch: the same records and the same continuation.

All comparisons are on bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
import plc_state_map as sm  # noqa: E402
import plc_state_replays as rp  # noqa: E402
from plc_run import run  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

STATE = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_state_v1.npz"))
N_SNAP = len(STATE["snap_at"])
SLOTS = (0, 3, 7)                          # the slot of a batch of eight a snapshot goes to, by snapshot index
NEIGHBOURS = (2, 7, 8, 9, 10, 11, 12)      # streams of plc_model.loss_patterns the other seven slots run from reset (losses within 20 frames)


@pytest.fixture(scope="module")
def blobs():
    return {"float": synth.blob_bytes(plc_synth.make_model_with_plc()), "int8": synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))}


@pytest.fixture(scope="module")
def events():
    return rp.events


def export(b, s):
    raw = C.create_string_buffer(b.L.lpcnet_batch_state_size())
    assert b.L.lpcnet_batch_get_raw_state(b.p, s, raw) == 0
    return b.get_plc_state(s), raw.raw, b.get_analysis_state(s)


def set_all(b, s, recs):
    b.set_plc_state(s, recs[0])
    assert b.L.lpcnet_batch_set_raw_state(b.p, s, C.create_string_buffer(recs[1], len(recs[1]))) == 0
    b.set_analysis_state(s, recs[2])


def snap_key(i):
    return str(STATE["replays"][STATE["snap_replay"][i]]), int(STATE["snap_stream"][i]), int(STATE["snap_at"][i])


def snapshot(i):
    return {k: STATE["snap_" + k][i] for k in sm.SNAP_FIELDS}


def advance(b, ev, t0, t1):
    """frames [t0, t1) of a whole replay: the plc_model replays through plc_run.run, the FEC script through one plc_fec_feed per frame"""
    if ev.name == "script":
        return rp.run_engine(b, ev, t0, t1)
    return run(b, ev.pcm, ev.lost, t0, t1, ops=ev.op, vec=ev._vec if ev.op is not None else None)


@pytest.mark.parametrize("replay", list(rp.REPLAYS))
def test_export_equals_the_reference_at_every_checkpoint(replay, blobs, events, hip_lib):
    ev = events(replay)
    b = api.LPCNetBatch(ev.n, blobs[ev.flavour])
    b.plc_enable(ev.options)
    bad, t = [], 0
    for k, c in enumerate(ev.checkpoints):
        advance(b, ev, t, c)
        t = c
        for s in range(ev.n):
            recs = export(b, s)
            for name in sm.differing(sm.crcs(*recs), STATE["crc_" + replay][k, s]):
                bad.append((replay, "stream %d" % s, "after %d frames" % c, name))
            ints = np.frombuffer(recs[0], sm.PLC_REC)[0]["ctl"]
            for j in np.flatnonzero(ints != STATE["ctl_" + replay][c - 1, s]):
                bad.append((replay, "stream %d" % s, "after %d frames" % c, "host int " + sm.CTL_NAMES[j]))
    b.close()
    print("%s: %d (stream, checkpoint, field) differ" % (replay, len(bad)))
    for line in bad[:40]:
        print("  ", line)
    assert not bad, "%d differences, the first: %s; fields: %s" % (len(bad), bad[0], sorted({x[3] for x in bad}))


_NEIGHBOUR_INPUT = []


def neighbour_frames(slot, k):
    """frame k of the batch of eight without the slot's row: (pcm [8][160], lost [8]); the other slots run NEIGHBOURS in order, from frame 0"""
    if not _NEIGHBOUR_INPUT:
        _NEIGHBOUR_INPUT.extend([pm.loss_patterns()[list(NEIGHBOURS), :rp.CONT], np.stack([pm.stream_pcm(s, rp.CONT) for s in NEIGHBOURS])])
    lost_n, pcm_n = _NEIGHBOUR_INPUT
    pcm = np.zeros((8, 160), np.int16)
    lost = np.zeros(8, np.uint8)
    for j, i in enumerate(x for x in range(8) if x != slot):
        lost[i] = lost_n[j, k]
        pcm[i] = 0 if lost[i] else pcm_n[j, k]
    return pcm, lost


def continue_slot(b, slot, ev, s, at):
    """the slot's next 20 frames with its FEC traffic, beside the neighbours' first 20 -> [8][20][160]"""
    out = np.zeros((8, rp.CONT, 160), np.int16)
    for k in range(rp.CONT):
        ev.feed_engine(b, slot, at + k, s)
        pcm, lost = neighbour_frames(slot, k)
        pcm[slot], lost[slot] = ev.frame(at + k, s), ev.lost[s, at + k]
        out[:, k] = b.plc_step(pcm, lost)
    return out


def check_after_continuation(b, slot, replay, s, at):
    """the slot's state after the 20 frames: the reference's ints, and its fields where a checkpoint falls there"""
    recs = export(b, slot)
    assert np.array_equal(np.frombuffer(recs[0], sm.PLC_REC)[0]["ctl"], STATE["ctl_" + replay][at + rp.CONT - 1, s])
    ck = rp.REPLAYS[replay][4]
    if at + rp.CONT in ck:
        assert sm.differing(sm.crcs(*recs), STATE["crc_" + replay][ck.index(at + rp.CONT), s]) == []


@pytest.mark.parametrize("i", range(N_SNAP))
def test_import_of_the_references_state_continues_like_the_reference(i, blobs, events, hip_lib):
    replay, s, at = snap_key(i)
    ev, slot = events(replay), SLOTS[i % 3]
    # the neighbours without the import: the slot runs the snapshot's stream from reset instead
    base = api.LPCNetBatch(8, blobs[ev.flavour])
    base.plc_enable(ev.options)
    want = continue_slot(base, slot, ev, s, 0)
    base.close()
    b = api.LPCNetBatch(8, blobs[ev.flavour])
    b.plc_enable(ev.options)
    recs = sm.from_reference(snapshot(i))
    set_all(b, slot, recs)
    back = export(b, slot)
    assert sm.diff_report(sm.fields(*back), sm.fields(*recs)) == []
    got = continue_slot(b, slot, ev, s, at)
    others = [x for x in range(8) if x != slot]
    d = np.argwhere(got[slot] != STATE["snap_cont"][i])
    assert d.size == 0, "%s stream %d after %d frames (%s): continuation frame %d sample %d is %d, the reference has %d" % (
        replay, s, at, STATE["snap_why"][i], d[0][0], d[0][1], got[slot][tuple(d[0])], STATE["snap_cont"][i][tuple(d[0])])
    assert np.array_equal(got[others], want[others]), "the import changed a neighbour's output"
    check_after_continuation(b, slot, replay, s, at)
    b.close()


@pytest.mark.parametrize("i", range(N_SNAP))
def test_round_trip_of_the_devices_export_at_every_snapshot_state(i, blobs, events, hip_lib):
    replay, s, at = snap_key(i)
    ev, slot = events(replay), SLOTS[(i + 1) % 3]
    # the stream's own replay up to the snapshot's frame, in a slot of a batch of eight whose other slots receive silence until then
    a = api.LPCNetBatch(8, blobs[ev.flavour])
    a.plc_enable(ev.options)
    for t in range(at):
        ev.feed_engine(a, slot, t, s)
        pcm, lost = np.zeros((8, 160), np.int16), np.zeros(8, np.uint8)
        pcm[slot], lost[slot] = ev.frame(t, s), ev.lost[s, t]
        a.plc_step(pcm, lost)
    recs = export(a, slot)
    report = sm.diff_report(sm.fields(*recs), sm.fields(*sm.from_reference(snapshot(i))))
    assert report == [], "%s stream %d after %d frames: the export differs from the reference's snapshot: %s" % (replay, s, at, report)
    other = SLOTS[(i + 2) % 3]
    b = api.LPCNetBatch(8, blobs[ev.flavour])
    b.plc_enable(ev.options)
    set_all(b, other, recs)
    assert export(b, other) == recs, "get after set returns other bytes"
    got_a = continue_slot(a, slot, ev, s, at)
    got_b = continue_slot(b, other, ev, s, at)
    assert np.array_equal(got_a[slot], STATE["snap_cont"][i]) and np.array_equal(got_b[other], got_a[slot])
    ea, eb = export(a, slot), export(b, other)
    assert sm.diff_report(sm.fields(*eb), sm.fields(*ea)) == []
    check_after_continuation(b, other, replay, s, at)
    a.close()
    b.close()


@pytest.mark.parametrize("why", ["before_received_causal", "before_received_codec"])
def test_import_with_swapped_plc_copies_does_not_continue_like_the_reference(why, blobs, events, hip_lib):
    """the import test has teeth: with plc_copy[1] and plc_copy[2] exchanged in the imported record -- a mix-up the engine's own get -> set round
    trip cannot see -- the first received frame after the loss restores the wrong network state (plc_copy[2] in the cross-fade mode, plc_copy[1]
    in the codec mode) and the continuation leaves the reference's"""
    i = [str(w).split(";")[0] for w in STATE["snap_why"]].index(why)
    replay, s, at = snap_key(i)
    ev = events(replay)
    recs = sm.from_reference(snapshot(i))
    p = np.frombuffer(recs[0], sm.PLC_REC).copy()
    p[0]["net"][[2, 3]] = p[0]["net"][[3, 2]]
    assert p.tobytes() != recs[0]
    b = api.LPCNetBatch(8, blobs[ev.flavour])
    b.plc_enable(ev.options)
    set_all(b, 3, (p.tobytes(), recs[1], recs[2]))
    got = continue_slot(b, 3, ev, s, at)
    b.close()
    assert not np.array_equal(got[3], STATE["snap_cont"][i])
