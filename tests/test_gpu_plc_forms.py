"""Batched packet-loss concealment on EVERY form of the sample kernel and at outage scale.

Every group of a PLC step (run_group, engine_plc.hip) launches with the batch's own streams per workgroup, two-workgroups-per-CU choice and twelve-wave
choice.  A batch of at most one stream per CU picks one stream per workgroup, so tests/test_gpu_plc.py and tests/test_gpu_plc_i8.py compare the
concealment on that form alone; the service shape runs eight.  Here the forms are pinned (as tests/test_gpu_loud.py pins them) and the same
fixtures decide: the reference's own output in tests/golden/golden_plc_v1.npz (generic-C float build) and golden_plc_i8_v1.npz (generic-C int8
build), tolerance 0.  What the groups bring to each form: frames of 80 samples with 80 imposed, the tail-only launch, the trial run whose states
are not scattered back, the kept frame products gathered through the index map -- on compacted groups of 1 to 10 streams that leave most rows of a
workgroup dead (the fixture's independent loss patterns), and on groups that are the whole batch (the outage below).

Each test prints the form it read back from the batch (run with -s to see it)."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from plc_run import run  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

B = pm.BLOCK
# form name -> (flavour, streams per workgroup, twelve waves, LPCNET_HIP_PACK2=1)
FORMS = {
    "f32-S1": ("f32", 1, 0, False), "f32-S2": ("f32", 2, 0, False), "f32-S4": ("f32", 4, 0, False), "f32-S8": ("f32", 8, 0, False),
    "f32-12waves": ("f32", 8, 1, False),
    "int8-S1": ("int8", 1, 0, False), "int8-S2": ("int8", 2, 0, False), "int8-S4": ("int8", 4, 0, False), "int8-S2-pack2": ("int8", 2, 0, True),
}
_cache = {}


def model(flavour):
    """-> (blob, fixture) of a flavour, the blob checked against the fixture's record of it"""
    if flavour not in _cache:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_v1.npz" if flavour == "f32" else "golden_plc_i8_v1.npz"))
        blob = synth.blob_bytes(plc_synth.make_model_with_plc(flavour="float" if flavour == "f32" else "int8"))
        assert np.uint32(zlib.crc32(blob)) == gold["blob_crc"]
        _cache[flavour] = (blob, gold)
    return _cache[flavour]


@pytest.fixture(scope="module")
def pcm_in():
    pcm = np.stack([pm.stream_pcm(s) for s in range(pm.N_STREAMS)])
    assert np.uint32(zlib.crc32(pcm.tobytes())) == model("f32")[1]["in_crc"]
    return pcm


def make_batch(form, n, options, monkeypatch, devices=None):
    """a batch of n streams pinned to the form, the PLC enabled; every setting is read back.  The two-workgroups-per-CU form of the int8 kernel
    cannot be read back: the engine has no getter for it.  LPCNET_HIP_PACK2=1, read when the batch is created, selects it wherever it exists
    (use_pack2, engine.hip: an int8 blob of at most 32 items per lane -- the test blob, tests/test_gpu_wide.py -- at one or two streams per
    workgroup); this test sets the variable and does not assert the selection."""
    flavour, S, twelve, pack2 = FORMS[form]
    if pack2:
        monkeypatch.setenv("LPCNET_HIP_PACK2", "1")
    b = api.LPCNetBatch(n, model(flavour)[0], devices=devices)
    b.streams_per_workgroup = S
    if S == 8:
        b.twelve_waves = twelve
    assert b.streams_per_workgroup == S and b.twelve_waves == twelve
    b.plc_enable(options)
    assert b.plc_flavour() == (flavour == "int8")
    print("form %s: streams_per_workgroup %d, twelve_waves %d%s" % (form, b.streams_per_workgroup, b.twelve_waves, ", LPCNET_HIP_PACK2=1" if pack2 else ""))
    return b


def check_form_after(b, form):
    """the pinned form is still what the batch runs after its steps (nothing measured and replaced it)"""
    _, S, twelve, _ = FORMS[form]
    assert b.streams_per_workgroup == S and b.twelve_waves == twelve


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_end_to_end_on_every_form_of_the_sample_kernel(form, k, pcm_in, hip_lib, monkeypatch):
    """the 64 fixture streams, frames 0 .. 120: the loss in frame 0, the alternating loss, the bursts of 5 and 15 with their recoveries and
    FULL_FRAMES; LPCNET_PLC_CAUSAL and LPCNET_PLC_CODEC | LPCNET_PLC_DC_FILTER"""
    T = 120
    gold = model(FORMS[form][0])[1]
    opt = pm.OPTION_SETS[k]
    assert opt == (api.PLC_CAUSAL, None, None, api.PLC_CODEC | api.PLC_DC_FILTER)[k]
    lost = pm.loss_patterns()
    b = make_batch(form, pm.N_STREAMS, opt, monkeypatch)
    out = run(b, pcm_in, lost, 0, T)
    check_form_after(b, form)
    b.close()
    f0, f1 = pm.FULL_FRAMES
    assert f1 <= T
    bad = np.argwhere(out[pm.FULL_STREAM, f0:f1] != gold["pcm_full"][k])
    assert bad.size == 0, "options %d stream %d from frame %d: first differing (frame, sample) %s of %d" % (opt, pm.FULL_STREAM, f0, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["pcm_crc"][k][:, :T // B])
    assert bad.size == 0, "options %d: first differing (stream, block of %d frames) %s of %d" % (opt, B, bad[:6].tolist(), len(bad))
    assert (out[lost[:, :T].astype(bool)] != 0).mean() > 0.5          # the concealment is not silence


@pytest.mark.parametrize("form", ["f32-S8", "f32-12waves"])
def test_fec_schedules_on_eight_streams_per_workgroup(form, pcm_in, hip_lib, monkeypatch):
    T, n = 180, 16                                     # the FEC streams and eight without a schedule
    gold = model("f32")[1]
    ops, vec = pm.fec_schedule()
    lost = pm.fec_loss_patterns()
    b = make_batch(form, n, api.PLC_CAUSAL, monkeypatch)
    out = run(b, pcm_in, lost, 0, T, ops=ops, vec=vec)
    check_form_after(b, form)
    b.close()
    f0, f1 = pm.FEC_FULL_FRAMES
    assert f1 <= T
    bad = np.argwhere(out[pm.FEC_FULL_STREAM, f0:f1] != gold["fec_full"])
    assert bad.size == 0, "stream %d from frame %d: first differing (frame, sample) %s of %d" % (pm.FEC_FULL_STREAM, f0, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["fec_crc"][:n, :T // B])
    assert bad.size == 0, "first differing (stream, block of %d frames) %s of %d" % (B, bad[:6].tolist(), len(bad))


# ---- an outage: most of the batch lost in the same frames and recovering in the same frame, so every group kind (flush, three queue rounds, tail,
# concealed half, trial synthesis, teacher-forced half) is several full workgroups plus a ragged one.  Slots 0 .. 23 replay fixture stream 6 (lost
# in frames 80 .. 94 and 200 .. 229), slots 24 .. 39 cycle through streams 5, 2, 8 and 0, whose small groups run next to the large one.
OUTAGE = [6] * 24 + [5, 2, 8, 0] * 4


def check_outage(out, gold, k, T, tag):
    # replicas first: a difference between two slots fed the same input is a leak between streams, whatever the fixture says
    for i, s in enumerate(OUTAGE):
        first = OUTAGE.index(s)
        bad = np.argwhere(out[i] != out[first])
        assert bad.size == 0, "%s: slot %d differs from slot %d (both replay stream %d): first (frame, sample) %s of %d" % (tag, i, first, s, bad[:4].tolist(), len(bad))
    bad = np.argwhere(pm.block_crc(out) != gold["pcm_crc"][k][OUTAGE, :T // B])
    assert bad.size == 0, "%s: first differing (slot, block of %d frames) %s of %d" % (tag, B, bad[:6].tolist(), len(bad))


@pytest.mark.parametrize("form,k", [("f32-S4", 0), ("f32-S8", 0), ("f32-S8", 1), ("f32-12waves", 0), ("int8-S4", 0)])
def test_outage_the_whole_batch_in_one_group(form, k, pcm_in, hip_lib, monkeypatch):
    T = 120
    lost = pm.loss_patterns()
    assert lost[6, 80:95].all() and not lost[6, :80].any() and not lost[6, 95:T].any()
    gold = model(FORMS[form][0])[1]
    b = make_batch(form, len(OUTAGE), pm.OPTION_SETS[k], monkeypatch)
    out = run(b, pcm_in, lost, 0, T, streams=OUTAGE)
    check_form_after(b, form)
    b.close()
    check_outage(out, gold, k, T, "%s options %d" % (form, pm.OPTION_SETS[k]))
    assert (out[:24, 80:95] != 0).mean() > 0.5


def test_outage_slots_on_two_shards(pcm_in, hip_lib, monkeypatch):
    T = 60
    b = make_batch("f32-S8", len(OUTAGE), api.PLC_CAUSAL, monkeypatch, devices=[0, 0])
    assert [c for _, c, _ in b.shards] == [20, 20]
    out = run(b, pcm_in, pm.loss_patterns(), 0, T, streams=OUTAGE)
    check_form_after(b, "f32-S8")
    b.close()
    check_outage(out, model("f32")[1], 0, T, "two shards")
