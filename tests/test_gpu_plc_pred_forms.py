"""The PLC prediction kernels at 2, 4 and 8 streams per workgroup (plc_kernels.hip.h: plc_pred_s_kernel<S>, plc_pred_s_int8_kernel<S>), pinned with
LPCNetBatch.plc_pred_form: bit for bit what one stream per workgroup gives.

  prediction seam   11 streams, each with its own input trace -- every S has full workgroups and a short last one (8 + 3, 4 + 4 + 3, 5 x 2 + 1) --
                    against the NumPy restatements (plc_i8_model.pred_traces) at the widths where the kernels take another path; one stream at S = 8
  whole step        the reference-tied fixtures replayed under each pinned S: golden_plc_v1 / golden_plc_i8_v1 (the first 100 of their 300 frames, all
                    64 streams) and golden_plc_fec_v1 (all of it).  The fixtures hold PCM, no state records: the PCM is compared with the fixture and
                    every stream's get_plc_state bytes with the S = 1 run of the same replay.  Before that the host planner must show that the
                    replay puts different flag words into one workgroup at S = 2
  across forms      11 streams under random loss with FEC on some, on the 128 / 256 / 256 networks: S = 2, 4, 8 against S = 1
  layout            two shards with an active prefix below the capacity, copy_streams between steps
All comparisons on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_fec_script as fs  # noqa: E402
import plc_i8_model as pq  # noqa: E402
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from plc_run import run  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

N = 11
FORMS = (2, 4, 8)
FLAVOURS = ("float", "int8")
WIDTHS = [((4, 8, 8), None), ((8, 8, 40), None), ((64, 264, 24), 0.3), ((128, 256, 256), None), ((512, 512, 512), None)]
PLC_T_PRED, PRED_REC = 1, 6                              # plc_plan.h, plc_records.h


def width_id(w):
    return "%d-%d-%d%s" % (w[0] + (("-sparse",) if w[1] else ("",)))


# ------------------------------------------------------------------------------------------------ prediction seam -----
@pytest.fixture(scope="module")
def restated():
    """(widths, density, flavour) -> (blob, inputs [N][steps][57], the restatement's outputs [N][steps][20]), made once and shared by the forms"""
    made = {}

    def get(widths, density, flavour):
        key = (widths, density, flavour)
        if key not in made:
            d1, g1, g2 = widths
            blob = pm.blob_widths(d1, g1, g2, flavour, block_density=density)
            if density:                                  # about 30 % of the blocks, and in each GRU at least one row group without any
                a = pm.blob_arrays(blob)
                for name, n_in, n in (("plc_gru1", d1, g1), ("plc_gru2", g1, g2)):
                    counts = pm.group_counts(np.frombuffer(a[name + "_weights_idx"], np.int32), 3 * n // 8)
                    assert counts.count(0) >= 1 and 0.2 < sum(counts) / (n_in // 4 * len(counts)) < 0.4, (name, counts)
            steps = 3 if g1 == 512 else 4
            xs = np.stack([pm.pred_inputs(steps, seed=[0x9ED, s]) for s in range(N)])
            assert len({x.tobytes() for x in xs}) == N
            want = pq.pred_traces(blob, flavour == "int8", xs)
            want.setflags(write=False)
            made[key] = (blob, xs, want)
        return made[key]
    return get


@pytest.mark.parametrize("S", FORMS)
@pytest.mark.parametrize("widths,density", WIDTHS, ids=[width_id(w) for w in WIDTHS])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_prediction_equals_the_restatement_in_every_form(flavour, widths, density, S, restated, hip_lib):
    blob, xs, want = restated(widths, density, flavour)
    steps = xs.shape[1]
    b = api.LPCNetBatch(N, blob)
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_flavour() == (flavour == "int8")
    assert b.plc_pred_form(S) == S and b.plc_pred_form(n_streams=1) == S
    got = np.stack([b.plc_pred(xs[:, t]) for t in range(steps)])                        # [steps][N][20]
    b.close()
    for s in range(N):
        bad = np.argwhere(got[:, s].view(np.uint32) != want[s].view(np.uint32))
        assert bad.size == 0, "%s %s S = %d stream %d: first differing (step, feature) %s of %d" % (flavour, widths, S, s, bad[:4].tolist(), len(bad))
    assert np.isfinite(got).all() and len({got[-1, s].tobytes() for s in range(N)}) == N


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_one_stream_at_eight_per_workgroup(flavour, restated, hip_lib):
    blob, xs, want = restated((128, 256, 256), None, flavour)
    b = api.LPCNetBatch(1, blob)
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_pred_form(8) == 8
    got = np.stack([b.plc_pred(xs[3:4, t]) for t in range(xs.shape[1])])
    b.close()
    assert np.array_equal(got[:, 0].view(np.uint32), want[3].view(np.uint32))


# ----------------------------------------------------------------------------------------------------- whole step -----
def flag_mix_at_two(options, n, lost, feeds=None, ops=None):
    """the host planner over a replay (lost [T][n]; FEC traffic as feeds [T] of (count, skip, clear) or as ops [T][n]) -> (prediction launches in
    which the records 2 w and 2 w + 1 -- one workgroup at S = 2 -- carry different flag words, launches in which they carry different offsets)"""
    ctl = np.zeros((n, 9), np.int32)
    ctl[:, 0] = 400
    mixed = offsets = 0
    for t in range(lost.shape[0]):
        if feeds is not None:
            api.plc_fec_feed_plan(ctl, *feeds[t])
        _, launches, lists = api.plc_plan_lanes(options, ctl, lost[t], 1, None if ops is None else ops[t])
        for la in launches:
            if la[0] != PLC_T_PRED:
                continue
            assert la[6] == PRED_REC
            recs = lists[la[5]:la[5] + la[4] * PRED_REC].reshape(-1, PRED_REC)
            pairs = recs[:len(recs) // 2 * 2].reshape(-1, 2, PRED_REC)
            mixed += bool((pairs[:, 0, 1] != pairs[:, 1, 1]).any())
            offsets += bool((pairs[:, 0, 3:5] != pairs[:, 1, 3:5]).any())
    return mixed, offsets


GOLD_T = 100                                            # frames of the 300 (the fixtures check the output per block of 10 frames)
GOLD_N = {"plain": pm.N_STREAMS, "fec": 16}             # the FEC replay as tests/test_gpu_plc.py runs it: the FEC streams and eight without a schedule


@pytest.fixture(scope="module")
def fixture_runs(hip_lib):
    """(flavour, replay, S) -> (PCM [n][GOLD_T][160], every stream's state record) of the first GOLD_T frames of a replay of golden_plc_v1 /
    golden_plc_i8_v1 in causal mode -- "plain": the loss patterns alone, "fec": the FEC schedule and its loss patterns --, made once each"""
    blobs = {"float": synth.blob_bytes(plc_synth.make_model_with_plc()), "int8": synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))}
    pcm = np.stack([pm.stream_pcm(s)[:GOLD_T] for s in range(pm.N_STREAMS)])          # (the fixture's traces: a shorter trace is another signal)
    ops, vec = pm.fec_schedule()
    script = {"plain": (pm.loss_patterns()[:, :GOLD_T], None, None), "fec": (pm.fec_loss_patterns()[:, :GOLD_T], ops, vec)}
    made = {}

    def get(flavour, replay, S):
        if (flavour, replay, S) not in made:
            lost, ops, vec = script[replay]
            b = api.LPCNetBatch(GOLD_N[replay], blobs[flavour])
            b.plc_enable(api.PLC_CAUSAL)
            assert b.plc_pred_form(S) == S
            out = run(b, pcm, lost, 0, GOLD_T, ops=ops, vec=vec)
            made[(flavour, replay, S)] = (out, [b.get_plc_state(s) for s in range(b.n)])
            b.close()
        return made[(flavour, replay, S)]
    return get, blobs, script


def test_the_replays_put_different_records_into_one_workgroup(fixture_runs, hip_lib):
    """The planner lists the records of one branch of the step together, so the flag words of a list differ where some of its streams conceal from
    FEC vectors and others do not (input selection, PLC_F_KEEP): in the FEC replays.  The plain replay gives a workgroup's streams different
    attenuation offsets (their loss counts differ) under one flag word.  A list never holds a stream with PLC_F_COMPUTE beside one without: what
    separates them is an option of the whole batch"""
    script = fixture_runs[2]
    lost, ops, _ = script["fec"]
    n = GOLD_N["fec"]
    mixed, _ = flag_mix_at_two(api.PLC_CAUSAL, n, np.ascontiguousarray(lost[:n].T), ops=ops[:GOLD_T, :n])
    assert mixed >= 10, mixed
    mixed, offsets = flag_mix_at_two(api.PLC_CAUSAL, pm.N_STREAMS, np.ascontiguousarray(script["plain"][0].T))
    assert mixed == 0 and offsets >= 10, (mixed, offsets)
    sc = fs.script()
    feeds = [(sc["count"][t], sc["skip"][t], sc["clear"][t]) for t in range(fs.T)]
    for options in (api.PLC_CODEC, api.PLC_CAUSAL | api.PLC_DC_FILTER):
        assert flag_mix_at_two(options, fs.N, sc["lost"], feeds=feeds)[0] >= 3, options
    assert api.plc_pred_form_table(pm.N_STREAMS, 256, 128, 16, 16) == 1          # (left alone, these batches run one stream per workgroup)


@pytest.mark.parametrize("S", FORMS)
@pytest.mark.parametrize("replay", ["plain", "fec"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_fixture_replay_in_every_form(flavour, replay, S, fixture_runs, hip_lib):
    get, blobs, script = fixture_runs
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_v1.npz" if flavour == "float" else "golden_plc_i8_v1.npz"))
    assert np.uint32(zlib.crc32(blobs[flavour])) == gold["blob_crc"]
    out, state = get(flavour, replay, S)
    n = GOLD_N[replay]
    want = (gold["pcm_crc"][0] if replay == "plain" else gold["fec_crc"])[:n, :GOLD_T // pm.BLOCK]
    bad = np.argwhere(pm.block_crc(out) != want)
    assert bad.size == 0, "%s %s S = %d: first differing (stream, block of %d frames) %s of %d" % (flavour, replay, S, pm.BLOCK, bad[:6].tolist(), len(bad))
    if replay == "plain":
        f0, f1 = pm.FULL_FRAMES[0], min(pm.FULL_FRAMES[1], GOLD_T)
        assert np.array_equal(out[pm.FULL_STREAM, f0:f1], gold["pcm_full"][0][:f1 - f0])
    assert (out[script[replay][0][:n].astype(bool)] != 0).mean() > 0.5          # the concealment is not silence
    want_out, want_state = get(flavour, replay, 1)
    assert np.array_equal(out, want_out)
    assert [s for s in range(n) if state[s] != want_state[s]] == []


@pytest.fixture(scope="module")
def fec_runs(hip_lib):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_fec_v1.npz"))
    sc = fs.script()
    for k in ("lost", "count", "skip", "clear", "vec"):
        assert np.array_equal(gold[k], sc[k]), k
    assert np.array_equal(gold["pcm_in"], sc["pcm"])
    blobs = [synth.blob_bytes(plc_synth.make_model_with_plc()), synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))]
    assert [zlib.crc32(x) for x in blobs] == gold["blob_crc"].tolist()
    made = {}

    def get(case, S):
        if (case, S) not in made:
            options, i8 = (int(x) for x in gold["cases"][case])
            b = api.LPCNetBatch(fs.N, blobs[i8])
            b.plc_enable(options)
            assert b.plc_pred_form(S) == S
            out = np.zeros((fs.N, fs.T, 160), np.int16)
            for t in range(fs.T):
                r0, r1 = fs.step_rows(sc, t)
                b.plc_fec_feed(sc["vec"][r0:r1], sc["count"][t], sc["skip"][t], sc["clear"][t])
                lo = np.ascontiguousarray(sc["lost"][t])
                frame = np.ascontiguousarray(sc["pcm"][:, t])
                frame[lo != 0] = 0
                out[:, t] = b.plc_step(frame, lo)
            made[(case, S)] = (out, [b.get_plc_state(s) for s in range(fs.N)])
            b.close()
        return made[(case, S)]
    return get, gold


@pytest.mark.parametrize("S", FORMS)
@pytest.mark.parametrize("case", range(3))
def test_fec_fixture_replay_in_every_form(case, S, fec_runs, hip_lib):
    get, gold = fec_runs
    out, state = get(case, S)
    bad = np.argwhere(out != gold["pcm_out"][case])
    assert bad.size == 0, "case %d S = %d: first differing (stream, frame, sample) %s of %d" % (case, S, bad[:4].tolist(), len(bad))
    assert state == get(case, 1)[1]


# --------------------------------------------------------------------------------------------------- across forms -----
T_MIX = 12


def mixed_script(n):
    rng = np.random.default_rng(0x5F0)
    lost = (rng.uniform(size=(T_MIX, n)) < 0.35).astype(np.uint8)
    lost[0] = 0
    count = np.zeros((T_MIX, n), np.int32)
    fed = [1, 4, 5, 8, 10]                               # streams with FEC: some of every workgroup at S = 4, both kinds in one at S = 2
    count[:, fed] = rng.integers(0, 3, (T_MIX, len(fed)))
    vec = (rng.standard_normal((int(count.sum()), 20)) * 0.5).astype(np.float32)
    vec[:, 0] -= np.float32(3.0)
    pcm = np.stack([pm.stream_pcm(s, T_MIX) for s in range(n)])
    return lost, count, vec, pcm


def run_mixed(b, script, steps=range(T_MIX), between=None):
    lost, count, vec, pcm = script
    out = np.zeros((b.n, len(steps), 160), np.int16)
    for i, t in enumerate(steps):
        r0 = int(count[:t].sum())
        b.plc_fec_feed(vec[r0:r0 + int(count[t].sum())], count[t])
        frame = np.ascontiguousarray(pcm[:, t])
        frame[lost[t] != 0] = 0
        out[:, i] = b.plc_step(frame, lost[t])
        if between:
            between(t)
    return out


@pytest.fixture(scope="module")
def blobs_256():
    return {"float": pm.blob_256(), "int8": pq.blob_256_i8()}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_random_loss_and_fec_give_the_same_bytes_in_every_form(flavour, blobs_256, hip_lib):
    script = mixed_script(N)
    mixed = flag_mix_at_two(api.PLC_CODEC, N, script[0], feeds=[(c, None, None) for c in script[1]])[0]
    assert mixed >= 5, mixed
    runs = {}
    for S in (1,) + FORMS:
        b = api.LPCNetBatch(N, blobs_256[flavour])
        b.plc_enable(api.PLC_CODEC)
        assert b.plc_pred_form(S) == S
        runs[S] = (run_mixed(b, script), [b.get_plc_state(s) for s in range(N)])
        b.close()
    assert (runs[1][0][script[0].T.astype(bool)] != 0).mean() > 0.5
    for S in FORMS:
        bad = np.argwhere(runs[S][0] != runs[1][0])
        assert bad.size == 0, "%s S = %d: first differing (stream, frame, sample) %s of %d" % (flavour, S, bad[:4].tolist(), len(bad))
        assert [s for s in range(N) if runs[S][1][s] != runs[1][1][s]] == [], S


# --------------------------------------------------------------------------------------------------------- layout -----
@pytest.mark.parametrize("S", FORMS)
def test_two_shards_an_active_prefix_and_copies_between_steps(S, blobs_256, hip_lib):
    """12 slots on two shards of six, five and four of them active; after step 5 stream 0 is copied over stream 3 (one shard) and stream 7 over
    stream 2 (across the shards).  The pinned form goes to both shards and stays; the results are those of one stream per workgroup"""
    lost, count, vec, pcm = mixed_script(12)
    active = [5, 4]
    idle = [5, 10, 11]
    count[:, idle] = 0
    vec = vec[:int(count.sum())]                         # (any vectors do: both runs feed the same)
    script = (lost, count, vec, pcm)
    runs = {}
    for form in (1, S):
        b = api.LPCNetBatch(12, blobs_256["float"], devices=[0, 0])
        assert [x[:2] for x in b.shards] == [(0, 6), (6, 6)]
        b.plc_enable(api.PLC_CAUSAL)
        b.active = active
        assert b.plc_pred_form(form) == form

        def between(t, b=b):
            if t == 5:
                b.copy_streams([0, 7], [3, 2])
                b.sync()
        out = run_mixed(b, script, between=between)
        assert b.plc_pred_form() == form and b.plc_pred_form(0, n_streams=4) == 1 and b.plc_pred_form(form) == form
        runs[form] = (out, [b.get_plc_state(s) for s in range(12) if s not in idle])
        b.close()
    assert np.array_equal(runs[S][0], runs[1][0]) and runs[S][1] == runs[1][1]
    assert (runs[1][0][:, 6:] != 0).any()


# ------------------------------------------------------------------------------------------------------------ get -----
def test_get_reports_the_pinned_or_the_table_value_and_refuses_other_values(blobs_256, hip_lib):
    b = api.LPCNetBatch(3, blobs_256["int8"])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.plc_pred_form(2)
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_pred_form() == 1 and b.plc_pred_form(0) == 1                            # the table at three streams
    big = b.plc_pred_form(n_streams=1 << 20)
    assert big == api.plc_pred_form_table(1 << 20, 256, 128, 256, 256, True)             # (an MI355X has 256 compute units)
    for S in (1, 2, 4, 8):
        assert b.plc_pred_form(S) == S and b.plc_pred_form(n_streams=5000) == S
    for S in (-1, 3, 16):
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*1, 2, 4 or 8"):
            b.plc_pred_form(S)
    assert b.plc_pred_form() == 8                                                        # (a refused value changes nothing)
    assert b.plc_pred_form(0) == 1
    b.close()
