"""GPU tests of the slot start and close of the two-group sample kernel (lpcnet_amd/csrc/sample_kernel_x2.hip.h, slot_plan.h; round 10) and of the
stage-2 pass on a chain wave: the benchmark model under FORCED dealings that give its waves every slot shape the plan distinguishes -- a chain wave
without a slot, with a candidate slot alone, with a candidate and two update / reset slots, a row wave whose only slot runs in its head, the
stage-2 host (LPCN_X2_S2W, chain wave 1) with and without items -- and five other models on their own dealing.  Three of those have a two-group
image with other shapes and other kernel variants (22 items per lane: chain waves with one slot, a leader with nothing but its head; 30 items: a
leader with update / reset slots behind its parked slot, a chain wave with a candidate slot alone; 32 items).  The other two -- densities 0.07 /
0.07 / 0.25 and skew 0.1, the models of `bench.py --densities` / `--skew` -- need more than 32 items per lane: the packer builds no two-group image
for them and the engine runs them on the kernel it chooses itself, as `bench.py` does; their cases check that what it chooses is bit-exact and that
a request for eight streams per workgroup is refused, not served by another kernel under that name.  Every case is compared with the plain-C oracle
bit for bit: PCM, GRU states, LPC history, last excitation, de-emphasis memory, frame count and RNG words, over 13 streams (one full workgroup and
one of 4 + 1), 2 frames and a continued call of 1 frame.

Every forced map is first given to the packer on the host (tests/tools/deal_print.py): a map it ignores, or one that does not produce the shape the
case is named after, fails the case before anything runs on the GPU; so does a model that is expected to have a two-group image and has none.
Round 10's search over the update / reset slots (tools/deal_search.py --x2 --keep-candidates) found no faster map than the model's own: there is no
adopted map to add to the list.

Every case is one GPU step: a child process of its own -- the dealing is read from the environment when the model is packed -- under its own time
limit.  A child that ends on a signal or runs into its limit marks the module: the cases behind it fail without starting anything on the GPU, and
nothing is run a second time."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_WAVE = 1                                                # LPCN_X2_S2W

# slot i of the forced map (candidate slots first, both kinds by descending length) goes to wave MAP[i]; the benchmark model's slots are
# c30 c22 c21 c19 c18 c15 | 12 8 7 6 5 5 5 4 3 3 3 2
OWN = [4, 7, 6, 5, 2, 3, 1, 0, 5, 6, 7, 0, 3, 5, 7, 6, 1, 2]


def moved(**to):
    m = list(OWN)
    for i, w in to.items():
        m[int(i[1:])] = w
    return ",".join(str(w) for w in m)


# name: (forced map, {wave: (bounds b1 b2 b3, head, slots with rows, slots with candidate rows)} the packer must answer with)
CASES = {
    "own_map":                        (moved(), {0: ((8, 13, 13), 0, 3, 0), HOST_WAVE: ((12, 15, 15), 0, 3, 0), 2: ((18, 20, 20), 0, 3, 1), 4: ((6, 6, 6), 24, 1, 1), 7: ((0, 5, 8), 22, 7, 1)}),
    "chain_wave_without_a_slot":      (moved(s7=1, s11=2), {0: ((0, 0, 0), 0, 0, 0), 1: ((12, 20, 23), 0, 7, 0)}),
    "chain_wave_candidate_and_two":   (moved(s11=2), {2: ((18, 23, 25), 0, 7, 1), 0: ((8, 8, 8), 0, 1, 0)}),
    "chain_wave_candidate_alone":     (moved(s17=1), {2: ((18, 18, 18), 0, 1, 1), 1: ((12, 15, 17), 0, 7, 0)}),
    "row_wave_head_and_nothing_else": (moved(s10=0, s14=1), {7: ((0, 0, 0), 22, 1, 1), 0: ((8, 13, 18), 0, 7, 0)}),
    "host_wave_without_items":        (moved(s6=0, s16=2), {HOST_WAVE: ((0, 0, 0), 0, 0, 0), 0: ((12, 20, 25), 0, 7, 0)}),
}
# name: (model, items per lane of its two-group image -- 0: it has none --, {wave: shape} as above)
MODELS = {
    "sparse_22_items":     (dict(densities=(0.03, 0.03, 0.12)), 22, {0: ((5, 5, 5), 0, 1, 0), 4: ((0, 4, 5), 17, 7, 1), 2: ((11, 13, 13), 0, 3, 1)}),
    "mid_30_items":        (dict(densities=(0.045, 0.045, 0.18)), 30, {4: ((2, 6, 6), 24, 3, 1), 2: ((16, 16, 16), 0, 1, 1), 7: ((0, 5, 9), 17, 7, 1)}),
    "seed5_32_items":      (dict(seed=5), 32, {4: ((8, 8, 8), 24, 1, 1), HOST_WAVE: ((10, 13, 13), 0, 3, 0)}),
    "sparse_update_reset": (dict(densities=(0.07, 0.07, 0.25)), 0, {}),
    "skewed":              (dict(skew=0.1), 0, {}),
}

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- the case (run in the child)
def case_parity(model_kw, two_group):
    from lpcnet_amd import api, synth
    from oracle import orc
    n, T1, T2 = 13, 2, 1
    blob = synth.blob_bytes(synth.make_model(**eval(model_kw)))
    om = orc.OracleModel(blob)
    sts = [om.new_state() for _ in range(n)]
    b = api.LPCNetBatch(n, blob)
    if int(two_group):
        b.streams_per_workgroup = 8
        assert b.streams_per_workgroup == 8
    else:                                                    # no two-group image: the request is an error and the engine's own choice stands
        with pytest.raises(api.LPCNetError):
            b.streams_per_workgroup = 8
        assert b.streams_per_workgroup != 8
    for seed, T in ((9700, T1), (9800, T2)):
        feats = np.stack([synth.make_features(seed + s, T) for s in range(n)])
        got = b.synthesize(feats)
        assert np.array_equal(got, np.stack([sts[s].synthesize(feats[s]) for s in range(n)]))
        for s in range(n):
            st = b.get_state(s)
            c1, c2, ga, gb = sts[s].nnet_state()
            ls, le, dm, fc, rng = sts[s].signal_state()
            assert np.array_equal(np.array(st.gru_a, np.float32), ga) and np.array_equal(np.array(st.gru_b, np.float32), gb), s
            assert np.array_equal(np.array(st.last_sig, np.float32), ls) and st.last_exc == le and st.frame_count == fc, s
            assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s
    assert np.any(got != 0)                                  # (the continued call is past the start-up frames)
    b.close()


# ---------------------------------------------------------------------------------------------------------- the parent
_faulted = []      # the first step that ended on a signal or a time limit


def run_step(model_kw, force=None, two_group=1, limit=300):
    assert not _faulted, "not started: GPU step %s ended abnormally before this one" % _faulted[0]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LPCN_DEAL")}
    if force:
        env["LPCN_DEAL_FORCE_X2"] = force
    cmd = [sys.executable, os.path.abspath(__file__), repr(model_kw), str(two_group)]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _faulted.append("%s %s (time limit of %d s)" % (model_kw, force, limit))
        pytest.fail("GPU step ran into its time limit: %s\n%s" % (_faulted[0], e.stdout or ""))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _faulted.append("%s %s (exit status %d)" % (model_kw, force, r.returncode))
    assert r.returncode == 0, "exit status %d\n%s" % (r.returncode, r.stdout[-4000:])
    assert "LPCN_DEAL_FORCE ignored" not in r.stdout


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    """the packer on the host: (items per lane of the two-group image or 0, {wave: (bounds, head, live, cand)}) of a model, under a forced map or its own"""
    from lpcnet_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import deal_print
    run = deal_print.build(tmp_path_factory.mktemp("deal_print"))

    def shapes(model_kw, force=None):
        have, nw, waves, maps, err = run(synth.blob_bytes(synth.make_model(**model_kw)), force)
        assert "ignored" not in err, err
        if force:
            assert have and [int(t.split(":")[1]) for t in maps[-1].split()] == [int(w) for w in force.split(",")]      # (the last map printed is the two-group image's)
        return (nw if have else 0), {w: (d["bounds"], d["head"], d["live"], d["cand"]) for w, d in waves.items()}
    return shapes


@pytest.mark.parametrize("name", list(CASES))
def test_forced_dealing(name, packer, hip_lib):
    force, shapes = CASES[name]
    nw, waves = packer({}, force)
    assert nw == 30
    for w, shape in shapes.items():
        assert waves[w] == shape, (w, waves[w])
    run_step({}, force)


@pytest.mark.parametrize("name", list(MODELS))
def test_other_models_on_their_own_dealing(name, packer, hip_lib):
    model_kw, items, shapes = MODELS[name]
    nw, waves = packer(model_kw)
    assert nw == items
    for w, shape in shapes.items():
        assert waves[w] == shape, (w, waves[w])
    run_step(model_kw, two_group=1 if items else 0)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    case_parity(sys.argv[1], sys.argv[2])
    print("ok")
