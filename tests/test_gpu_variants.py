"""LPC_GAMMA and END2END -- compile-time variants of the reference, run-time switches of a batch (lpcnet_batch_set_lpc_gamma,
lpcnet_batch_set_end2end) -- on every path that runs the frame network: the one-frame kernel in each tile size and its hand-over of the LPC delay
line to the chunk kernel and back, every form of the sample kernel, int8, per-stream steps on the kept products, teacher forcing, the codec path,
the batched PLC, shards, the active prefix, moved streams, a captured step, and the setters themselves.

Two references, tolerance 0 on samples and bit patterns throughout (the parity contract):
  * the reference's own variant builds, through tests/golden/golden_variants_v1.npz (tests/tools/make_golden_variants.py: flavours gg = LPC_GAMMA
    0.9, ge = END2END, gx = END2END with LPC_GAMMA 0.95);
  * the plain-C oracle with the same parameters (pinned to those builds by tests/test_oracle.py), where frame products and states are compared.
Every expected array is checked to differ from the plain model's, to be audible and to hold no sample at +-32767 (expected_ok): END2END with
gamma 1 is an unstable filter on the synthetic model, and SEEDS are streams on which it stays inside the range for twelve frames."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import make_golden_variants as mgv  # noqa: E402
import plc_synth  # noqa: E402
from plc_run import run as plc_run  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402
from oracle import orc  # noqa: E402

pytestmark = pytest.mark.gpu

V = {"gamma0.9": (0.9, False), "e2e-gamma0.95": (0.95, True), "e2e-gamma1": (1.0, True)}
FLAVOUR_OF = {"gg": "gamma0.9", "gx": "e2e-gamma0.95", "ge": "e2e-gamma1"}
# END2END with gamma 1 stays below full scale for twelve frames on these (found with the oracle; expected_ok asserts it of every array used)
SEEDS = (8200, 8202, 8203, 8205, 8208, 8221, 8233, 8237, 8247, 8258, 8259, 8201, 8204)
T7 = 7
PATTERNS = {"one-call": (7,), "frame-by-frame": (1,) * 7, "1-2-1-3": (1, 2, 1, 3), "2-1-3-1": (2, 1, 3, 1)}


def f32(x):
    return np.array(x, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def feats_for(seeds, T):
    return np.stack([synth.make_features(s, 60)[:T] for s in seeds])


def apply(b, v):
    gamma, e2e = V[v]
    if e2e:
        b.set_end2end(True)
    b.set_lpc_gamma(gamma)
    return b


def expected_ok(want, plain):
    """an expected PCM array [n][T * 160] is worth comparing with: not the plain model's, audible after the start-up frames, nowhere on the rails"""
    assert want.shape == plain.shape
    for s in range(want.shape[0]):
        assert not np.array_equal(want[s], plain[s]), s
        assert not want[s, :320].any() and (want[s, 320:] != 0).mean() > 0.5, s
    assert np.abs(want.astype(np.int32)).max() < 32767


_cache = {}


def oracle(blob, v, n, T, key="f32"):
    """the oracle on the first n SEEDS for T frames under variant v (None = the plain model): dict(pcm, ca, cb, lp, states), computed once"""
    k = (key, v, n, T)
    if k not in _cache:
        gamma, e2e = V[v] if v else (1.0, False)
        om = orc.OracleModel(blob, lpc_gamma=gamma, end2end=e2e)
        feats = feats_for(SEEDS[:n], T)
        pcm = np.zeros((n, T * 160), np.int16)
        ca, cb, lp = np.zeros((n, T, 1152), np.float32), np.zeros((n, T, 48), np.float32), np.zeros((n, T, 16), np.float32)
        states = []
        for s in range(n):
            st = om.new_state()
            for t in range(T):
                st.L.orc_synthesize(st.p, np.ascontiguousarray(feats[s, t, :20]), pcm[s, t * 160:(t + 1) * 160], 160, 0)
                lp[s, t], ca[s, t], cb[s, t] = st.frame_products()
            states.append(st)
        for a in (pcm, ca, cb, lp):
            a.setflags(write=False)
        _cache[k] = dict(pcm=pcm, ca=ca, cb=cb, lp=lp, states=states, om=om, feats=feats)
        if v:
            expected_ok(pcm, oracle(blob, None, n, T, key)["pcm"])
    return _cache[k]


def check_frame_state(b, s, o, e2e):
    """what the frame kernels keep per stream: conv memories, frame_count, the LPC delay line as stored (unweighted; left alone under END2END)"""
    st = b.get_state(s)
    c1, c2, _, _ = o.nnet_state()
    assert np.array_equal(bits(f32(st.conv1_mem)), bits(c1)) and np.array_equal(bits(f32(st.conv2_mem)), bits(c2)), s
    assert st.frame_count == o.signal_state()[3], s
    old = f32(st.old_lpc).reshape(2, 16)
    if e2e:
        assert not old.any(), s
    else:
        assert np.array_equal(bits(old), bits(o.old_lpc())) and old.any(), s


def check_sample_state(b, s, o):
    st = b.get_state(s)
    _, _, ga, gb = o.nnet_state()
    ls, le, dm, fc, rng = o.signal_state()
    assert np.array_equal(bits(f32(st.gru_a)), bits(ga)) and np.array_equal(bits(f32(st.gru_b)), bits(gb)), s
    assert np.array_equal(bits(f32(st.last_sig)), bits(ls)) and st.last_exc == le and st.frame_count == fc, s
    assert np.float32(st.deemph_mem) == np.float32(dm) and np.array_equal(np.array(st.rng, np.uint32), rng), s


@pytest.fixture(scope="module")
def gold():
    return np.load(mgv.PATH)


# ------------------------------------------------------------------ 1. every tile of the one-frame path; the delay line between the two cond kernels
@pytest.mark.parametrize("v", list(V))
@pytest.mark.parametrize("n", [1, 2, 3, 5, 9])
def test_one_frame_tiles_and_the_hand_over_between_the_cond_kernels(n, v, blob_f32, hip_lib):
    """frame_cond_t1_kernel<1 / 2 / 4 / 8> (n = 9: a full tile and one of a single stream) has its own delay-line shift and gamma chain; old_lpc is
    stored unweighted and weighted when consumed, by either cond kernel (the chunk kernel also with n_frames == 2, where it consumes both rows and
    shifts none).  Products and PCM against the oracle in four call patterns; afterwards the stored state is the oracle's."""
    e2e = V[v][1]
    w = oracle(blob_f32, v, 9, T7)
    feats = w["feats"][:n]
    if e2e:
        assert w["lp"][:n, :2].any(axis=2).all()                # rc2lpc's coefficients from the first frame on, no two-frame delay
    else:
        assert not w["lp"][:n, :2].any() and w["lp"][:n, 2:].any(axis=2).all()
    b = apply(api.LPCNetBatch(n, blob_f32), v)
    for name, lens in PATTERNS.items():
        edges = np.concatenate([[0], np.cumsum(lens)])
        b.reset()
        got = np.concatenate([b.synthesize(np.ascontiguousarray(feats[:, a:z])) for a, z in zip(edges[:-1], edges[1:])], axis=1)
        bad = np.argwhere(got != w["pcm"][:n])
        assert bad.size == 0, (name, bad[:4].tolist())
        for s in range(n):
            check_frame_state(b, s, w["states"][s], e2e)
            check_sample_state(b, s, w["states"][s])
        b.reset()
        parts = [b.run_frames(np.ascontiguousarray(feats[:, a:z])) for a, z in zip(edges[:-1], edges[1:])]
        ca, cb, lp = (np.concatenate([p[k] for p in parts], axis=1) for k in range(3))
        assert np.array_equal(bits(lp), bits(w["lp"][:n])), (name, np.argwhere(bits(lp) != bits(w["lp"][:n]))[:4].tolist())
        assert np.array_equal(bits(ca), bits(w["ca"][:n])) and np.array_equal(bits(cb), bits(w["cb"][:n])), name
        for s in range(n):
            check_frame_state(b, s, w["states"][s], e2e)
    b.close()


# ------------------------------------------------------------------ 2. the reference's own variant builds
@pytest.mark.parametrize("fl", mgv.FLAVOURS)
def test_reference_fixture(fl, gold, blob_f32, hip_lib):
    assert mgv.crc(np.frombuffer(blob_f32, np.uint8)) == gold["blob_crc"] and tuple(gold["seeds"]) == mgv.SEEDS and int(gold["n_frames"]) == mgv.T
    feats = np.stack([mgv.features(s) for s in mgv.SEEDS])
    assert [mgv.crc(f) for f in feats] == gold["feat_crc"].tolist()
    want = np.stack([gold[f"pcm_{fl}_{s}"] for s in mgv.SEEDS])
    plain = oracle(blob_f32, None, 3, mgv.T)                     # (SEEDS[:3] are the fixture's seeds)
    assert SEEDS[:3] == mgv.SEEDS
    expected_ok(want, plain["pcm"])
    assert np.array_equal(want, oracle(blob_f32, FLAVOUR_OF[fl], 3, mgv.T)["pcm"])      # (the oracle agrees with the build it is pinned to)
    for k, seed in enumerate(mgv.SEEDS):                         # alone, frame by frame
        b = apply(api.LPCNetBatch(1, blob_f32), FLAVOUR_OF[fl])
        got = np.concatenate([b.synthesize(feats[k:k + 1, t:t + 1]) for t in range(mgv.T)], axis=1)
        assert np.array_equal(got[0], want[k]), (seed, np.argwhere(got[0] != want[k])[:4].tolist())
        st = b.get_state(0)
        assert np.array_equal(bits(f32(st.gru_a)), bits(gold[f"gru_a_{fl}_{seed}"])) and np.array_equal(bits(f32(st.gru_b)), bits(gold[f"gru_b_{fl}_{seed}"]))
        b.close()
    slots = (1, 4, 8)                                            # together, among nine, in one call
    nine = feats_for(SEEDS[3:12], mgv.T)
    nine[list(slots)] = feats
    b = apply(api.LPCNetBatch(9, blob_f32), FLAVOUR_OF[fl])
    got = b.synthesize(nine)
    for k, (slot, seed) in enumerate(zip(slots, mgv.SEEDS)):
        assert np.array_equal(got[slot], want[k]), (slot, seed)
        st = b.get_state(slot)
        assert np.array_equal(bits(f32(st.gru_a)), bits(gold[f"gru_a_{fl}_{seed}"])) and np.array_equal(bits(f32(st.gru_b)), bits(gold[f"gru_b_{fl}_{seed}"]))
    b.close()


# ------------------------------------------------------------------ 3. every form of the sample kernel, and int8
FORMS = {"S1": (1, 0), "S2": (2, 0), "S4": (4, 0), "S8": (8, 0), "12waves": (8, 1)}


@pytest.mark.parametrize("v", ["gamma0.9", "e2e-gamma0.95"])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_of_the_sample_kernel(form, v, blob_f32, hip_lib):
    """13 streams (three workgroups of four, two of eight with five dead rows), the start-up frames and four more: every consumer of d_lpc"""
    n, T = 13, 6
    w = oracle(blob_f32, v, n, T)
    S, twelve = FORMS[form]
    b = apply(api.LPCNetBatch(n, blob_f32), v)
    b.streams_per_workgroup = S
    if S == 8:
        b.twelve_waves = twelve
    assert b.streams_per_workgroup == S and b.twelve_waves == twelve
    got = b.synthesize(w["feats"])
    bad = np.argwhere(got != w["pcm"])
    assert bad.size == 0, bad[:4].tolist()
    for s in range(n):
        check_sample_state(b, s, w["states"][s])
    assert b.streams_per_workgroup == S and b.twelve_waves == twelve
    b.close()


def test_int8_blob_with_lpc_gamma(blob_i8, hip_lib):
    n, T = 13, 6
    w = oracle(blob_i8, "gamma0.9", n, T, key="i8")
    b = apply(api.LPCNetBatch(n, blob_i8), "gamma0.9")
    b.streams_per_workgroup = 4
    got = np.concatenate([b.synthesize(np.ascontiguousarray(w["feats"][:, :1])), b.synthesize(np.ascontiguousarray(w["feats"][:, 1:]))], axis=1)
    assert np.array_equal(got, w["pcm"]), np.argwhere(got != w["pcm"])[:4].tolist()
    for s in range(n):
        check_sample_state(b, s, w["states"][s])
    b.close()


# ------------------------------------------------------------------ 4. per-stream step arguments, kept products, teacher forcing
@pytest.mark.parametrize("v", ["gamma0.9", "e2e-gamma0.95"])
def test_per_stream_steps_on_the_kept_products(v, blob_f32, hip_lib):
    """the scenario of test_batch_step_with_per_stream_arguments_like_a_batched_plc (tests/test_gpu_parity.py) under a variant: frame steps (one-frame
    kernel on a compacted group), tail-only steps on d_keep_lpc, per-stream n_samples and preload, against the oracle driven alone with the same calls"""
    rng = np.random.default_rng(7)
    n, calls = 7, 9
    gamma, e2e = V[v]
    om, plain = orc.OracleModel(blob_f32, lpc_gamma=gamma, end2end=e2e), orc.OracleModel(blob_f32)
    ost, pst = [om.new_state() for _ in range(n)], [plain.new_state() for _ in range(n)]
    b = apply(api.LPCNetBatch(n, blob_f32), v)
    had_frame = [False] * n
    differs = tails = 0
    for c in range(calls):
        feats = np.stack([synth.make_features(SEEDS[s] + 31 * c, 1)[0] for s in range(n)])
        pcm_in = rng.integers(-300, 300, size=(n, 160)).astype(np.int16)      # (imposed noise of +-3000 drives END2END with 0.95 to the rails in 1.3 % of the free samples)
        mode = rng.integers(0, 3, size=n)
        if c < 3:
            mode[:] = 1                                      # start-up frames for everybody
        mode = np.where((mode == 2) & ~np.array(had_frame), 1, mode)
        ns = rng.choice([160, 120, 40, 1, 77], size=n)
        pre = np.array([int(rng.integers(0, k + 1)) if rng.random() < 0.6 else 0 for k in ns])
        want, other = pcm_in.copy(), pcm_in.copy()
        for s in range(n):
            for sts, out in ((ost, want), (pst, other)):
                if mode[s] == 1:
                    sts[s].L.orc_synthesize(sts[s].p, np.ascontiguousarray(feats[s, :20]), out[s], int(ns[s]), int(pre[s]))
                elif mode[s] == 2:
                    lpc, ca, cb = sts[s].frame_products()
                    sts[s].L.orc_synthesize_tail(sts[s].p, ca, cb, lpc, out[s], int(ns[s]), int(pre[s]))
            had_frame[s] |= mode[s] == 1
        got = b.synthesize_step(feats, pcm_in, ns, pre, mode)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (c, bad[:4].tolist(), mode.tolist(), ns.tolist(), pre.tolist())
        assert np.abs(want.astype(np.int32)).max() < 32767
        differs += int((want != other).sum())
        tails += int((mode == 2).sum())
    assert tails >= 5 and differs > 1000                     # (tail-only steps were run; the plain model gives other samples for the same calls)
    for s in range(n):
        check_sample_state(b, s, ost[s])
        check_frame_state(b, s, ost[s], e2e)
    b.close()


@pytest.mark.parametrize("v", list(V))
def test_teacher_forcing(v, blob_f32, golden, hip_lib):
    """synthesize(..., preload_pcm): 80 imposed samples per frame, the rest sampled through the variant's filter"""
    n, T = 3, 6
    gamma, e2e = V[v]
    om = orc.OracleModel(blob_f32, lpc_gamma=gamma, end2end=e2e)
    feats = feats_for(SEEDS[:n], T)
    forced = np.zeros((n, T * 160), np.int16)
    for t in range(T):
        forced[:, t * 160:t * 160 + 80] = golden["forced_pcm_in"][t * 160:t * 160 + 80]
    want, plain = forced.copy(), forced.copy()
    states = []
    for m, out in ((om, want), (orc.OracleModel(blob_f32), plain)):
        for s in range(n):
            st = m.new_state()
            for t in range(T):
                st.L.orc_synthesize(st.p, np.ascontiguousarray(feats[s, t, :20]), out[s, t * 160:(t + 1) * 160], 160, 80)
            states.append(st)
    expected_ok(want, plain)
    b = apply(api.LPCNetBatch(n, blob_f32), v)
    got = np.concatenate([b.synthesize(feats[:, :1], preload_pcm=forced[:, :160], preload=80),
                          b.synthesize(feats[:, 1:], preload_pcm=forced[:, 160:], preload=80)], axis=1)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    for s in range(n):
        check_sample_state(b, s, states[s])
    b.close()


# ------------------------------------------------------------------ 5. the batched PLC: one-frame steps and deferred frame networks only
@pytest.fixture(scope="module")
def plc_in(gold):
    blob = synth.blob_bytes(plc_synth.make_model_with_plc())
    pcm, lost = mgv.plc_pcm(), mgv.plc_lost()
    assert mgv.crc(np.frombuffer(blob, np.uint8)) == gold["plc_blob_crc"] and mgv.crc(pcm) == gold["plc_in_crc"] and mgv.crc(lost) == gold["plc_lost_crc"]
    assert (lost.sum(axis=1) == 7).all()
    return blob, pcm, lost


@pytest.mark.parametrize("k", range(len(mgv.PLC_OPTIONS)), ids=["causal", "codec"])
@pytest.mark.parametrize("fl", mgv.PLC_FLAVOURS)
def test_batched_plc_equals_the_reference(fl, k, gold, plc_in, hip_lib):
    blob, pcm, lost = plc_in
    want_crc, want_full = gold[f"plc_crc_{fl}"][k], gold[f"plc_full_{fl}"][k]
    other = gold["plc_full_gx" if fl == "gg" else "plc_full_gg"][k]
    assert not np.array_equal(want_full, other) and (want_full[lost[mgv.PLC_FULL_STREAM] != 0] != 0).mean() > 0.5      # the variants differ; concealment is not silence
    assert np.abs(want_full[lost[mgv.PLC_FULL_STREAM] != 0].astype(np.int32)).max() < 32767      # (of the concealed frames: received ones pass the input on)
    b = apply(api.LPCNetBatch(mgv.PLC_STREAMS, blob), FLAVOUR_OF[fl])
    b.plc_enable(mgv.PLC_OPTIONS[k])
    out = plc_run(b, pcm, lost)
    b.close()
    bad = np.argwhere(out[mgv.PLC_FULL_STREAM] != want_full)
    assert bad.size == 0, "first differing (frame, sample) %s of %d" % (bad[:4].tolist(), len(bad))
    assert np.array_equal(mgv.block_crc(out), want_crc), np.argwhere(mgv.block_crc(out) != want_crc).tolist()
    order = [3, 0, 4, 1, 2, 0, 3, 1]                             # the five among eight, on the two-group kernel
    b = apply(api.LPCNetBatch(8, blob), FLAVOUR_OF[fl])
    b.streams_per_workgroup = 8
    b.twelve_waves = 0
    b.plc_enable(mgv.PLC_OPTIONS[k])
    out = plc_run(b, pcm, lost, streams=order)
    assert b.streams_per_workgroup == 8 and b.twelve_waves == 0
    b.close()
    got = mgv.block_crc(out)
    for i, s in enumerate(order):
        assert np.array_equal(got[i], want_crc[s]), (i, s)
    assert np.array_equal(out[order.index(mgv.PLC_FULL_STREAM)], want_full)


# ------------------------------------------------------------------ 6. the codec path
def test_codec_path_under_lpc_gamma(gold, golden, blob_f32, hip_lib):
    import torch
    pk = golden["packets"]
    assert mgv.crc(pk) == gold["packets_crc"]
    want = gold["packet_pcm_gg"].reshape(-1)
    assert not np.array_equal(want, golden["packet_pcm_gf"].reshape(-1)) and (want[640:] != 0).mean() > 0.5 and np.abs(want.astype(np.int32)).max() < 32767
    api.set_codebooks(*synth.make_codebooks(mgv.CODEBOOK_SEED))
    b = apply(api.LPCNetBatch(2, blob_f32), "gamma0.9")
    two = np.stack([pk, pk])
    out = np.concatenate([b.decode(two[:, :1]), b.decode(two[:, 1:])], axis=1)      # a packet is four frames: the chunk kernel; state across calls
    for s in range(2):
        assert np.array_equal(out[s], want), np.argwhere(out[s] != want)[:4].tolist()
    b.reset()
    P = pk.shape[0]
    d_pk = torch.from_numpy(np.ascontiguousarray(two)).cuda()
    d_pcm = torch.zeros((2, P * 640), dtype=torch.int16, device="cuda")
    b.decode_device(d_pk.data_ptr(), d_pcm.data_ptr(), P, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_pcm.cpu().numpy(), np.stack([want, want]))
    b.close()


# ------------------------------------------------------------------ 7. what a variant must leave alone
def test_analysis_and_encoder_ignore_the_variants(blob_f32, hip_lib):
    """analysis and the encoder share lpc_from_cepstrum_wave with lpc_kernel; the reference's encoder never weights (src/lpcnet_enc.c:523,715)"""
    import make_golden_encode as mge
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_analysis_v1.npz"))
    ints = [k for k in range(len(g["seeds"])) if k != int(g["float_stream"])]
    T = 20
    pcm = np.stack([synth.make_pcm(int(g["seeds"][k]), g["features"].shape[1]) for k in ints])[:, :T * 160]
    b = api.LPCNetBatch(len(ints), blob_f32)
    b.set_end2end(True)
    b.set_lpc_gamma(0.9)
    out = b.analyze(pcm)
    want = g["features"][ints, :T]
    assert want[:, :, 20:].any() and np.array_equal(bits(out), bits(want)), (bits(out) != bits(want)).sum(axis=(0, 1)).tolist()
    b.close()
    e = np.load(mge.PATH)
    P = 3
    epcm = np.stack([synth.make_pcm(int(s), 4 * e["packets"].shape[1]) for s in e["seeds"]])
    assert [zlib.crc32(p.tobytes()) for p in epcm] == e["pcm_crc32"].tolist()
    api.set_codebooks(*synth.make_codebooks(int(e["codebook_seed"])))
    b = api.LPCNetBatch(epcm.shape[0], blob_f32)
    b.set_end2end(True)
    b.set_lpc_gamma(0.9)
    assert np.array_equal(b.encode(epcm[:, :640 * P]), e["packets"][:, :P])
    b.close()


# ------------------------------------------------------------------ 8. shards, prefix, moved streams
def test_the_setter_reaches_every_shard_and_a_prefix_is_a_smaller_batch(blob_f32, hip_lib):
    n, T = 9, 5
    w = oracle(blob_f32, "gamma0.9", 9, T7)
    feats, want = w["feats"][:, :T], w["pcm"][:, :T * 160]
    b = api.LPCNetBatch(n, blob_f32, devices=[0, 0])
    assert b.shards == [(0, 5, 0), (5, 4, 0)]
    b.set_lpc_gamma(0.9)                                          # one call: both engines
    got = np.concatenate([b.synthesize(np.ascontiguousarray(feats[:, :1])), b.synthesize(np.ascontiguousarray(feats[:, 1:]))], axis=1)
    assert np.array_equal(got, want), sorted(set(np.argwhere(got != want)[:, 0].tolist()))
    b.reset()
    b.active = [3, 3]                                             # six active: streams 0..2 and 5..7
    on, off = [0, 1, 2, 5, 6, 7], [3, 4, 8]
    before = [bytes(b.get_state(s)) for s in off]
    got = np.concatenate([b.synthesize(np.ascontiguousarray(feats[:, :1])), b.synthesize(np.ascontiguousarray(feats[:, 1:]))], axis=1)
    assert np.array_equal(got[on], want[on]) and not got[off].any()
    assert [bytes(b.get_state(s)) for s in off] == before
    b.close()


def test_a_moved_stream_carries_its_unweighted_delay_line(blob_f32, hip_lib):
    w = oracle(blob_f32, "gamma0.9", 9, T7)
    feats, want = w["feats"][:2], w["pcm"][:2]
    b = apply(api.LPCNetBatch(3, blob_f32), "gamma0.9")
    b.active = 2
    three = np.concatenate([feats, feats[:1]])
    head = np.concatenate([b.synthesize(np.ascontiguousarray(three[:, t:t + 1])) for t in range(3)], axis=1)
    assert np.array_equal(head[:2], want[:, :480]) and not head[2].any()
    b.copy_streams([1], [2])
    src, dst = b.get_state(1), b.get_state(2)
    assert bytes(src) == bytes(dst) and f32(dst.old_lpc).any()
    o = w["om"].new_state()
    o.synthesize(feats[1, :3])
    assert np.array_equal(bits(f32(dst.old_lpc).reshape(2, 16)), bits(o.old_lpc()))        # as the cepstrum gave them: the weighting is applied on consumption
    b.active = 3
    three[2] = feats[1]
    tail = np.concatenate([b.synthesize(np.ascontiguousarray(three[:, 3:4])), b.synthesize(np.ascontiguousarray(three[:, 4:]))], axis=1)
    assert np.array_equal(tail[:2], want[:, 480:]) and np.array_equal(tail[2], want[1, 480:])
    assert bytes(b.get_state(2)) == bytes(b.get_state(1))
    b.close()


# ------------------------------------------------------------------ 9. one captured step
def test_a_captured_one_frame_step_replays_under_lpc_gamma(blob_f32, hip_lib):
    """as test_a_step_captured_in_a_hip_graph_replays_bit_exactly (tests/test_gpu_parity.py): the step is one linear chain of kernels on one stream"""
    import torch
    n, T = 9, 4
    w = oracle(blob_f32, "gamma0.9", 9, T7)
    feats = w["feats"]
    eager = apply(api.LPCNetBatch(n, blob_f32), "gamma0.9")
    eager.streams_per_workgroup = 4
    want = np.concatenate([eager.synthesize(np.ascontiguousarray(feats[:, t:t + 1])) for t in range(T)], axis=1)
    eager.close()
    assert np.array_equal(want, w["pcm"][:, :T * 160])
    dev = torch.device("cuda:0")
    b = apply(api.LPCNetBatch(n, blob_f32), "gamma0.9")
    b.streams_per_workgroup = 4
    d_feat = torch.zeros((n, 36), dtype=torch.float32, device=dev)
    d_pcm = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(s):                                   # frame 0 eagerly (first launch: function attributes, code-object load)
        d_feat.copy_(torch.from_numpy(np.ascontiguousarray(feats[:, 0])))
        b.synthesize_device(d_feat.data_ptr(), 36, d_pcm.data_ptr(), 1, s.cuda_stream)
        s.synchronize()
        out.append(d_pcm.cpu().numpy().copy())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.synthesize_device(d_feat.data_ptr(), 36, d_pcm.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    for t in range(1, T):
        d_feat.copy_(torch.from_numpy(np.ascontiguousarray(feats[:, t])))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out.append(d_pcm.cpu().numpy().copy())
    got = np.concatenate(out, axis=1)
    assert np.array_equal(got, want)
    assert b.get_state(n - 1).frame_count == T
    del g
    b.close()


# ------------------------------------------------------------------ 10. the setters
def test_setter_semantics(blob_f32, hip_lib):
    n, T = 2, 5
    w, plain = oracle(blob_f32, "gamma0.9", 9, T7), oracle(blob_f32, None, 9, T7)
    feats, want = np.ascontiguousarray(w["feats"][:n, :T]), w["pcm"][:n, :T * 160]
    b = apply(api.LPCNetBatch(n, blob_f32), "gamma0.9")
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
            b.set_lpc_gamma(bad)
    assert np.array_equal(b.synthesize(feats), want)             # a refused value leaves the batch at 0.9
    # a new model means new engines: both switches are back at their defaults
    b.set_end2end(True)
    assert b.L.lpcnet_batch_load_model(b.p, blob_f32, len(blob_f32)) == 0
    got = b.synthesize(feats)
    assert np.array_equal(got, plain["pcm"][:n, :T * 160]) and not np.array_equal(got, want)
    apply(b, "e2e-gamma0.95")                                    # ... and can be set again
    b.reset()
    assert np.array_equal(b.synthesize(feats), oracle(blob_f32, "e2e-gamma0.95", 9, T7)["pcm"][:n, :T * 160])
    b.set_end2end(False)                                         # END2END off again: the cepstral LPC and its delay line are back
    b.set_lpc_gamma(0.9)
    b.reset()
    assert np.array_equal(b.synthesize(feats), want)
    b.close()
    L = api.load_library()
    p = L.lpcnet_batch_create(2, 0)                              # no model yet
    assert p
    assert L.lpcnet_batch_set_lpc_gamma(p, 0.9) == -5 and L.lpcnet_batch_set_end2end(p, 1) == -5
    L.lpcnet_batch_destroy(p)


# ------------------------------------------------------------------ 11. the fixture as a whole is worth comparing with
def test_every_fixture_array_is_non_degenerate(gold, blob_f32, hip_lib):
    plain = oracle(blob_f32, None, 3, mgv.T)["pcm"]
    for fl in mgv.FLAVOURS:
        want = np.stack([gold[f"pcm_{fl}_{s}"] for s in mgv.SEEDS])
        expected_ok(want, plain)
        for other in mgv.FLAVOURS:
            assert other == fl or not np.array_equal(want, np.stack([gold[f"pcm_{other}_{s}"] for s in mgv.SEEDS]))
        for s in mgv.SEEDS:
            assert gold[f"gru_a_{fl}_{s}"].any() and gold[f"gru_b_{fl}_{s}"].any()
    assert not gold["rail_share"].any() and gold["max_abs"].max() < 32767
    for fl in mgv.PLC_FLAVOURS:
        crc = gold[f"plc_crc_{fl}"]
        assert all(len(set(c.reshape(-1).tolist())) == c.size for c in crc) and not np.array_equal(crc[0], crc[1])
        concealed = gold[f"plc_full_{fl}"][:, mgv.plc_lost()[mgv.PLC_FULL_STREAM] != 0]      # (received frames pass the input on, full-scale passages included)
        assert np.abs(concealed.astype(np.int32)).max() < 32767 and (concealed != 0).mean() > 0.5
    assert not np.array_equal(gold["plc_crc_gg"], gold["plc_crc_gx"])
