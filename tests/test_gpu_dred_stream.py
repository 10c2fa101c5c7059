"""The DRED decoder as a per-stream state on the device (lpcnet_batch_dred_state_enable, dred_init, dred_step: DRED_rdovae_dec_init_states and
DRED_rdovae_decode_qframe on a record the batch keeps per stream) against what the reference wrote: every cut of a latent chain reproduces
DRED_rdovae_decode_all's features (tests/golden/golden_dred_v1.npz, golden_dred_i8_v1.npz), the record equals the reference's RDOVAEDecState after
init_states and after every latent (tests/golden/golden_dred_state_v1.npz, made by tests/tools/make_golden_dred_state.py), FAST equals the same
batch's own dred_decode, and the record travels with its stream.  All comparisons on bit patterns."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_i8_model as di  # noqa: E402
import dred_model as dm  # noqa: E402
import make_golden_dred_fast as mf  # noqa: E402
import plc_model as pm  # noqa: E402
from lpcnet_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

N, ML = dm.N_STREAMS, dm.N_LATENTS
SENTINEL = np.float32(-12345.678)
FORMS = (0, 1, 2, 4, 8)          # nine streams: a full workgroup and one stream at 8, two full and one at 4; 0 = the table's form
NT = mf.TILE_STREAMS


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def fresh(n=N, ml=ML):
    return np.full((n, 4 * ml, 20), SENTINEL, np.float32)


# ---- schedules: lists of (start [n], count [n]) whose ranges are consecutive and partition [0, count[s]) for every stream
def one_by_one(count, ml=ML):
    return [(np.minimum(l, count).astype(np.int32), (count > l).astype(np.int32)) for l in range(ml)]


def three_cuts(count):
    out = []
    for a, b in ((0, 3), (3, 4), (4, 7)):
        lo, hi = np.minimum(a, count), np.minimum(b, count)
        out.append((lo.astype(np.int32), (hi - lo).astype(np.int32)))
    return out


def ragged(count):
    """stream s advances min(remaining, 1 + s % 3) per call: the counts differ inside every workgroup of every form"""
    done, out = np.zeros_like(count), []
    while (done < count).any():
        adv = np.minimum(count - done, 1 + np.arange(count.size) % 3).astype(np.int32)
        out.append((done.astype(np.int32), adv))
        done = done + adv
    return out


SCHEDULES = {"one latent per call": one_by_one, "cuts 0-3-4-7": three_cuts, "ragged": ragged}


def run(b, state, latents, sched, out, which=None):
    b.dred_init(state, which)
    for start, cnt in sched:
        b.dred_step(latents, start, cnt, out)
    return out


def assert_decoded(got, want, count, what=""):
    """rows below 4 count[s] equal the reference's, the others still hold the sentinel"""
    for s in range(got.shape[0]):
        k = 4 * int(count[s])
        assert np.array_equal(bits(got[s, :k]), bits(want[s, :k])), (what, s, np.argwhere(bits(got[s, :k]) != bits(want[s, :k]))[:4].tolist())
        assert (bits(got[s, k:]) == bits(SENTINEL)).all(), (what, s, "rows past the count were written")


@pytest.fixture(scope="module")
def gold(hip_lib):
    return {"f": np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_v1.npz")), "i": np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_i8_v1.npz"))}


@pytest.fixture(scope="module")
def gold_state():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_state_v1.npz"))


@pytest.fixture(scope="module")
def cases(gold):
    """per flavour and width set: the blob, the inputs and the reference's features, made once and left unchanged"""
    out = {}
    for fl in ("f", "i"):
        for name in dm.SETS:
            blob = dm.set_blob(name) if fl == "f" else di.blob_dec(name)
            state, latents = dm.set_inputs(name)
            assert np.uint32(zlib.crc32(blob)) == gold[fl]["blob_crc_" + name] and np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold[fl]["in_crc_" + name]
            out[fl, name] = (blob, state, latents, gold[fl]["feat_" + name])
    return out


@pytest.fixture(scope="module")
def batches(cases):
    """one nine-stream batch per flavour and width set, shared by the tests that leave it as they found it (form 0, every stream active)"""
    made = {}

    def get(fl, name):
        if (fl, name) not in made:
            b = api.LPCNetBatch(N, cases[fl, name][0])
            b.dred_enable(ML)
            b.dred_state_enable()
            made[fl, name] = b
        return made[fl, name]
    yield get
    for b in made.values():
        b.close()


# ------------------------------------------------------------------------------------------------------------------ every cut is decode_all
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(dm.SETS))
@pytest.mark.parametrize("fl", ["f", "i"])
def test_every_cut_is_decode_all(fl, name, form, cases, batches):
    _, state, latents, want = cases[fl, name]
    b = batches(fl, name)
    assert b.dred_flavour() == (fl == "i") and b.dred_form(form) == (form if form else 1)
    try:
        for what, make in SCHEDULES.items():
            sched = make(dm.COUNT)
            assert all((c >= 0).all() for _, c in sched) and (sum(c for _, c in sched) == dm.COUNT).all() and not any(c[2] for _, c in sched)
            got = run(b, state, latents, sched, fresh())
            assert_decoded(got, want, dm.COUNT, (fl, name, form, what))
    finally:
        b.dred_form(0)
    # (the ragged schedule's counts differ inside a workgroup of two)
    assert any(len(set(c[k:k + 2])) == 2 for _, c in ragged(dm.COUNT) for k in range(0, N - 1, 2))


@pytest.mark.parametrize("fl", ["f", "i"])
def test_a_long_chain_in_one_call_of_13_and_13_calls_of_one(fl, cases, gold):
    state, latents = dm.long_inputs()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold[fl]["long_in_crc"]
    b = api.LPCNetBatch(dm.LONG_STREAMS, cases[fl, "w256"][0])
    b.dred_enable(dm.LONG_LATENTS)
    b.dred_state_enable()
    c = dm.LONG_COUNT
    head = np.minimum(c, 13)
    sched = [(np.zeros_like(c), head)] + [(np.minimum(13 + l, c).astype(np.int32), (c > 13 + l).astype(np.int32)) for l in range(13)]
    got = run(b, state, latents, sched, fresh(dm.LONG_STREAMS, dm.LONG_LATENTS))
    b.close()
    s = dm.LONG_FULL_STREAM
    assert np.array_equal(bits(got[s]), bits(gold[fl]["long_full"]))
    assert dm.stream_crc(got, c).tolist() == gold[fl]["long_crc"].tolist()
    for s in range(dm.LONG_STREAMS):
        assert (bits(got[s, 4 * int(c[s]):]) == bits(SENTINEL)).all()


# ------------------------------------------------------------------------------------------------------------------ the record is the reference's
@pytest.mark.parametrize("fl,name", [("f", "small"), ("i", "small"), ("f", "mixed")])
def test_the_record_is_the_references_state(fl, name, cases, batches, gold_state):
    _, state, latents, want = cases[fl, name]
    ref = gold_state["state_%s_%s" % (fl, name)]
    assert gold_state["blob_crc_%s_%s" % (fl, name)] == np.uint32(zlib.crc32(cases[fl, name][0]))
    b = batches(fl, name)
    assert b.dred_dec_state_size() == ref.shape[2]
    records = lambda: np.stack([b.get_dred_dec_state(s) for s in range(N)])
    b.dred_init(state)
    assert np.array_equal(bits(records()), bits(ref[:, 0]))
    out = fresh()
    for l, (start, cnt) in enumerate(one_by_one(dm.COUNT)):
        b.dred_step(latents, start, cnt, out)
        at = np.minimum(l + 1, dm.COUNT)          # (a stream whose latents are through keeps the state after its own last one)
        assert np.array_equal(bits(records()), bits(ref[np.arange(N), at])), (fl, name, l)
    assert_decoded(out, want, dm.COUNT, (fl, name))
    # an init of some streams leaves the others' records alone; so does a step with a count of zero
    before = records()
    which = (np.arange(N) % 2).astype(np.int32)
    b.dred_init(state, which)
    after = records()
    assert np.array_equal(bits(after[which == 1]), bits(ref[which == 1, 0])) and np.array_equal(bits(after[which == 0]), bits(before[which == 0]))
    cnt = ((np.arange(N) % 3) == 1).astype(np.int32)
    out = fresh()
    b.dred_step(latents, np.zeros(N, np.int32), cnt, out)
    last = records()
    assert np.array_equal(bits(last[cnt == 0]), bits(after[cnt == 0])) and (bits(out[cnt == 0]) == bits(SENTINEL)).all()
    assert not any(np.array_equal(bits(last[s]), bits(after[s])) for s in np.nonzero(cnt)[0])


@pytest.mark.parametrize("fl", ["f", "i"])
def test_reset_is_init_decoder(fl, cases, batches, gold_state):
    _, state, latents, _ = cases[fl, "small"]
    zs, zf = gold_state["zero_state_%s_small" % fl], gold_state["zero_feat_%s_small" % fl]
    b = batches(fl, "small")
    b.dred_init(state)
    assert all(b.get_dred_dec_state(s).any() for s in range(N))
    b.reset(3, 2)                                  # a range: the others keep their records
    assert [bool(b.get_dred_dec_state(s).any()) for s in range(N)] == [s not in (3, 4) for s in range(N)]
    b.reset()
    assert not any(b.get_dred_dec_state(s).any() for s in range(N))
    out = fresh()
    for l in range(2):
        b.dred_step(latents, np.full(N, l, np.int32), np.ones(N, np.int32), out)
        assert np.array_equal(bits(np.stack([b.get_dred_dec_state(s) for s in range(N)])), bits(zs[:, l + 1])), l
    assert np.array_equal(bits(out[:, :8]), bits(zf)) and (bits(out[:, 8:]) == bits(SENTINEL)).all()


# ------------------------------------------------------------------------------------------------------------------ FAST
@pytest.fixture(scope="module")
def tile_case(hip_lib):
    """the 69-stream case on the small set and FAST's own one-shot output at T = 32: what init + steps must reproduce bit for bit in every tile"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_fast_v1.npz"))
    blob = dm.set_blob(mf.TILE_SET)
    state, latents = mf.tile_inputs()
    count = mf.tile_counts()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes() + count.tobytes())) == gold["tile_in_crc"]
    b = api.LPCNetBatch(NT, blob)
    b.dred_enable(ML)
    b.dred_fast = 32
    base = b.dred_decode(state, latents, count, fresh(NT))
    b.close()
    return blob, state, latents, count, base, gold


def fast_batch(blob, n, mode):
    b = api.LPCNetBatch(n, blob)
    b.dred_enable(ML)
    b.dred_state_enable()
    b.dred_fast = mode
    return b


@pytest.mark.parametrize("mode", [16, 32, 1])
def test_fast_steps_equal_the_batchs_own_decode(mode, tile_case):
    blob, state, latents, count, base, gold = tile_case
    b = fast_batch(blob, NT, mode)
    own = b.dred_decode(state, latents, count, fresh(NT))
    got = run(b, state, latents, ragged(count), fresh(NT))
    final = np.stack([b.get_dred_dec_state(s) for s in range(NT)])
    one = run(b, state, latents, one_by_one(count), fresh(NT))
    final_one = np.stack([b.get_dred_dec_state(s) for s in range(NT)])
    b.close()
    assert np.array_equal(bits(got), bits(own)) and np.array_equal(bits(one), bits(own))
    assert np.array_equal(bits(own), bits(base))          # the same bits at both tiles
    assert np.array_equal(bits(final), bits(final_one)) and np.isfinite(final).all()
    # ... and through that inside the envelope between the reference's generic-C and AVX2 builds
    for l in range(ML):
        live = count > l
        dev = float(np.abs(got[live, 4 * l:4 * l + 4].astype(np.float64) - gold["tile_gf"][live, 4 * l:4 * l + 4].astype(np.float64)).max())
        print("mode %d latent %d: deviation %.3g envelope %.3g" % (mode, l, dev, float(gold["tile_env"][l])))
        assert dev <= float(gold["tile_env"][l])


def test_fast_bits_do_not_depend_on_the_neighbours(tile_case):
    blob, state, latents, count, base, _ = tile_case
    pick = [3, 40, 68]
    b = fast_batch(blob, 3, 1)
    got = run(b, state[pick], latents[pick], ragged(count[pick]), fresh(3))
    rec3 = np.stack([b.get_dred_dec_state(s) for s in range(3)])
    b.close()
    assert count[pick].min() > 0 and np.array_equal(bits(got), bits(base[pick]))
    b = fast_batch(blob, NT, 1)
    got = run(b, state[::-1], latents[::-1], ragged(count[::-1]), fresh(NT))
    rec = np.stack([b.get_dred_dec_state(s) for s in range(NT)])[::-1]
    assert np.array_equal(bits(got[::-1]), bits(base)) and np.array_equal(bits(rec[pick]), bits(rec3))
    # the mode may change between calls: the record is the same floats.  PARITY finishes a chain FAST began, as the PARITY decoder would from that state
    b.dred_init(state[::-1])
    b.dred_fast = 0
    par = np.stack([b.get_dred_dec_state(s) for s in range(NT)])
    b.dred_fast = 16
    assert np.array_equal(bits(par), bits(np.stack([b.get_dred_dec_state(s) for s in range(NT)])))
    b.close()


def test_fast_nan_and_inf_latents_stay_in_their_stream(tile_case):
    blob, state, latents, count, base, _ = tile_case
    bad = 35                      # (inside the second tile of 32, a stream that decodes)
    lat, c = latents.copy(), count.copy()
    c[bad] = ML
    lat[bad, 0, ::2] = np.nan
    lat[bad, 1, 1::3] = np.inf
    lat[bad, 2, 5] = -np.inf
    b = fast_batch(blob, NT, 1)
    clean = run(b, state, latents, ragged(count), fresh(NT))
    rec_clean = np.stack([b.get_dred_dec_state(s) for s in range(NT)])
    got = run(b, state, lat, ragged(c), fresh(NT))
    rec = np.stack([b.get_dred_dec_state(s) for s in range(NT)])
    b.close()
    others = np.arange(NT) != bad
    assert np.array_equal(bits(clean), bits(base))
    assert np.array_equal(bits(got[others]), bits(base[others])) and np.array_equal(bits(rec[others]), bits(rec_clean[others]))
    assert not np.isfinite(got[bad, :4]).all() and not np.isfinite(rec[bad]).all()


# ------------------------------------------------------------------------------------------------------------------ a stream carries its decoder
def two_latents(count):
    return np.minimum(count, 2).astype(np.int32)


def finish(b, latents, count, rows, out):
    """the rest of every chain, latents 2 .. count - 1, on the streams `rows` of b (latents / out: b's own arrays)"""
    n = out.shape[0]
    start, cnt = np.zeros(n, np.int32), np.zeros(n, np.int32)
    start[rows], cnt[rows] = two_latents(count), count - two_latents(count)
    return b.dred_step(latents, start, cnt, out)


def widen(x, n, rows):
    out = np.zeros((n,) + x.shape[1:], x.dtype)
    out[rows] = x
    return out


def assert_finished(out, rows, want, count, what):
    """rows 8 .. 4 count - 1 of the moved streams are the fixture's; nothing else was written"""
    mask = np.zeros(out.shape[:2], bool)
    for k, r in enumerate(rows):
        lo, hi = 4 * int(two_latents(count)[k]), 4 * int(count[k])
        assert np.array_equal(bits(out[r, lo:hi]), bits(want[k, lo:hi])), (what, k)
        mask[r, lo:hi] = True
    assert (bits(out[~mask]) == bits(SENTINEL)).all(), what


@pytest.mark.parametrize("fl", ["f", "i"])
def test_a_stream_carries_its_decoder(fl, cases):
    blob, state, latents, want = cases[fl, "small"]
    S = api.SNAP
    C2, rows_a, rows_b = 2 * N, np.arange(N), N + np.arange(N)[::-1]          # (the copies land in reversed order)

    def begun(devices=None):
        """a batch of 18 whose streams 0 .. 8 stand after init + two latents"""
        b = api.LPCNetBatch(C2, blob, devices=devices)
        b.dred_enable(ML)
        b.dred_state_enable()
        b.dred_init(widen(state, C2, rows_a), (np.arange(C2) < N).astype(np.int32))
        b.dred_step(widen(latents, C2, rows_a), np.zeros(C2, np.int32), widen(two_latents(dm.COUNT), C2, rows_a), fresh(C2))
        return b

    # copy_streams to other slots, in one shard and across the two shards of devices=[0, 0]
    for devices in (None, [0, 0]):
        b = begun(devices)
        assert devices is None or [x[:2] for x in b.shards] == [(0, N), (N, N)]
        assert S["DRED_DEC"] in [x[0] for x in b.snapshot_layout()["sections"]]
        b.copy_streams(rows_a, rows_b)
        b.sync()
        out = finish(b, widen(latents, C2, rows_b), dm.COUNT, rows_b, fresh(C2))
        assert_finished(out, rows_b, want, dm.COUNT, ("copy_streams", devices))
        out = finish(b, widen(latents, C2, rows_a), dm.COUNT, rows_a, fresh(C2))          # (the sources still stand where they stood)
        assert_finished(out, rows_a, want, dm.COUNT, ("copy_streams, sources", devices))
        b.close()
    # snapshot -> restore into a batch of another capacity and shard layout; copy_streams_to; get / set into a fresh batch
    b = begun()
    snap = b.snapshot(rows_a)
    info = api.snapshot_info(snap)
    assert info["version"] == 1 and [x[0] for x in info["sections"]][-1] == S["DRED_DEC"] == 21
    C3, rows_c = 11, 1 + np.arange(N)
    for how in ("restore", "restore into a batch that has only dred_enable'd", "copy_streams_to", "get / set"):
        d = api.LPCNetBatch(C3, blob, devices=[0, 0])
        d.dred_enable(ML)
        if "only" not in how:
            d.dred_state_enable()
        if how.startswith("restore"):
            d.restore(rows_c, snap)
        elif how == "copy_streams_to":
            b.copy_streams_to(rows_a, d, rows_c)
            d.sync()
        else:
            for k in range(N):
                d.set_dred_dec_state(int(rows_c[k]), b.get_dred_dec_state(k))
        assert S["DRED_DEC"] in [x[0] for x in d.snapshot_layout()["sections"]]
        out = finish(d, widen(latents, C3, rows_c), dm.COUNT, rows_c, fresh(C3))
        assert_finished(out, rows_c, want, dm.COUNT, how)
        d.close()
    # a decoder of other widths: refused with the section named, nothing changed
    o = api.LPCNetBatch(N, cases[fl, "mixed"][0])
    o.dred_enable(ML)
    o.dred_state_enable()
    o.dred_init(cases[fl, "mixed"][1])
    before = [o.get_dred_dec_state(s) for s in range(N)]
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*section DRED_DEC"):
        o.restore(rows_a, snap)
    assert all(np.array_equal(bits(x), bits(o.get_dred_dec_state(s))) for s, x in enumerate(before))
    o.close()
    # a batch without the decoder cannot take the section; a batch that never enabled the record has no such section
    p = api.LPCNetBatch(N, blob)
    assert S["DRED_DEC"] not in [x[0] for x in p.snapshot_layout()["sections"]]
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*DRED_DEC"):
        p.restore(rows_a, snap)
    assert S["DRED_DEC"] not in [x[0] for x in p.snapshot_layout()["sections"]]
    p.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ forms of the call
def test_device_forms_shards_and_the_active_prefix(cases, batches):
    import torch
    _, state, latents, want = cases["f", "mixed"]
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state).to(dev), torch.from_numpy(latents).to(dev)
    b = batches("f", "mixed")
    sched = ragged(dm.COUNT)
    # on the batch's own stream, then on a caller's
    d_out = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.dred_init_device(d_state.data_ptr())
    for start, cnt in sched:
        b.dred_step_device(d_lat.data_ptr(), start, cnt, d_out.data_ptr())
    b.sync()
    assert_decoded(d_out.cpu().numpy(), want, dm.COUNT, "own stream")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_out2 = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
        b.dred_init_device(d_state.data_ptr(), np.ones(N, np.int32), hip_stream=st.cuda_stream)
        for start, cnt in sched:
            b.dred_step_device(d_lat.data_ptr(), start, cnt, d_out2.data_ptr(), hip_stream=st.cuda_stream)
        got = d_out2.cpu().numpy()
    assert_decoded(got, want, dm.COUNT, "caller's stream")
    # the host-array forms refuse a capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_init_device(d_state.data_ptr(), np.ones(N, np.int32), hip_stream=cs)
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_step_device(d_lat.data_ptr(), sched[0][0], sched[0][1], d_out2.data_ptr(), hip_stream=cs)
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            b.dred_step_packed(d_lat.data_ptr(), sched[0][0], sched[0][1], 4 * sched[0][0], 4 * sched[0][1], hip_stream=cs)
        d_out2.add_(0)                                    # (the capture stays usable and is not empty)
    b.sync()
    # the active prefix of six: the uniform forms cover it, the others' rows and records stay
    b.dred_init(state)
    before = [b.get_dred_dec_state(s) for s in range(N)]
    b.active = 6
    try:
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*not active"):
            b.dred_step(latents, np.zeros(N, np.int32), np.ones(N, np.int32), fresh())
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*not active"):
            b.dred_init(state, np.ones(N, np.int32))
        assert all(np.array_equal(bits(x), bits(b.get_dred_dec_state(s))) for s, x in enumerate(before))
        d_out3 = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        b.dred_step_device(d_lat.data_ptr(), None, None, d_out3.data_ptr(), first_latent=0, n_latents=1)
        b.sync()
    finally:
        b.active = N
    got = d_out3.cpu().numpy()
    live = [s for s in range(6) if dm.COUNT[s] > 0]
    assert np.array_equal(bits(got[live, :4]), bits(want[live, :4])) and (bits(got[:, 4:]) == bits(SENTINEL)).all() and (bits(got[6:]) == bits(SENTINEL)).all()
    assert all(np.array_equal(bits(before[s]), bits(b.get_dred_dec_state(s))) for s in range(6, N))
    assert not any(np.array_equal(bits(before[s]), bits(b.get_dred_dec_state(s))) for s in range(6))
    # two unequal shards on one device: the host forms, then every shard's device forms
    sb = api.LPCNetBatch(N, cases["f", "mixed"][0], devices=[0, 0])
    assert [x[:2] for x in sb.shards] == [(0, 5), (5, 4)]
    sb.dred_enable(ML)
    sb.dred_state_enable()
    assert_decoded(run(sb, state, latents, sched, fresh()), want, dm.COUNT, "sharded host forms")
    d_out4 = torch.full((N, 4 * ML, 20), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for k, (first, cnt_k, _) in enumerate(sb.shards):
        sl = slice(first, first + cnt_k)
        sb.dred_init_device(d_state[sl].data_ptr(), shard=k)
        for start, cnt in sched:
            sb.dred_step_device(d_lat[sl].data_ptr(), start[sl], cnt[sl], d_out4[sl].data_ptr(), shard=k)
    sb.sync()
    assert_decoded(d_out4.cpu().numpy(), want, dm.COUNT, "device shards")
    with pytest.raises(api.LPCNetError, match=r"\(-4\).*shard"):
        sb.dred_step_device(d_lat.data_ptr(), sched[0][0], sched[0][1], d_out4.data_ptr())
    sb.close()


@pytest.mark.parametrize("form", [0, 8])
def test_packed_form_is_the_permutation_of_the_plain_rows(form, cases, batches):
    import torch
    _, state, latents, want = cases["f", "small"]
    dev = torch.device("cuda:0")
    d_lat = torch.from_numpy(latents).to(dev)
    b = batches("f", "small")
    b.dred_form(form)
    try:
        b.dred_init(state)
        torch.cuda.synchronize()
        for start, cnt in three_cuts(dm.COUNT):
            # per stream: the whole range (0, 5), nothing (2, 4), the last row alone (6), ranges inside -- in the stream's own row numbers
            lo, hi = 4 * start, 4 * (start + cnt)
            first, take = lo.copy(), (hi - lo).copy()
            take[4] = 0
            first[6], take[6] = max(hi[6] - 1, lo[6]), min(1, hi[6] - lo[6])
            for s in (1, 3, 7, 8):
                if take[s] > 2:
                    first[s], take[s] = first[s] + 1, take[s] - 2
            out = b.dred_step_packed(d_lat.data_ptr(), start, cnt, first, take)
            b.sync()
            assert out.shape == (int(take.sum()), 20)
            assert np.array_equal(bits(out.cpu().numpy()), bits(dm.packed(want, first, take))), (form, start.tolist())
        # first / take outside the call's rows: refused, the records untouched
        before = [b.get_dred_dec_state(s) for s in range(N)]
        start, cnt = np.ones(N, np.int32), np.ones(N, np.int32)
        ok_f, ok_t = 4 * start, 4 * cnt
        one = lambda s: (np.arange(N) == s).astype(np.int32)
        for f, t in ((ok_f - one(3), ok_t), (ok_f, ok_t + one(1)), (ok_f + 2 * one(5), ok_t - one(5)), (ok_f, ok_t - 5 * one(2))):
            with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
                b.dred_step_packed(d_lat.data_ptr(), start, cnt, f, t)
        assert all(np.array_equal(bits(x), bits(b.get_dred_dec_state(s))) for s, x in enumerate(before))
    finally:
        b.dred_form(0)


def test_refusals_leave_records_and_outputs_untouched(cases, batches, blob_f32):
    _, state, latents, _ = cases["f", "small"]
    zero, ones = np.zeros(N, np.int32), np.ones(N, np.int32)
    # before dred_enable, and after it but before dred_state_enable
    b = api.LPCNetBatch(N, cases["f", "small"][0])
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*enabled"):
        b.dred_state_enable()
    b.dred_enable(ML)
    for call in (lambda: b.dred_init(state), lambda: b.dred_step(latents, zero, ones), lambda: b.dred_init_device(0), lambda: b.dred_step_device(0, zero, ones, 0),
                 lambda: b.dred_step_device(0, None, None, 0, n_latents=1), lambda: b.dred_step_packed(0, zero, ones, zero, ones), lambda: b.get_dred_dec_state(0),
                 lambda: b.set_dred_dec_state(0, np.zeros(48, np.float32)), lambda: b.dred_dec_state_size()):
        with pytest.raises(api.LPCNetError, match=r"\(-5\).*state.*enabled"):
            call()
    assert api.SNAP["DRED_DEC"] not in [x[0] for x in b.snapshot_layout()["sections"]]
    b.close()
    b = batches("f", "small")
    b.dred_init(state)
    before = [b.get_dred_dec_state(s) for s in range(N)]
    for start, cnt in ((-one_hot(4), ones), (zero, -one_hot(5)), (zero + (ML - 1) * one_hot(1), ones + one_hot(1)), (zero + ML * one_hot(7), ones)):
        out = fresh()
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*latents outside"):
            b.dred_step(latents, start, cnt, out)
        assert (bits(out) == bits(SENTINEL)).all()
    for first, n in ((-1, 1), (0, -1), (ML, 1), (3, ML - 2)):
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*outside"):
            b.dred_step_device(0, None, None, 0, first_latent=first, n_latents=n)
    assert all(np.array_equal(bits(x), bits(b.get_dred_dec_state(s))) for s, x in enumerate(before))
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.get_dred_dec_state(N)


def one_hot(s):
    return (np.arange(N) == s).astype(np.int32)


def test_the_uniform_form_in_a_capture(cases):
    """init + step(3) + step(4) captured once and replayed with new states and latents in the same buffers"""
    import torch
    blob, state, latents, want = cases["f", "small"]
    dev = torch.device("cuda:0")
    full = np.full(N, ML, np.int32)
    b = api.LPCNetBatch(N, blob)
    b.dred_enable(ML)
    b.dred_state_enable()
    d_state, d_lat = torch.zeros((N, state.shape[1]), dtype=torch.float32, device=dev), torch.zeros(latents.shape, dtype=torch.float32, device=dev)
    d_out = torch.zeros((N, 4 * ML, 20), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.dred_init_device(d_state.data_ptr())                # (a first launch outside the capture)
    b.dred_step_device(d_lat.data_ptr(), None, None, d_out.data_ptr(), first_latent=0, n_latents=1)
    b.sync()
    b.reset()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=st):
        cs = torch.cuda.current_stream().cuda_stream
        b.dred_init_device(d_state.data_ptr(), hip_stream=cs)
        b.dred_step_device(d_lat.data_ptr(), None, None, d_out.data_ptr(), hip_stream=cs, first_latent=0, n_latents=3)
        b.dred_step_device(d_lat.data_ptr(), None, None, d_out.data_ptr(), hip_stream=cs, first_latent=3, n_latents=4)
    assert not b.get_dred_dec_state(0).any()              # (the capture ran nothing)
    e = api.LPCNetBatch(N, blob)
    e.dred_enable(ML)
    e.dred_state_enable()
    for k, (s_in, l_in) in enumerate(((state, latents), (state[::-1].copy(), (latents[::-1] * np.float32(0.5)).copy()))):
        d_state.copy_(torch.from_numpy(s_in))
        d_lat.copy_(torch.from_numpy(l_in))
        d_out.fill_(float(SENTINEL))
        g.replay()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        eager = run(e, s_in, l_in, [(np.zeros(N, np.int32), np.full(N, 3, np.int32)), (np.full(N, 3, np.int32), np.full(N, 4, np.int32))], fresh())
        assert np.array_equal(bits(got), bits(eager)) and np.array_equal(bits(got), bits(e.dred_decode(s_in, l_in, full, fresh()))), k
        assert all(np.array_equal(bits(b.get_dred_dec_state(s)), bits(e.get_dred_dec_state(s))) for s in range(N))
        if k == 0:                                        # (every stream ran all seven; the fixture has a stream's first COUNT[s])
            assert all(np.array_equal(bits(got[s, :4 * int(dm.COUNT[s])]), bits(want[s, :4 * int(dm.COUNT[s])])) for s in range(N))
    b.close()
    e.close()


# ------------------------------------------------------------------------------------------------------------------ into the PLC
def test_stepped_redundancy_goes_into_the_plc_without_a_host_hop(cases):
    """two batches of eight streams on a blob with the PLC network and the decoder: one fed by dred_init -> two dred_step_packed -> plc_fec_feed_device
    on one stream, the other by the host feed with the reference's vectors; then twelve steps with a five-frame loss"""
    import torch
    n = 8
    blob = dm.set_blob("mixed", with_plc=True)
    _, state, latents, want = cases["f", "mixed"]
    count = dm.COUNT[:n]
    c1 = np.minimum(count, 2).astype(np.int32)
    calls = [(np.zeros(n, np.int32), c1), (c1, (count - c1).astype(np.int32))]
    dev = torch.device("cuda:0")
    d_state, d_lat = torch.from_numpy(state[:n]).to(dev), torch.from_numpy(latents[:n]).to(dev)
    pcm = np.stack([pm.stream_pcm(s, 12) for s in range(n)])
    lost = np.zeros(12, np.uint8)
    lost[4:9] = 1

    def steps(b):
        out = np.zeros((n, 12, 160), np.int16)
        for t in range(12):
            frame = np.ascontiguousarray(pcm[:, t])
            if lost[t]:
                frame[:] = 0
            out[:, t] = b.plc_step(frame, np.full(n, lost[t], np.uint8))
        return out, [b.get_plc_state(s) for s in range(n)]

    a = api.LPCNetBatch(n, blob)
    a.plc_enable(api.PLC_CAUSAL)
    a.dred_enable(ML)
    a.dred_state_enable()
    h = api.LPCNetBatch(n, blob)
    h.plc_enable(api.PLC_CAUSAL)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        a.dred_init_device(d_state.data_ptr(), hip_stream=st.cuda_stream)
        for start, cnt in calls:
            first, take = (4 * start).astype(np.int32), (4 * cnt).astype(np.int32)
            buf = a.dred_step_packed(d_lat.data_ptr(), start, cnt, first, take, hip_stream=st.cuda_stream)
            dropped = a.plc_fec_feed_device(buf.data_ptr(), take, hip_stream=st.cuda_stream)          # (nothing waits between the decoder and the feed)
            assert not dropped.any()
            assert not h.plc_fec_feed(dm.packed(want[:n], first, take), take).any()
    a.sync()
    got, got_state = steps(a)
    a.close()
    ref, ref_state = steps(h)
    h.plc_reset()
    bare, _ = steps(h)
    h.close()
    assert np.array_equal(got, ref) and got_state == ref_state
    assert not np.array_equal(bare[:, 4:9], ref[:, 4:9])          # (the vectors matter: without them the concealment differs)
