"""Stream snapshots on the device (lpcnet_batch_snapshot / _restore, their _device forms, lpcnet_batch_copy_streams_to, StreamRoster.migrate): m
streams' complete records to or from one contiguous buffer in one launch.  At most twelve streams and a handful of frames per case; every
comparison is on bit patterns, against the source batch, an undisturbed twin or a batch that moved the same streams with copy_streams.
Between them the cases cover m = 1 and m > 1, the last stream of the capacity, a row shorter than one pass of 256 lanes (the PLC's `delta`,
4 bytes) and one longer than an int4 pass (its FEC ring, 8 000 bytes), the three vector widths in one launch (int4: the kept products; int2:
the 3 592-byte state; int: the 3 924-byte analysis record) and a PLC network record whose size comes from the blob."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dred_enc_model as em  # noqa: E402
import plc_fec_script as fs  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402
from lpcnet_amd.roster import StreamRoster  # noqa: E402
from test_gpu_parity import feats_for  # noqa: E402

pytestmark = pytest.mark.gpu

S = api.SNAP


def raw(b, s):
    return bytes(b.get_state(s))


def getters(b, s, an=False, enc=False, plc=False, denc=False):
    """every existing getter of stream s that the batch's configuration has (get_analysis_state would allocate the analysis where it is missing)"""
    out = [raw(b, s), b.get_decoder_vq_mem(s).tobytes()]
    if an:
        out.append(b.get_analysis_state(s))
    if enc:
        out.append(b.get_encoder_vq_mem(s).tobytes())
    if plc:
        out.append(b.get_plc_state(s))
    if denc:
        out.append(b.get_dred_enc_state(s).tobytes())
    return out


def tone(n, samples, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(samples)
    return np.stack([(6000 * np.sin(2 * np.pi * t * (120. + 37. * s) / 16000.) + rng.normal(0, 300, t.size)).astype(np.int16) for s in range(n)])


# ---------------------------------------------------------------------------------------------------------- 1. a restored stream carries on
@pytest.mark.parametrize("src,dst", [([1, 5, 6, 11], [0, 3, 4, 6]), ([11], [6])], ids=["m4", "m1-last-stream"])
def test_a_restored_stream_carries_on(src, dst, blob_f32, hip_lib):
    fa = feats_for(range(9100, 9112), 5)
    fb = feats_for(range(9150, 9157), 2)
    a, b, ctrl = api.LPCNetBatch(12, blob_f32), api.LPCNetBatch(7, blob_f32), api.LPCNetBatch(7, blob_f32)
    a.synthesize(fa[:, :3])
    blob = a.snapshot(src)
    assert api.snapshot_info(blob)["m"] == len(src)
    b.restore(dst, blob)
    pa = a.synthesize(fa[:, 3:])
    fb[dst] = fa[src, 3:]
    pb, pc = b.synthesize(fb), ctrl.synthesize(fb)
    assert np.array_equal(pb[dst], pa[src])
    assert [raw(b, d) for d in dst] == [raw(a, s) for s in src]
    rest = [s for s in range(7) if s not in dst]
    assert np.array_equal(pb[rest], pc[rest]) and [raw(b, s) for s in rest] == [raw(ctrl, s) for s in rest]
    for x in (a, b, ctrl):
        x.close()


# ---------------------------------------------------------------------------------------------------------- 2. every subsystem, one launch
N5 = fs.N
LOST = np.zeros((5, N5), np.uint8)
LOST[2:5, 1] = 1               # stream 1: lost from step 2 on -- the burst is open when the snapshot is taken
LOST[3:5, 2] = 1               # stream 2: one frame into its outage
LOST[2, 3] = 1                 # stream 3: just out of one, samples in its PCM queue
STEPS = 4
MD = 2                         # double frames per DRED encoder call
DENC_COUNT = np.array([2, 1, 0, 2, 1], np.int32)
STEP_MODE = np.array([1, 0, 0, 0, 1], np.int32)          # the per-stream step: streams 0 and 4


@pytest.fixture(scope="module")
def blob_all():
    m = plc_synth.make_model_with_plc()
    s = em.SETS["narrow"]
    em.add_dred_enc(m, s["widths"], taps=s["taps"], latent_dim=s["latent_dim"], gdense1=s["gdense1"], state_dim=s["state_dim"])
    return synth.blob_bytes(m)


def make_all(n, blob):
    b = api.LPCNetBatch(n, blob)
    b.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    b.encoder_enable(1)
    b.dred_enc_enable(MD)
    return b


def test_every_subsystem_in_one_launch(blob_all, hip_lib):
    api.set_codebooks(*synth.make_codebooks(5))
    sc = fs.script()
    a, b = make_all(N5, blob_all), make_all(N5, blob_all)
    lay = a.snapshot_layout()
    size = {s[0]: s[1] for s in lay["sections"]}
    assert [s[0] for s in lay["sections"]] == list(range(1, 21))            # every section there is
    assert size[S["PLC_NET"]] == 4 * (plc_synth.PLC_G1 + plc_synth.PLC_G2) * 4 and size[S["PLC_DELTA"]] == 4 and size[S["PLC_FEC"]] == 8000
    assert 0 <= size[S["DRED_ENC"]] - 4 * a.dred_enc_info()[6] <= 16      # (the device record: the exported state and the conv ring's head)
    assert size[S["KEEP_A"]] % 16 == 0 and size[S["SYNTH"]] % 16 == 8 and size[S["AN"]] % 8 == 4
    step_feat = feats_for([9200 + s for s in range(N5)], 1)[:, 0]
    enc_pcm = tone(N5, 2 * 640, 41)
    denc_feat = em.inputs(N5, 2 * MD)[:, :, :20]

    def plc_step(bt, t, rows):
        r0 = fs.step_rows(sc, t)[0]
        starts = r0 + np.concatenate([[0], np.cumsum(sc["count"][t])[:-1]])
        vec = [sc["vec"][starts[s]:starts[s] + sc["count"][t, s]] for s in rows]
        bt.plc_fec_feed(vec, sc["count"][t, rows], sc["skip"][t, rows], sc["clear"][t, rows])
        frame = np.ascontiguousarray(sc["pcm"][rows, t])
        frame[LOST[t, rows] != 0] = 0
        return bt.plc_step(frame, LOST[t, rows])

    ident = list(range(N5))
    for t in range(STEPS):
        plc_step(a, t, ident)
    a.encode(enc_pcm[:, :640])
    a.dred_encode(np.ascontiguousarray(denc_feat[:, :2 * MD]), DENC_COUNT)
    for n in (160, 160, 80):           # (last: any other call drops the kept products' flag; three frames: the first two of a stream give silence and
        a.synthesize_step(step_feat, np.zeros((N5, 160), np.int16), [n] * N5, [0] * N5, STEP_MODE)      #  leave the sample state alone)
    ctl = np.stack([np.frombuffer(a.get_plc_state(s)[:36], np.int32) for s in range(N5)])
    assert ctl[1, 2] == 1 and ctl[2, 3] == 1 and 0 < ctl[1, 4] < 100      # streams 1, 2: mid-outage; 1: a partly filled FEC ring ...
    assert ctl[1, 6] > 0 and ctl[3, 0] == 80 and ctl[0, 8] == 4           # ... that it reads from; stream 3: a PCM queue; stream 0: deferred features
    src, dst = [4, 2, 0, 1, 3], [1, 3, 0, 4, 2]
    blob = a.snapshot(src)
    assert api.snapshot_info(blob)["sections"] == lay["sections"]
    b.restore(dst, blob)
    owner = np.zeros(N5, np.int64)                                          # slot of b -> stream of a
    owner[dst] = src
    cfg = dict(an=True, enc=True, plc=True, denc=True)
    for slot in range(N5):
        assert getters(b, slot, **cfg) == getters(a, int(owner[slot]), **cfg), slot
    # the next call of every subsystem; the tail-only step first: it needs the kept products and their flag, and any other call drops the flag
    z = np.zeros((N5, 160), np.int16)
    at_snapshot = raw(a, 0)
    ta = a.synthesize_step(step_feat, z, [80] * N5, [0] * N5, 2 * STEP_MODE)
    tb = b.synthesize_step(step_feat[owner], z, [80] * N5, [0] * N5, 2 * STEP_MODE[owner])
    assert np.array_equal(tb, ta[owner]) and raw(a, 0) != at_snapshot and raw(b, int(dst[src.index(0)])) == raw(a, 0)
    assert np.array_equal(plc_step(b, STEPS, [int(x) for x in owner]), plc_step(a, STEPS, ident)[owner])
    assert np.array_equal(b.encode(enc_pcm[owner, 640:]), a.encode(enc_pcm[:, 640:])[owner])
    la, ia = a.dred_encode(np.ascontiguousarray(denc_feat[:, 2 * MD:]), DENC_COUNT[::-1].copy())
    lb, ib = b.dred_encode(np.ascontiguousarray(denc_feat[owner, 2 * MD:]), DENC_COUNT[::-1][owner].copy())
    assert np.array_equal(lb.view(np.uint32), la[owner].view(np.uint32)) and np.array_equal(ib.view(np.uint32), ia[owner].view(np.uint32))
    for slot in range(N5):
        assert getters(b, slot, **cfg) == getters(a, int(owner[slot]), **cfg), slot
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 3. the same as copy_streams
def test_snapshot_and_restore_inside_a_batch_equal_copy_streams(blob_f32, hip_lib):
    api.set_codebooks(*synth.make_codebooks(5))
    feats = feats_for(range(9300, 9310), 2)
    pcm = tone(10, 640, 42)
    both = []
    for _ in range(2):
        b = api.LPCNetBatch(10, blob_f32)
        b.encoder_enable(1)
        b.synthesize(feats)
        b.encode(pcm)
        both.append(b)
    a, twin = both
    a.restore([4, 0], a.snapshot([2, 9]))
    twin.copy_streams([2, 9], [4, 0])
    for s in range(10):
        assert getters(a, s, an=True, enc=True) == getters(twin, s, an=True, enc=True), s
    assert getters(a, 4, an=True, enc=True) == getters(a, 2, an=True, enc=True) and raw(a, 0) == raw(a, 9) != raw(a, 1)
    a.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------- 4. the host blob
def test_host_blob_round_trip(blob_f32, hip_lib):
    feats = feats_for(range(9400, 9406), 2)
    a = api.LPCNetBatch(6, blob_f32)
    a.analysis_enable(1)
    a.analyze(tone(6, 320, 43))
    a.synthesize(feats)
    blob = a.snapshot([5, 0, 3])
    assert blob == a.snapshot([5, 0, 3])                                    # nothing in between: the same bytes, padding included
    assert blob[:4] == b"LPCS" and len(blob) == hip_lib.lpcnet_batch_snapshot_bytes(a.p, 3)
    info, lay = api.snapshot_info(blob), a.snapshot_layout()
    assert info["sections"] == lay["sections"] and info["record_bytes"] == lay["record_bytes"] and info["m"] == 3
    assert [s[0] for s in lay["sections"]] == [S["SYNTH"], S["DEC_VQ"], S["AN"], S["KEEP_FLAG"]]
    assert info["int8"] == 0 and info["plc"] == 0 and info["state_size"] == hip_lib.lpcnet_batch_state_size() and info["model_hash"] != 0
    b = api.LPCNetBatch(2, blob_f32)
    b.analysis_enable(1)
    b.restore([1, 0], blob)                                                 # the first two records of three
    assert getters(b, 1, an=True) == getters(a, 5, an=True) and getters(b, 0, an=True) == getters(a, 0, an=True)
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        b.restore([0, 1, 0], blob)
    with pytest.raises(api.LPCNetError, match=r"\(-4\).*fewer"):
        api.LPCNetBatch(4, blob_f32).restore([0, 1, 2, 3], blob)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 5. ordering without a wait
def test_device_forms_are_ordered_by_enqueue_alone(blob_f32, hip_lib):
    import torch
    feats = feats_for(range(9500, 9506), 2)
    d_f1, d_f2 = (torch.from_numpy(np.ascontiguousarray(feats[:, t:t + 1])).cuda() for t in (0, 1))
    d_pcm = torch.zeros((6, 160), dtype=torch.int16, device="cuda")
    s = torch.cuda.Stream()
    a, twin, c = (api.LPCNetBatch(6, blob_f32) for _ in range(3))
    lay = a.snapshot_layout()
    rb = lay["record_bytes"]
    streams = [5, 2, 0]
    rec = torch.full((3 * rb,), 0x55, dtype=torch.uint8, device="cuda")
    rec_twin = torch.full((3 * rb,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.synthesize_device(d_f1.data_ptr(), 36, d_pcm.data_ptr(), 1, s.cuda_stream)
    meta = a.snapshot_device(streams, rec.data_ptr(), s.cuda_stream)
    assert meta.shape == (3, api.SNAP_META) and not meta.any()              # (written when the call returned: no PLC, no kept products)
    a.synthesize_device(d_f2.data_ptr(), 36, d_pcm.data_ptr(), 1, s.cuda_stream)
    s.synchronize(); a.sync()
    twin.synthesize(feats[:, :1])
    twin.snapshot_device(streams, rec_twin.data_ptr())
    twin.sync()
    assert torch.equal(rec, rec_twin)                                       # the state after the FIRST frame, padding zeroed
    assert raw(a, 5) != raw(twin, 5)                                        # (a itself is a frame further)
    # ... and back in, behind a frame that the restore must come after: c runs frame 1, takes the records, runs frame 2 == the twin's second frame
    c.synthesize_device(d_f1.data_ptr(), 36, d_pcm.data_ptr(), 1, s.cuda_stream)
    c.restore_device([1, 3, 4], rec.data_ptr(), meta, lay["sections"], s.cuda_stream)
    d_f = torch.from_numpy(np.ascontiguousarray(feats[[0, 5, 2, 2, 0, 5], 1:2])).cuda()
    c.synthesize_device(d_f.data_ptr(), 36, d_pcm.data_ptr(), 1, s.cuda_stream)
    s.synchronize(); c.sync()
    want = twin.synthesize(feats[:, 1:])
    assert np.array_equal(d_pcm.cpu().numpy(), want[[0, 5, 2, 2, 0, 5]])
    assert [raw(c, x) for x in range(6)] == [raw(twin, x) for x in (0, 5, 2, 2, 0, 5)]
    g = torch.cuda.CUDAGraph()
    before = [raw(c, x) for x in range(6)]
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            c.snapshot_device(streams, rec.data_ptr(), cs)
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*captur"):
            c.restore_device([0, 1, 2], rec.data_ptr(), meta, lay["sections"], cs)
        d_pcm.add_(0)                                                       # (the capture stays usable and is not empty)
    c.sync()
    assert torch.equal(rec, rec_twin) and [raw(c, x) for x in range(6)] == before
    for x in (a, twin, c):
        x.close()


# ---------------------------------------------------------------------------------------------------------- 6. shards
@pytest.mark.parametrize("flavour", ["float", "int8"])
def test_records_change_shard(flavour, blob_f32, blob_i8, hip_lib):
    blob = blob_f32 if flavour == "float" else blob_i8
    feats = feats_for(range(9600, 9610), 4)
    u = api.LPCNetBatch(10, blob, devices=[0, 0])                           # an undisturbed twin
    want = u.synthesize(feats).reshape(10, 4, 160)
    b = api.LPCNetBatch(10, blob, devices=[0, 0])
    assert [(f, c) for f, c, _ in b.shards] == [(0, 5), (5, 5)]
    assert np.array_equal(b.synthesize(feats[:, :2]).reshape(10, 2, 160), want[:, :2])
    src, dst = [7, 1, 9, 3], [2, 8, 0, 6]                                   # every record changes shard
    blob_s = b.snapshot(src)
    assert api.snapshot_info(blob_s)["int8"] == (flavour == "int8")
    b.restore(dst, blob_s)
    rows = list(range(10))
    for s, d in zip(src, dst):
        rows[d] = s
    got = b.synthesize(feats[rows, 2:]).reshape(10, 2, 160)
    assert np.array_equal(got, want[rows, 2:])
    assert [raw(b, s) for s in range(10)] == [raw(u, r) for r in rows]
    with pytest.raises(api.LPCNetError, match=r"\(-4\).*shard"):
        b.snapshot_device([0], 256)                                         # device pointers belong to one shard
    u.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 7. inactive slots and the prefix
def test_inactive_slots_move_and_the_counts_stay(blob_f32, hip_lib):
    feats = feats_for(range(9700, 9708), 3)
    b = api.LPCNetBatch(8, blob_f32)
    b.synthesize(feats[:, :1])
    b.active = 3
    before = [raw(b, s) for s in range(8)]
    b.restore([7], b.snapshot([6]))
    assert b.active == 3 and b.active_streams == 3
    assert [raw(b, s) for s in range(7)] == before[:7] and raw(b, 7) == before[6] != before[7]
    b.active = 8
    rows = [0, 1, 2, 3, 4, 5, 6, 6]
    p = b.synthesize(feats[rows, 1:])
    assert np.array_equal(p[7], p[6]) and raw(b, 7) == raw(b, 6)
    u = api.LPCNetBatch(8, blob_f32)                                        # an undisturbed twin: slot 7 carried on as stream 6 would
    want = u.synthesize(feats)[:, 160:]
    assert np.array_equal(p, want[rows]) and [raw(b, s) for s in range(8)] == [raw(u, r) for r in rows]
    u.close(); b.close()


# ---------------------------------------------------------------------------------------------------------- 8. refusals leave the batch as it was
def test_refusals_leave_the_batch_as_it_was(blob_f32, blob_i8, hip_lib):
    import torch
    blob_plc = synth.blob_bytes(plc_synth.make_model_with_plc())
    feats = feats_for(range(9800, 9804), 1)
    p = api.LPCNetBatch(2, blob_plc)
    p.plc_enable(api.PLC_CAUSAL | api.PLC_DC_FILTER)
    p.plc_step(tone(2, 160, 44), [0, 0])
    snap_plc = p.snapshot([0, 1])

    def refused(batch, code, word, streams, blob, **cfg):
        before = [getters(batch, s, **cfg) for s in range(batch.n)]
        layout = batch.snapshot_layout()
        with pytest.raises(api.LPCNetError, match=r"\(%d\)" % code) as e:
            batch.restore(streams, blob)
        assert word in str(e.value), str(e.value)
        assert [getters(batch, s, **cfg) for s in range(batch.n)] == before and batch.snapshot_layout() == layout

    d = api.LPCNetBatch(4, blob_f32)
    d.synthesize(feats)
    refused(d, -5, "PLC_CTL", [0, 1], snap_plc)                             # PLC on one side only
    q = api.LPCNetBatch(3, blob_plc)
    q.plc_enable(api.PLC_CODEC)
    q.plc_step(tone(3, 160, 45), [0, 1, 0])
    refused(q, -5, "PLC_CTL", [0, 1], snap_plc, an=True, plc=True)          # other PLC options
    snap_f = d.snapshot([0, 1])
    i8 = api.LPCNetBatch(3, blob_i8)
    i8.synthesize(feats[:3])
    refused(i8, -5, "int8", [0, 1], snap_f)                                 # another flavour
    refused(d, -4, "twice", [2, 2], snap_f)                                 # a duplicate destination
    refused(d, -4, "outside", [1, 4], snap_f)                               # an index equal to the capacity
    refused(d, -4, "not a snapshot blob", [2, 3], snap_f[:-1])              # a blob truncated by one byte
    # a section only the snapshot has: refused by the enqueue-only form, allocated by the host form
    s = api.LPCNetBatch(2, blob_f32)
    s.analysis_enable(1)
    s.analyze(tone(2, 320, 46))
    s.synthesize(feats[:2])
    lay = s.snapshot_layout()
    rec = torch.zeros(lay["record_bytes"], dtype=torch.uint8, device="cuda")
    meta = s.snapshot_device([1], rec.data_ptr())
    s.sync()
    before = [getters(d, x) for x in range(4)]
    with pytest.raises(api.LPCNetError, match=r"\(-5\).*section AN"):
        d.restore_device([2], rec.data_ptr(), meta, lay["sections"])
    assert [getters(d, x) for x in range(4)] == before and S["AN"] not in [x[0] for x in d.snapshot_layout()["sections"]]
    d.restore([2], s.snapshot([1]))
    assert S["AN"] in [x[0] for x in d.snapshot_layout()["sections"]]
    assert getters(d, 2, an=True) == getters(s, 1, an=True) and [getters(d, x) for x in (0, 1, 3)] == [before[x] for x in (0, 1, 3)]
    d.restore_device([3], rec.data_ptr(), meta, lay["sections"])            # ... after which the enqueue-only form fits
    d.sync()
    assert getters(d, 3, an=True) == getters(s, 1, an=True)
    for x in (p, d, q, i8, s):
        x.close()


# ---------------------------------------------------------------------------------------------------------- 9. another batch
@pytest.mark.parametrize("device", [0, 1], ids=["one-device", "two-devices"])
def test_copy_streams_to_and_migrate(device, blob_f32, hip_lib):
    import torch
    if device >= torch.cuda.device_count():
        pytest.skip("the two-device copy needs a second GPU (hipGetDeviceCount() < 2)")
    ids_a, ids_b = ["a0", "a1", "a2", "a3", "a4"], ["b0", "b1"]
    feats = feats_for(range(9900, 9907), 4)                                 # a0 .. a4, b0, b1
    u = api.LPCNetBatch(7, blob_f32)
    want = u.synthesize(feats).reshape(7, 4, 160)
    row = {k: i for i, k in enumerate(ids_a + ids_b)}
    a, b, c = api.LPCNetBatch(6, blob_f32), api.LPCNetBatch(6, blob_f32, device=device), api.LPCNetBatch(3, blob_f32, device=device)
    ra, rb = StreamRoster(batch=a), StreamRoster(batch=b)
    assert [ra.join(k) for k in ids_a] == [0, 1, 2, 3, 4] and [rb.join(k) for k in ids_b] == [0, 1]

    def run(batch, roster, t0, t1):
        """frames [t0, t1) of every stream in the roster, each in its slot"""
        f = np.zeros((batch.n, t1 - t0, 36), np.float32)
        slots = roster.slots()
        for k, slot in slots.items():
            f[slot] = feats[row[k], t0:t1]
        p = batch.synthesize(f).reshape(batch.n, t1 - t0, 160)
        for k, slot in slots.items():
            assert np.array_equal(p[slot], want[row[k], t0:t1]), k

    run(a, ra, 0, 2); run(b, rb, 0, 2)
    # copy_streams_to alone: the source is unchanged, the destination carries on
    before = [raw(a, s) for s in range(6)]
    fresh = raw(c, 1)
    a.copy_streams_to([4, 0], c, [2, 0])
    c.sync(); a.sync()
    assert [raw(a, s) for s in range(6)] == before and raw(c, 2) == before[4] and raw(c, 0) == before[0] and raw(c, 1) == fresh
    pc = c.synthesize(feats[[0, 6, 4], 2:]).reshape(3, 2, 160)
    assert np.array_equal(pc[[0, 2]], want[[0, 4], 2:])
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        a.copy_streams_to([0, 1], c, [1, 1])
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        a.copy_streams_to([0], a, [1])
    # migrate: two streams move to b, a closes its ranks, both books follow
    assert ra.migrate(["a1", "a3"], rb) == {"a1": 2, "a3": 3}
    assert ra.slots() == {"a0": 0, "a4": 1, "a2": 2} and rb.slots() == {"b0": 0, "b1": 1, "a1": 2, "a3": 3}
    assert a.active == 3 and ra.active == [3] and b.active == 4 and rb.active == [4]
    run(a, ra, 2, 4); run(b, rb, 2, 4)
    for k, slot in ra.slots().items():
        assert raw(a, slot) == raw(u, row[k]), k
    for k, slot in rb.slots().items():
        assert raw(b, slot) == raw(u, row[k]), k
    with pytest.raises(ValueError):
        ra.migrate(["a1"], rb)                                              # not in this roster any more
    for x in (u, a, b, c):
        x.close()
