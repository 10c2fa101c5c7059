"""The encoder and the feature analysis in the forms a production-sized batch runs: the VQ kernels with 2, 3 and 4 (stream, packet) items per
wavefront, their ragged last workgroups, and calls that the 65 536-item bound cuts into two chunks (lpcnet_amd/csrc/encode_plan.h).  One batch of
capacity 2 048; the active prefix selects the item count.  Every stream is compared on bytes -- packets or the bit patterns of the features,
get_encoder_vq_mem, get_analysis_state -- with the same streams through batches of 256 streams, which run one item per wavefront and one chunk:
the form tests/test_gpu_encode.py and tests/test_gpu_analysis.py pin against the reference.  Six of the streams are those of
tests/golden/golden_encode_v1.npz and are compared with that fixture directly.  api.encode_plan (the engine's own rule) is asserted before each run,
so a change of the rule that lets a case fall back to the small form fails here and in tests/test_encode_plan_host.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import encode_large_cases as cases  # noqa: E402
import make_golden_encode as mge  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

pytestmark = pytest.mark.gpu
N, SMALL, GOLD_AT = cases.N, cases.SMALL, cases.GOLD_AT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def states(b, count):
    return [b.get_analysis_state(s) for s in range(count)], np.stack([b.get_encoder_vq_mem(s) for s in range(count)])


def assert_states(b, count, want, what):
    an, mem = states(b, count)
    bad = [s for s in range(count) if an[s] != want[0][s]]
    assert not bad, (what, "analysis state", len(bad), bad[:8])
    bad = np.flatnonzero((bits(mem) != bits(want[1][:count])).any(axis=1))
    assert bad.size == 0, (what, "vq_mem", bad.size, bad[:8].tolist())


def small_runs(blob, pcm, run):
    """run(batch of SMALL streams from reset, its pcm rows) -> a tuple of arrays / lists per call; -> the same, over all N streams"""
    b = api.LPCNetBatch(SMALL, blob)
    parts = []
    for k in range(0, N, SMALL):
        b.analysis_reset()
        parts.append(run(b, pcm[k:k + SMALL]))
    b.close()
    out = []
    for col in zip(*parts):
        out.append(np.concatenate(col) if isinstance(col[0], np.ndarray) else [x for part in col for x in part])
    return out


@pytest.fixture(scope="module")
def gold():
    g = np.load(mge.PATH)
    return dict(packets=g["packets"], feats=g["features"], cbs=synth.make_codebooks(int(g["codebook_seed"])))


@pytest.fixture(scope="module")
def pcm():
    return cases.big_pcm()


@pytest.fixture(scope="module")
def big(blob_f32, hip_lib):
    cases.check_plans()
    b = api.LPCNetBatch(N, blob_f32)
    yield b
    b.close()


@pytest.fixture()
def codebooks(gold, hip_lib):
    api.set_codebooks(*gold["cbs"])


@pytest.fixture(scope="module")
def ref_encode(blob_f32, pcm, gold):
    """packets 0..7, then 8, then 9 in three calls of the small form, the states after each"""
    api.set_codebooks(*gold["cbs"])

    def run(b, rows):
        out = []
        for lo, hi in ((0, 8), (8, 9), (9, 10)):
            out.append(b.encode(rows[:, lo * 640:hi * 640]))
            an, mem = states(b, SMALL)
            out += [an, mem]
        return tuple(out)
    r = small_runs(blob_f32, pcm, run)
    return dict(packets=np.concatenate([r[0], r[3], r[6]], axis=1), after={8: (r[1], r[2]), 9: (r[4], r[5]), 10: (r[7], r[8])})


def test_the_small_form_reference_equals_the_fixture_on_its_six_streams(ref_encode, gold):
    assert np.array_equal(ref_encode["packets"][list(GOLD_AT)], gold["packets"][:, :10])


def test_encode_in_two_chunks_at_four_items_per_wavefront(big, pcm, gold, codebooks, ref_encode):
    active, P, plan = cases.ENCODE["chunked"]
    assert api.encode_plan(N, active, P) == plan and [(r["packets"], r["ipw_end"], r["ipw_mid"]) for r in plan] == [(8, 4, 2), (1, 1, 1)]
    big.active = active
    big.analysis_reset()
    out = big.encode(pcm[:, :P * 640])
    assert np.array_equal(out[list(GOLD_AT)], gold["packets"][:, :P])
    bad = np.flatnonzero((out != ref_encode["packets"][:, :P]).any(axis=(1, 2)))
    assert bad.size == 0, (bad.size, bad[:8].tolist(), [int((out[:, p] != ref_encode["packets"][:, p]).any(axis=1).sum()) for p in range(P)])
    assert_states(big, N, ref_encode["after"][9], "after the chunked call")
    # the state and vq_mem a chunked call leaves are the ones the next call starts from
    nxt = big.encode(pcm[:, P * 640:(P + 1) * 640])
    assert np.array_equal(nxt[list(GOLD_AT)], gold["packets"][:, P:P + 1]) and np.array_equal(nxt, ref_encode["packets"][:, P:P + 1])
    assert_states(big, N, ref_encode["after"][10], "after the following call")


@pytest.mark.parametrize("case", ["ragged3", "ragged2"])
def test_encode_device_with_a_ragged_last_workgroup(big, pcm, gold, codebooks, ref_encode, case):
    active, P, plan = cases.ENCODE[case]
    assert api.encode_plan(N, active, P) == plan and len(plan) == 1 and plan[0]["last_end"] == 8 and plan[0]["last_mid"] == 8
    assert (plan[0]["ipw_end"], plan[0]["ipw_mid"]) == ((3, 2) if case == "ragged3" else (2, 2))
    big.active = active
    big.analysis_reset()
    import torch
    dev = torch.device("cuda:0")
    rows = np.array(pcm[:, :P * 640])
    rows[active:] = 0x5555                                                       # (inactive rows are not read)
    d_in = torch.from_numpy(rows).to(dev)
    d_pk = torch.full((N, P, 8), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    big.encode_device(d_in.data_ptr(), d_pk.data_ptr(), P)
    big.sync()
    out = d_pk.cpu().numpy()
    at = [s for s in GOLD_AT if s < active]
    assert at[-1] == active - 1                                                  # the last active stream, alone in the last workgroup
    assert np.array_equal(out[at], gold["packets"][[GOLD_AT.index(s) for s in at], :P])
    bad = np.flatnonzero((out[:active] != ref_encode["packets"][:active, :P]).any(axis=(1, 2)))
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert (out[active:] == 0xA5).all()                                          # slots past the end write nothing: no packet ...
    assert not big.get_encoder_vq_mem(active).any() and not big.get_encoder_vq_mem(N - 1).any()      # ... and no vq_mem
    assert_states(big, active, ref_encode["after"][8], case)
    big.active = N


def test_compute_features_device_in_two_chunks_into_a_callers_stride(big, pcm, gold, blob_f32):
    import torch
    active, P, chunks = cases.FEATURES
    assert [r["packets"] for r in api.encode_plan(N, active, P)] == chunks and len(chunks) == 2

    def run(b, rows):
        f = b.compute_features(rows[:, :P * 640])
        an, mem = states(b, SMALL)
        return f, an, mem
    want, an, mem = small_runs(blob_f32, pcm, run)
    assert np.array_equal(bits(want[list(GOLD_AT)]), bits(gold["feats"][:, :4 * P]))
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(np.ascontiguousarray(pcm[:, :P * 640])).to(dev)
    d_feat = torch.full((N, 4 * P, 40), -777.25, dtype=torch.float32, device=dev)
    big.active = active
    big.analysis_reset()
    torch.cuda.synchronize()
    big.compute_features_device(d_in.data_ptr(), d_feat.data_ptr(), 40, P)
    big.sync()
    f = d_feat.cpu().numpy()
    assert (f[:, :, 36:] == np.float32(-777.25)).all()                           # in every row of both chunks
    assert np.array_equal(bits(f[list(GOLD_AT), :, :36]), bits(gold["feats"][:, :4 * P]))
    bad = (bits(f[:, :, :36]) != bits(want)).any(axis=2)
    assert not bad.any(), (int(bad.any(axis=1).sum()), bad.sum(axis=0).tolist())
    assert_states(big, N, (an, mem), "compute_features_device")


@pytest.fixture(scope="module")
def ref_analyze(blob_f32, pcm):
    T = cases.ANALYZE[1]

    def run(b, rows):
        f = b.analyze(rows[:, :T * 160])
        an, mem = states(b, SMALL)
        b.analysis_reset()
        ff = b.analyze(rows[:, :T * 160].astype(np.float32))                    # the float entry point, from reset
        return f, an, mem, ff, [b.get_analysis_state(s) for s in range(SMALL)]
    f, an, mem, ff, anf = small_runs(blob_f32, pcm, run)
    return dict(feats=f, state=(an, mem), feats_float=ff, state_float=(anf, mem))


def test_analyze_from_host_int16_in_chunks_of_32_and_1_frames(big, pcm, ref_analyze):
    active, T, chunks = cases.ANALYZE
    assert [r["frames"] for r in api.encode_plan(N, active, T, analysis=True)] == chunks == [32, 1]
    big.active = active
    big.analysis_reset()
    out = big.analyze(pcm[:, :T * 160])
    bad = (bits(out) != bits(ref_analyze["feats"])).any(axis=2)
    assert not bad.any(), (int(bad.any(axis=1).sum()), bad.sum(axis=0).tolist())
    assert_states(big, N, ref_analyze["state"], "analyze")


def test_analyze_device_from_float_in_chunks_into_a_callers_stride(big, pcm, ref_analyze):
    import torch
    active, T, chunks = cases.ANALYZE
    assert [r["frames"] for r in api.encode_plan(N, active, T, analysis=True)] == chunks
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(pcm[:, :T * 160].astype(np.float32)).to(dev)
    d_feat = torch.full((N, T, 40), -777.25, dtype=torch.float32, device=dev)
    big.active = active
    big.analysis_reset()
    torch.cuda.synchronize()
    big.analyze_device(d_in.data_ptr(), True, d_feat.data_ptr(), 40, T)
    big.sync()
    f = d_feat.cpu().numpy()
    assert (f[:, :, 36:] == np.float32(-777.25)).all()
    bad = (bits(f[:, :, :36]) != bits(ref_analyze["feats_float"])).any(axis=2)
    assert not bad.any(), (int(bad.any(axis=1).sum()), bad.sum(axis=0).tolist())
    assert np.array_equal(bits(ref_analyze["feats_float"]), bits(ref_analyze["feats"]))      # (integer-valued floats: what the int16 entry gives)
    assert_states(big, N, ref_analyze["state_float"], "analyze_device")
