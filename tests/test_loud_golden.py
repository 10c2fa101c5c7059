"""The oracle's LOOP tied to the real reference at full scale: tests/golden/golden_loud_v1.npz holds what the compiled reference
(generic-C float and int8 builds) produces on the loud families of tests/tools/loud_inputs.py (tests/tools/make_golden_loud.py);
the plain-C oracle must reproduce PCM and final state bit for bit, for both flavours.  Every family is in the fixture: the forced
ones through lpcnet_synthesize_impl, the resonator-LPC ones through lpcnet_synthesize_tail_impl with the caller's LPC put into
the state by oracle/ref_harness.c."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import loud_inputs  # noqa: E402
from oracle import orc  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_loud_v1.npz")
FAMS = loud_inputs.families()


@pytest.fixture(scope="module")
def loud_golden():
    return np.load(PATH)


def test_fixture_was_made_from_these_inputs(loud_golden):
    assert list(loud_golden["names"]) == [f.name for f in FAMS] and int(loud_golden["n_frames"]) == loud_inputs.T
    assert np.array_equal(loud_golden["input_crc"], np.array([f.digest() for f in FAMS], np.uint32))
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(os.path.dirname(PATH), "golden_v1.npz"))


@pytest.mark.parametrize("fl", ["f", "i"], ids=["float", "int8"])
def test_oracle_reproduces_the_reference_on_the_loud_families(fl, loud_golden, blob_f32, blob_i8):
    om = orc.OracleModel(blob_f32 if fl == "f" else blob_i8)
    assert om.is_int8 == (fl == "i")
    for fam in FAMS:
        pcm, st, _ = loud_inputs.run_oracle(om, fam)
        assert np.array_equal(pcm, loud_golden[f"pcm_{fl}_{fam.name}"]), fam.name
        for k in loud_inputs.STATE_KEYS:
            want = loud_golden[f"{k}_{fl}_{fam.name}"]
            got = np.asarray(st[k])
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fam.name, k)
        # teacher forcing leaves the imposed samples of live frames untouched
        for t in range(2, loud_inputs.T):
            p = fam.preload[t]
            assert np.array_equal(pcm[t * 160:t * 160 + p], fam.forced[t * 160:t * 160 + p])
    # the fixture is loud: the reference clipped, on both rails
    allpcm = np.concatenate([loud_golden[f"pcm_{fl}_{f.name}"][t * 160 + f.preload[t]:(t + 1) * 160] for f in FAMS for t in range(2, loud_inputs.T)])
    assert (allpcm == 32767).sum() >= 100 and (allpcm == -32767).sum() >= 100


def test_every_stream_slot_of_the_gpu_arrangements_gets_a_clipping_stream(loud_golden):
    """tests/test_gpu_loud.py fills a batch with one group's families in two arrangements (loud_inputs.arrangements): per group that clips
    at all, every stream slot of 8 (every row, both groups of the two-group kernel) and of 13 holds a stream whose free-running samples
    clip in at least one of the two"""
    T = loud_inputs.T

    def clips(f, fl):
        pcm = loud_golden[f"pcm_{fl}_{f.name}"]
        free = np.concatenate([pcm[t * 160 + f.preload[t]:(t + 1) * 160] for t in range(2, T)])
        return int((np.abs(free.astype(np.int32)) == 32767).sum())

    for fl in "fi":
        clipping = [g for g, fams in loud_inputs.groups().items() if any(clips(f, fl) > 0 for f in fams)]
        assert set(clipping) >= {"p80", "p40", "p1", "tail16"} | ({"tail0"} if fl == "f" else set())      # (the int8 model's free resonator peaks at 27692)
        for n in (8, 13):
            for g in clipping:
                arr = loud_inputs.arrangements(g, n)
                assert all(any(clips(a[s], fl) > 0 for a in arr) for s in range(n)), (g, n, fl)
    # ... and the calls it cuts directly behind a clipped sample have one to cut behind (frames 5.., not the frame's last sample)
    for fl in "fi":
        for name in ("alt80", "altrun80"):
            f = loud_inputs.by_name()[name]
            pcm = loud_golden[f"pcm_{fl}_{name}"].astype(np.int32)
            assert any(abs(pcm[t * 160 + i]) == 32767 for t in range(5, T) for i in range(f.preload[t], 159)), (fl, name)
