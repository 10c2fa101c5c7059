"""The PLC prediction kernels over the widths the loader admits (d1 a multiple of 4, g1 and g2 multiples of 8, each up to 512), against their NumPy
restatements: plc_model.PlcNetNumpy for plc_pred_kernel, plc_i8_model.PlcNetNumpyI8 for plc_pred_i8_kernel.  The fixtures tie both restatements to
the reference at 128 / 16 / 16 (tests/test_plc_host.py, tests/test_plc_i8_host.py); the reference has no build at other widths.  All 20 outputs of
every step are compared bit pattern for bit pattern.

  (4, 8, 8)        the minimum: one input block per row group, a GRU of 8 units on 256 lanes
  (512, 512, 512)  the maximum: two full passes of units, 1536 gate rows, 128 input blocks per row group
  (64, 264, 24)    eight units in the second pass, 792 rows, g1 > g2, d1 != 128
  (128, 512, 264)  the width the int8 kernel already ran (tests/test_gpu_plc_i8.py), new for the float one
  (8, 8, 40)       g2 > 3 g1: a stream's network state (g1 + g2 floats) is longer than 4 g1, so a state stride that forgets g2 makes neighbouring
                   streams' states overlap within the prediction steps themselves
and at (64, 264, 24) and (512, 512, 512) also with input matrices that keep about 30 % of their blocks and have row groups without any.

Every stream of a batch gets its OWN input trace, so an offset into the per-stream network state (stride 4 (g1 + g2) floats) or the per-stream
inputs that is wrong by a stream shows.  Two more slots repeat stream 0: after the prediction steps the whole PLC step runs on the batch with
mixed loss flags, and the slots that were given the same inputs must give the same PCM."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_i8_model as pq  # noqa: E402
from lpcnet_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

N = 5                                                  # streams with a trace of their own; slots N and N + 1 repeat stream 0
CASES = [((4, 8, 8), None), ((512, 512, 512), None), ((64, 264, 24), None), ((128, 512, 264), None), ((8, 8, 40), None), ((64, 264, 24), 0.3), ((512, 512, 512), 0.3)]


@pytest.mark.parametrize("widths,density", CASES, ids=["%d-%d-%d%s" % (w + (("-sparse",) if d else ("",))) for w, d in CASES])
@pytest.mark.parametrize("flavour", ["float", "int8"])
def test_prediction_equals_the_restatement_and_the_step_runs(flavour, widths, density, hip_lib):
    d1, g1, g2 = widths
    blob = pm.blob_widths(d1, g1, g2, flavour, block_density=density)
    if density:                                        # about 30 % of the blocks, and in each GRU at least one row group without any
        a = pm.blob_arrays(blob)
        for name, n_in, n in (("plc_gru1", d1, g1), ("plc_gru2", g1, g2)):
            counts = pm.group_counts(np.frombuffer(a[name + "_weights_idx"], np.int32), 3 * n // 8)
            assert counts.count(0) >= 1 and 0.2 < sum(counts) / (n_in // 4 * len(counts)) < 0.4, (name, counts)
    info = api.plc_model_info(blob)
    assert (info["servable"], info["d1"], info["g1"], info["g2"]) == (1, d1, g1, g2)
    steps = 8 if g1 == 512 else 16
    xs = np.stack([pm.pred_inputs(steps, seed=[0x9ED, s]) for s in range(N)])          # [N][steps][57]
    assert not np.array_equal(xs[0], xs[1])
    want = pq.pred_traces(blob, flavour == "int8", xs)                                  # [N][steps][20]
    slots = list(range(N)) + [0, 0]
    b = api.LPCNetBatch(len(slots), blob)
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_flavour() == (flavour == "int8")
    got = np.stack([b.plc_pred(xs[slots, t]) for t in range(steps)])                    # [steps][slots][20]
    for i, s in enumerate(slots):
        bad = np.argwhere(got[:, i].view(np.uint32) != want[s].view(np.uint32))
        assert bad.size == 0, "%s %s slot %d (trace %d): first differing (step, feature) %s of %d" % (flavour, widths, i, s, bad[:4].tolist(), len(bad))
    assert np.isfinite(got).all() and len({got[-1, i].tobytes() for i in range(N)}) == N
    # the whole step on that network and those network states: received frames, then losses on some streams, then the recovery
    pcm = np.stack([pm.stream_pcm(s, 6) for s in slots])
    lost = np.zeros((len(slots), 6), np.uint8)
    lost[[0, 2, 3], 2:4] = 1
    lost[[1, 3], 4] = 1
    lost[N:] = lost[0]
    out = np.zeros((len(slots), 6, 160), np.int16)
    for t in range(6):
        frame = np.ascontiguousarray(pcm[:, t])
        frame[lost[:, t] != 0] = 0
        out[:, t] = b.plc_step(frame, lost[:, t])
    b.close()
    bad = np.argwhere(out[N:] != out[0])
    assert bad.size == 0, "%s %s: slots %d and %d were given slot 0's inputs: first differing (slot - %d, frame, sample) %s of %d" % (flavour, widths, N, N + 1, N, bad[:4].tolist(), len(bad))
