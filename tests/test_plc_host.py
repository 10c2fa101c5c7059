"""Batched packet-loss concealment, the parts that need no GPU: the exported interface, the refusals of lpcnet_batch_plc_enable, the host
planner against the control flow restated from the reference (tests/tools/plc_model.py, recorded in tests/golden/golden_plc_v1.npz), the NumPy
restatement of compute_plc_pred against the reference's prediction traces, and the new kernels' resources."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

SYMBOLS = ("lpcnet_batch_plc_enable", "lpcnet_batch_plc_reset", "lpcnet_batch_plc_step", "lpcnet_batch_plc_step_device", "lpcnet_batch_plc_step_device_shard",
           "lpcnet_batch_plc_fec_add", "lpcnet_batch_plc_fec_clear", "lpcnet_batch_plc_state_size", "lpcnet_batch_get_plc_state", "lpcnet_batch_set_plc_state",
           "lpcnet_batch_plc_burg", "lpcnet_batch_plc_pred", "lpcnet_hip_plc_plan")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_v1.npz"))


def test_symbols_are_exported_declared_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
    for m in ("plc_enable", "plc_step", "plc_step_device", "plc_reset", "plc_fec_add", "plc_fec_clear", "get_plc_state", "set_plc_state", "plc_burg", "plc_pred"):
        assert callable(getattr(api.LPCNetBatch, m)), m
    assert L.lpcnet_batch_plc_state_size() > 560 * 2 + 100 * 20 * 4


def test_calls_on_a_batch_without_a_model_fail_with_a_message():
    L = api.load_library()
    L.lpcnet_batch_create.restype = C.c_void_p
    b = L.lpcnet_batch_create(2, 0)
    assert b
    try:
        pcm = np.zeros((2, 160), np.int16)
        lost = np.zeros(2, np.uint8)
        for rc in (L.lpcnet_batch_plc_enable(b, 0), L.lpcnet_batch_plc_step(b, pcm, lost), L.lpcnet_batch_plc_reset(b, 0, 2), L.lpcnet_batch_plc_fec_clear(b, 0)):
            assert rc == -5 and api.last_error()
    finally:
        L.lpcnet_batch_destroy(b)


def test_planner_refuses_the_non_causal_mode_and_bad_state():
    ctl = np.zeros((1, 9), np.int32)
    ctl[0, 0] = 400
    with pytest.raises(api.LPCNetError):
        api.plc_plan(api.PLC_NONCAUSAL, ctl, [0])
    ctl[0, 0] = 123                                   # not a fill the state machine can reach
    with pytest.raises(api.LPCNetError):
        api.plc_plan(api.PLC_CAUSAL, ctl, [1])


def test_model_parse_reports_the_plc_network():
    L = api.load_library()
    # (the layout entry parses the blob: a blob with and without the PLC arrays, and an int8 one, all still load as LPCNet models)
    for blob in (synth.blob_bytes(synth.make_model()), synth.blob_bytes(plc_synth.make_model_with_plc()), pm.blob_256(),
                 synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))):
        out = (C.c_int * 65)()
        assert L.lpcnet_hip_model_layout(blob, len(blob), out) == 0


def _run_planner(options, lost, ops=None):
    n, T = lost.shape
    ctl = np.zeros((n, 9), np.int32)
    ctl[:, 0] = 400
    out = np.zeros((T, n, 10), np.int32)
    for t in range(T):
        op = None if ops is None else ops[t]
        out[t] = api.plc_plan(options, ctl, lost[:, t], op)
    return out


def test_planner_follows_the_reference_control_flow(golden):
    lost = pm.loss_patterns()
    for k, opt in enumerate(pm.OPTION_SETS):
        got = _run_planner(opt, lost)
        assert np.array_equal(got, golden["summary"][k % 2]), "options %d" % opt          # (the DC filter does not change the control flow)
    # what the patterns must have exercised: three queue rounds, the attenuation beyond ten lost frames, both first-frame paths
    sm = golden["summary"]
    assert sm[0, :, :, 2].max() == 3 and sm[0, :, :, 9].max() >= 15 and (sm[0, :, :, 5] == 1).any() and (sm[1, :, :, 5] == 2).any()


def test_planner_follows_the_fec_bookkeeping(golden):
    ops, _ = pm.fec_schedule()
    got = _run_planner(0, pm.fec_loss_patterns(), ops)
    assert np.array_equal(got, golden["fec_summary"])
    assert golden["fec_summary"][..., 4].sum() > 50


def test_python_control_restatement_is_what_the_fixture_records(golden):
    lost = pm.loss_patterns()
    for k, opt in enumerate(pm.OPTION_SETS):
        for s in (0, 3, 6, 7, 20):
            c = pm.PlcControl(opt)
            assert np.array_equal(np.array([c.step(int(x)) for x in lost[s]]), golden["summary"][k % 2][:, s])


def test_numpy_restatement_of_the_plc_network_equals_the_reference(golden):
    blob = synth.blob_bytes(plc_synth.make_model_with_plc())
    import zlib
    assert np.uint32(zlib.crc32(blob)) == golden["blob_crc"]
    net = pm.PlcNetNumpy(blob)
    assert (net.d1, net.g1, net.g2) == (128, 16, 16)
    mine = np.stack([net.pred(x) for x in pm.pred_inputs()])
    assert np.array_equal(mine.view(np.uint32), golden["pred"].view(np.uint32))


def test_generated_plc_tables_are_in_sync_and_correctly_rounded():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_tables
    text = open(os.path.join(ROOT, "lpcnet_amd", "csrc", "lpcnet_plc_tables_gen.h")).read()
    body = re.search(r"lpcn_plc_pow995\[16\] = \{(.*?)\};", text, re.S).group(1)
    vals = np.array([float.fromhex(x) for x in re.findall(r"0x[0-9a-fp.+-]+", body)])
    assert np.array_equal(vals, gen_tables.plc_pow995()) and vals[0] == 0.995 and vals[15] == 0.995 ** 16
    body = re.search(r"lpcn_plc_fade\[80\] = \{(.*?)\};", text, re.S).group(1)
    w = np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fp.+-]+f", body)], np.float32)
    assert np.array_equal(w, gen_tables.plc_fade_window()) and w[0] == 0 and w[40] == 0.5
