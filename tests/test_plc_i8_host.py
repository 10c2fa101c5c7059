"""The int8 (DOT_PROD) PLC network, the parts that need no GPU: the NumPy restatement of compute_plc_pred in the generic-C int8 build's order
(tests/tools/plc_i8_model.py) against the reference's prediction trace (tests/golden/golden_plc_i8_v1.npz), the new entry points, and what the
loader reports about int8 PLC arrays: servable beside an int8 LPCNet model, not beside a float one, rejected when hostile or truncated."""
import os
import re
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
import plc_i8_model as pq  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_i8_v1.npz"))


@pytest.fixture(scope="module")
def model_i8():
    return plc_synth.make_model_with_plc(flavour="int8")


def test_numpy_restatement_of_the_int8_plc_network_equals_the_reference(golden, model_i8):
    blob = synth.blob_bytes(model_i8)
    assert np.uint32(zlib.crc32(blob)) == golden["blob_crc"]
    net = pq.PlcNetNumpyI8(blob)
    assert (net.d1, net.g1, net.g2) == (128, 16, 16)
    mine = np.stack([net.pred(x) for x in pm.pred_inputs()])
    assert np.array_equal(mine.view(np.uint32), golden["pred"].view(np.uint32))
    # the int8 arithmetic is not the float build's: the two fixtures differ
    float_pred = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_v1.npz"))["pred"]
    assert not np.array_equal(float_pred.view(np.uint32), golden["pred"].view(np.uint32))


def test_quantisation_restated_as_in_the_reference():
    x = np.array([0.0, 1.0, -1.0, 0.5 / 127, -0.5 / 127, 1.5 / 127, -1.5 / 127, 0.999], np.float32)
    assert pq.quant_s8(x).tolist() == [0, 127, -127, 1, 0, 2, -1, 127]          # floor(.5 + t): ties go up


def test_flavour_call_is_exported_declared_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    for name in ("lpcnet_batch_plc_flavour", "lpcnet_hip_plc_model_info"):
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
    assert callable(api.LPCNetBatch.plc_flavour)


def test_an_int8_plc_network_is_present_int8_and_servable(model_i8):
    info = api.plc_model_info(synth.blob_bytes(model_i8))
    assert info == dict(present=2, servable=1, d1=128, g1=16, g2=16, nb1=32 * 6, nb2=4 * 6)
    info = api.plc_model_info(pq.blob_256_i8())
    assert (info["present"], info["servable"], info["d1"], info["g1"], info["g2"]) == (2, 1, 128, 256, 256)
    info = api.plc_model_info(pq.blob_sparse_i8())
    assert (info["present"], info["servable"]) == (2, 1) and info["nb1"] == int(pq.sparse_mask().sum())
    # the float network beside the float model, as before; no PLC arrays: nothing to serve
    info = api.plc_model_info(synth.blob_bytes(plc_synth.make_model_with_plc()))
    assert (info["present"], info["servable"]) == (1, 1)
    info = api.plc_model_info(synth.blob_bytes(synth.make_model()))
    assert (info["present"], info["servable"]) == (0, 0)


def test_mixed_flavours_are_reported_not_servable():
    info = api.plc_model_info(synth.blob_bytes(pq.model_with_plc("float", "int8")))
    assert (info["present"], info["servable"]) == (2, 0)
    info = api.plc_model_info(synth.blob_bytes(pq.model_with_plc("int8", "float")))
    assert (info["present"], info["servable"]) == (1, 0)
    # one GRU int8, the other float: inconsistent
    m = pq.model_with_plc("int8", "int8")
    plc_synth._gru(m, "plc_gru2", np.random.default_rng(2), 16, 16, "float")
    info = api.plc_model_info(synth.blob_bytes(m))
    assert (info["present"], info["servable"]) == (-1, 0)


def test_an_input_matrix_without_any_block_is_no_loadable_blob():
    """0 blocks make a 0-byte weight array, and a record of size 0 ends the reference's own loader (parse_weights, src/parse_lpcnet_weights.c:61-73:
    `ret > 0`): the whole blob is refused, as there, so a served PLC network always has at least one input block per GRU"""
    blob = synth.blob_bytes(pq.model_with_plc("int8", "int8", np.zeros((32, 6), bool)))
    assert api.check_model(blob)[0] == -1
    with pytest.raises(api.LPCNetError):
        api.plc_model_info(blob)


def test_info_entry_returns_the_named_error_codes():
    import ctypes as C
    L = api.load_library()
    info = (C.c_int * 7)()
    assert L.lpcnet_hip_plc_model_info(b"junk", 4, info) == -5 and api.last_error()
    assert L.lpcnet_hip_plc_model_info(b"junk", 4, None) == -4


def _broken(model_i8, name, edit):
    m = synth.Model(model_i8.flavour, dict(model_i8.arrays))
    arr, wtype = m.arrays[name]
    m.add(name, edit(arr.copy()), wtype)
    blob = synth.blob_bytes(m)
    assert api.check_model(blob)[0] == 0          # (the LPCNet model itself still loads: plc_enable is what reports the PLC arrays)
    return api.plc_model_info(blob)


def test_hostile_index_lists_and_truncated_int8_arrays_are_rejected_at_load(model_i8):
    def pos_beyond_the_input(idx):
        idx[1] = 128                                   # first block of GRU 1's first row group: input width is 128
        return idx

    def pos_beyond_the_input_gru2(idx):
        idx[2] = 16
        return idx

    def count_overruns(idx):
        idx[0] = idx.size                              # more blocks than the list (and the weights) hold
        return idx

    def count_one_more(idx):
        idx[0] += 1                                    # swallows the next group's count: the groups no longer add up to 3 N / 8
        return idx

    def huge_count(idx):
        idx[0] = 0x7FFFFFFF
        return idx

    for name, edit in (("plc_gru1_weights_idx", pos_beyond_the_input), ("plc_gru2_weights_idx", pos_beyond_the_input_gru2),
                       ("plc_gru1_weights_idx", count_overruns), ("plc_gru1_weights_idx", count_one_more), ("plc_gru2_weights_idx", huge_count),
                       ("plc_gru1_weights_idx", lambda idx: idx[:-1]),                       # the list ends inside a row group
                       ("plc_gru1_weights", lambda w: w[:-32]),                              # one block short of what the lists name
                       ("plc_gru1_weights", lambda w: w[:-1]),
                       ("plc_gru1_recurrent_weights", lambda r: r.reshape(-1)[:-8]),         # not 3 N N bytes
                       ("plc_gru2_recurrent_weights", lambda r: r.reshape(-1)[:3 * 16 * 16 // 2]),
                       ("plc_gru2_bias", lambda b: b.reshape(-1)[:-4])):                     # the width no longer a multiple of 8
        info = _broken(model_i8, name, edit)
        assert (info["present"], info["servable"]) == (-1, 0), (name, edit.__name__, info)


def test_widths_beyond_the_kernel_limit_are_rejected():
    m = synth.make_model(flavour="int8")
    rng = np.random.default_rng(3)
    m.add("plc_dense1_weights", np.zeros((57, 128), np.float32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", np.zeros(128, np.float32), synth.WEIGHT_TYPE_FLOAT)
    pq.add_gru_i8(m, "plc_gru1", rng, 128, 520)
    pq.add_gru_i8(m, "plc_gru2", rng, 520, 16)
    m.add("plc_out_weights", np.zeros((16, 20), np.float32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_out_bias", np.zeros(20, np.float32), synth.WEIGHT_TYPE_FLOAT)
    assert api.plc_model_info(synth.blob_bytes(m))["present"] == -1


def test_sparse_test_blob_has_an_empty_a_single_and_irregular_row_groups():
    a = pm.blob_arrays(pq.blob_sparse_i8())
    counts = pq.group_counts(np.frombuffer(a["plc_gru1_weights_idx"], np.int32), 6)
    assert counts[0] == 0 and counts[1] == 1 and len(set(counts[2:])) == 4 and all(0 < c < 32 for c in counts[2:]), counts
