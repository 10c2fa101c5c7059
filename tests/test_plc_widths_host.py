"""The width range of the PLC network, the parts that need no GPU: what the loader reports at the edges of the admitted widths (d1 a multiple of 4,
g1 and g2 multiples of 8, each up to 512, both GRUs of one flavour), and the proof that the width / density arguments added to the test blob
builders (tests/tools/plc_model.py: blob_widths, pred_inputs(seed); tests/tools/plc_synth.py: _gru(block_density)) left every earlier blob and
input trace byte for byte what it was."""
import os
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


def test_earlier_blobs_and_input_traces_keep_their_bytes():
    """CRC-32 of every blob the PLC tests built before the builders took widths and a block density (the first two are also what the fixtures
    record as blob_crc), and of the default prediction input trace"""
    gold_f = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_v1.npz"))
    gold_i = np.load(os.path.join(ROOT, "tests", "golden", "golden_plc_i8_v1.npz"))
    crc = lambda b: zlib.crc32(b)
    assert crc(synth.blob_bytes(plc_synth.make_model_with_plc())) == 0x77EF09E2 == int(gold_f["blob_crc"])
    assert crc(synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))) == 0x55180856 == int(gold_i["blob_crc"])
    assert crc(pm.blob_256()) == 0x2CFDD834
    assert crc(pq.blob_256_i8()) == 0x3F376407
    assert crc(pq.blob_wide_i8()) == 0x5FEFFF70
    assert crc(pq.blob_sparse_i8()) == 0x49D8E477
    assert crc(pm.pred_inputs().tobytes()) == 137340136
    # the generalised builder at the earlier widths is the earlier builder
    assert crc(pm.blob_widths(128, 256, 256, "int8")) == 0x3F376407
    assert crc(pm.blob_widths(128, 512, 264, "int8", seed=778)) == 0x5FEFFF70
    # and a seed of its own gives another trace of the same form
    x = pm.pred_inputs(16, seed=[0x9ED, 3])
    assert x.shape == (16, 57) and not x[::5, :56].any() and not np.array_equal(x, pm.pred_inputs(16))


@pytest.mark.parametrize("widths", [(4, 8, 8), (512, 512, 512), (64, 264, 24), (128, 512, 264), (8, 8, 40)])
@pytest.mark.parametrize("flavour", ["float", "int8"])
def test_admitted_widths_are_present_and_servable(flavour, widths):
    info = api.plc_model_info(pm.blob_widths(*widths, flavour))
    d1, g1, g2 = widths
    assert info == dict(present=2 if flavour == "int8" else 1, servable=1, d1=d1, g1=g1, g2=g2, nb1=d1 // 4 * (3 * g1 // 8), nb2=g1 // 4 * (3 * g2 // 8))


@pytest.mark.parametrize("widths", [(64, 264, 24), (512, 512, 512)])
def test_block_density_thins_the_lists_and_empties_row_groups(widths):
    d1, g1, g2 = widths
    a = pm.blob_arrays(pm.blob_widths(*widths, block_density=0.3))
    for name, n_in, n in (("plc_gru1", d1, g1), ("plc_gru2", g1, g2)):
        counts = pm.group_counts(np.frombuffer(a[name + "_weights_idx"], np.int32), 3 * n // 8)
        assert counts.count(0) >= 1 and 0.2 < sum(counts) / (n_in // 4 * len(counts)) < 0.4, (name, counts)
        assert np.array_equal(np.array(counts), plc_synth.block_mask(n_in, n, 0.3).sum(axis=0))
    info = api.plc_model_info(pm.blob_widths(*widths, "int8", block_density=0.3))
    assert (info["present"], info["servable"]) == (2, 1) and info["nb1"] == int(plc_synth.block_mask(d1, g1, 0.3).sum())


def _mixed_gru_flavours():
    m = synth.make_model()
    rng = np.random.default_rng(7)
    m.add("plc_dense1_weights", np.zeros((57, 128), np.float32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", np.zeros(128, np.float32), synth.WEIGHT_TYPE_FLOAT)
    plc_synth._gru(m, "plc_gru1", rng, 128, 16, "int8")
    plc_synth._gru(m, "plc_gru2", rng, 16, 16, "float")
    m.add("plc_out_weights", np.zeros((16, 20), np.float32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_out_bias", np.zeros(20, np.float32), synth.WEIGHT_TYPE_FLOAT)
    return synth.blob_bytes(m)


@pytest.mark.parametrize("case", ["g1=520", "d1=516", "d1=6", "g2=12", "g1 int8, g2 float"])
def test_widths_outside_the_admitted_range_are_reported_invalid(case):
    """one step beyond each limit: the LPCNet model of the blob still loads, its PLC network is reported invalid and not servable"""
    blob = {"g1=520": lambda: pm.blob_widths(128, 520, 16), "d1=516": lambda: pm.blob_widths(516, 16, 16), "d1=6": lambda: pm.blob_widths(6, 16, 16),
            "g2=12": lambda: pm.blob_widths(128, 16, 12), "g1 int8, g2 float": _mixed_gru_flavours}[case]()
    assert api.check_model(blob)[0] == 0
    info = api.plc_model_info(blob)
    assert (info["present"], info["servable"]) == (-1, 0), info
