"""The DRED decoder, the parts that need no GPU: what the loader reports about a blob's decoder arrays (lpcnet_hip_dred_model_info), the new
entry points (declared, exported, bound), and the NumPy restatement of DRED_rdovae_decode_all (tests/tools/dred_model.py: DredDecNumpy) against
the reference's output (tests/golden/golden_dred_v1.npz, made by tests/tools/make_golden_dred.py)."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_model as dm  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

C_NAMES = ("lpcnet_hip_dred_model_info", "lpcnet_batch_dred_enable", "lpcnet_batch_dred_decode", "lpcnet_batch_dred_decode_device",
           "lpcnet_batch_dred_decode_device_shard", "lpcnet_batch_dred_decode_packed_device", "lpcnet_batch_dred_decode_packed_device_shard",
           "lpcnet_batch_dred_info", "lpcnet_batch_dred_set_form", "lpcnet_batch_dred_get_form")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_v1.npz"))


def info_of(blob):
    assert api.check_model(blob)[0] == 0          # (the LPCNet model itself loads: dred_enable is what reports the decoder's arrays)
    return api.dred_model_info(blob)


def edited(name, edit, widths=dm.SETS["small"]["widths"], latent_dim=36):
    """the small decoder with one array replaced (edit returns the new array) or dropped (edit is None)"""
    m = dm.add_dred(synth.make_model(), widths, latent_dim)
    if edit is None:
        del m.arrays[name]
    else:
        arr, wtype = m.arrays[name]
        m.add(name, edit(arr.copy()), wtype)
    return synth.blob_bytes(m)


def test_a_blob_without_decoder_arrays_reports_none_and_loads_as_before(blob_f32):
    assert info_of(blob_f32) == dict(present=0, servable=0, latent_dim=0, state_dim=0, widths=[0] * 8)


@pytest.mark.parametrize("name", list(dm.SETS))
def test_the_three_width_sets_are_float_and_servable(name):
    s = dm.SETS[name]
    assert info_of(dm.set_blob(name)) == dict(present=1, servable=1, latent_dim=s["latent_dim"], state_dim=dm.STATE_DIM, widths=list(s["widths"]))


def test_decoder_arrays_beside_the_plc_network_load_too():
    s = dm.SETS["mixed"]
    blob = dm.set_blob("mixed", with_plc=True)
    assert info_of(blob)["widths"] == list(s["widths"]) and api.plc_model_info(blob)["present"] == 1


@pytest.mark.parametrize("name", ["dec_dense5_bias", "dec_dense4_recurrent_weights", "dec_dense2_weights_idx", "dec_dense6_subias", "state2_weights", "dec_final_weights"])
def test_one_array_dropped_is_incomplete(name):
    info = info_of(edited(name, None))
    assert (info["present"], info["servable"]) == (-1, 0), info


def test_sizes_that_do_not_fit_together_are_inconsistent():
    for name, edit in (("dec_dense3_bias", lambda b: b[:-1]),                      # a bias length that does not match its matrix
                       ("dec_dense2_bias", lambda b: b.reshape(-1)[:-6]),           # a GRU width that is no multiple of 8
                       ("dec_dense4_recurrent_weights", lambda r: r.reshape(-1)[:-1]),
                       ("state3_bias", lambda b: b[:-1]),                           # state3 no longer as wide as its GRU
                       ("dec_final_weights", lambda w: w[:-1]),                     # dec_final does not take the whole buffer
                       ("dec_dense2_weights_idx", lambda i: np.concatenate([[i.size], i[1:]]).astype(np.int32))):
        info = info_of(edited(name, edit))
        assert (info["present"], info["servable"]) == (-1, 0), (name, info)


def test_a_width_of_264_is_beyond_the_kernel_limit():
    assert info_of(dm.blob_dred((256, 128, 264, 128, 256, 128, 128, 128)))["present"] == -1
    assert info_of(dm.blob_dred((256, 264, 256, 128, 256, 128, 128, 128)))["present"] == -1
    assert info_of(dm.blob_dred((256,) * 8, latent_dim=260))["present"] == -1


def test_dec_final_with_60_outputs_is_refused():
    assert info_of(dm.blob_dred(dm.SETS["small"]["widths"], 36, final_out=60))["present"] == -1


def test_int8_arrays_are_reported_and_not_servable():
    w = dm.SETS["small"]["widths"]
    info = info_of(dm.blob_dred(w, 36, gru_flavour="int8"))
    assert (info["present"], info["servable"], info["widths"]) == (2, 0, list(w))
    assert info_of(dm.blob_dred(w, 36, gru_flavour=("float", "int8", "float")))["present"] == -1      # a mix of float and int8 GRUs
    # float decoder arrays beside an int8 LPCNet model: present, not served
    blob = synth.blob_bytes(dm.add_dred(synth.make_model(flavour="int8"), w, 36))
    info = info_of(blob)
    assert (info["present"], info["servable"]) == (1, 0)


def test_info_entry_returns_the_named_error_codes():
    import ctypes as C
    L = api.load_library()
    info = (C.c_int * 12)()
    assert L.lpcnet_hip_dred_model_info(b"junk", 4, info) == -5 and api.last_error()
    assert L.lpcnet_hip_dred_model_info(b"junk", 4, None) == -4


def test_new_names_are_declared_exported_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name in C_NAMES:
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
        assert name in exported, name
    assert not [s for s in exported if s.startswith("lpcn_")]
    assert not [s for s in exported if s.startswith("DRED_rdovae")]
    for name in ("dred_enable", "dred_decode", "dred_decode_device", "dred_decode_packed", "dred_form"):
        assert callable(getattr(api.LPCNetBatch, name)), name
    assert callable(api.dred_model_info)
    assert "No per-stream state" in header


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_numpy_restatement_equals_the_reference(name, golden):
    blob = dm.set_blob(name)
    state, latents = dm.set_inputs(name)
    assert np.uint32(zlib.crc32(blob)) == golden["blob_crc_" + name]
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == golden["in_crc_" + name]
    net = dm.DredDecNumpy(blob)
    assert net.widths == list(dm.SETS[name]["widths"]) and (net.latent_dim, net.state_dim) == (dm.SETS[name]["latent_dim"], dm.STATE_DIM)
    mine = net.decode_all(state, latents, dm.COUNT)
    want = golden["feat_" + name]
    assert want.shape == (dm.N_STREAMS, 4 * dm.N_LATENTS, 20)
    assert np.array_equal(mine.view(np.uint32), want.view(np.uint32))


def test_fixture_shapes_and_the_packed_permutation(golden):
    assert golden["long_crc"].shape == (dm.LONG_STREAMS,) and golden["long_full"].shape == (4 * dm.LONG_LATENTS, 20)
    assert golden["long_crc"][dm.LONG_FULL_STREAM] == zlib.crc32(golden["long_full"][:4 * int(dm.LONG_COUNT[dm.LONG_FULL_STREAM])].tobytes())
    feat = golden["feat_small"]
    first, take = np.array([0, 1, 0, 3, 27, 0, 5, 0, 15]), np.array([28, 2, 0, 5, 1, 0, 20, 20, 1])
    p = dm.packed(feat, first, take)
    assert p.shape == (int(take.sum()), 20)
    assert np.array_equal(p[0], feat[0, 27]) and np.array_equal(p[27], feat[0, 0]) and np.array_equal(p[28], feat[1, 2]) and np.array_equal(p[29], feat[1, 1])
