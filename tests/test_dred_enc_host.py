"""The DRED encoder, the parts that need no GPU: what the loader reports about a blob's encoder arrays (lpcnet_hip_dred_enc_model_info), the new
entry points (declared, exported, bound), and the NumPy restatement of dred_rdovae_encode_dframe (tests/tools/dred_enc_model.py: DredEncNumpy)
against the reference's output (tests/golden/golden_dred_enc_v1.npz, made by tests/tools/make_golden_dred_enc.py)."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_enc_model as em  # noqa: E402
import dred_model as dm  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

C_NAMES = ("lpcnet_hip_dred_enc_model_info", "lpcnet_batch_dred_enc_enable", "lpcnet_batch_dred_enc_info", "lpcnet_batch_dred_encode",
           "lpcnet_batch_dred_encode_device", "lpcnet_batch_dred_encode_device_shard", "lpcnet_batch_dred_enc_get_state",
           "lpcnet_batch_dred_enc_set_state", "lpcnet_batch_dred_enc_set_form", "lpcnet_batch_dred_enc_get_form")
NARROW = em.SETS["narrow"]
NONE = dict(present=0, servable=0, latent_dim=0, state_dim=0, taps=0, gdense1=0, state_floats=0, widths=[0] * 8)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_v1.npz"))


def info_of(blob):
    assert api.check_model(blob)[0] == 0          # (the LPCNet model itself loads: dred_enc_enable is what reports the encoder's arrays)
    return api.dred_enc_model_info(blob)


def narrow_kw(**kw):
    return dict(dict(taps=NARROW["taps"], latent_dim=NARROW["latent_dim"], gdense1=NARROW["gdense1"], state_dim=NARROW["state_dim"]), **kw)


def edited(name, edit):
    """the narrow encoder with one array replaced (edit returns the new array) or dropped (edit is None)"""
    m = em.add_dred_enc(synth.make_model(), NARROW["widths"], **narrow_kw())
    if edit is None:
        del m.arrays[name]
    else:
        arr, wtype = m.arrays[name]
        m.add(name, edit(arr.copy()), wtype)
    return synth.blob_bytes(m)


def expected(s):
    w = list(s["widths"])
    return dict(present=1, servable=1, latent_dim=s["latent_dim"], state_dim=s["state_dim"], taps=s["taps"], gdense1=s["gdense1"],
                state_floats=w[1] + w[3] + w[5] + (s["taps"] - 1) * sum(w), widths=w)


def test_a_blob_without_encoder_arrays_reports_none(blob_f32):
    assert info_of(blob_f32) == NONE
    assert info_of(dm.set_blob("small")) == NONE          # (a decoder alone is no encoder)


@pytest.mark.parametrize("name", list(em.SETS))
def test_the_three_width_sets_are_float_and_servable(name):
    assert info_of(em.set_blob(name)) == expected(em.SETS[name])
    assert expected(em.SETS["tf"])["state_floats"] == 3 * 128 + 3 * 1408          # (the conv memory: 16.9 KB at the training defaults)


def test_int8_mixed_and_float_beside_an_int8_model():
    w = NARROW["widths"]
    info = info_of(em.blob_enc(w, **narrow_kw(gru_flavour="int8")))
    assert (info["present"], info["servable"], info["widths"]) == (2, 0, list(w))
    assert info_of(em.blob_enc(w, **narrow_kw(gru_flavour=("float", "int8", "float"))))["present"] == -1
    blob = synth.blob_bytes(em.add_dred_enc(synth.make_model(flavour="int8"), w, **narrow_kw()))
    info = info_of(blob)
    assert (info["present"], info["servable"]) == (1, 0)


@pytest.mark.parametrize("name", ["enc_dense5_bias", "enc_dense4_recurrent_weights", "enc_dense2_weights_idx", "enc_dense6_subias", "bits_dense_weights",
                                  "bits_dense_bias", "gdense1_weights", "gdense2_bias"])
def test_one_array_missing_is_incomplete(name):
    info = info_of(edited(name, None))
    assert (info["present"], info["servable"]) == (-1, 0), info


def test_a_width_of_264_is_beyond_the_kernel_limit():
    assert info_of(em.blob_enc((256, 128, 264, 128, 256, 128, 128, 128)))["present"] == -1
    assert info_of(em.blob_enc((256, 264, 256, 128, 256, 128, 128, 128)))["present"] == -1
    assert info_of(em.blob_enc((256,) * 8, latent_dim=264))["present"] == -1
    assert info_of(em.blob_enc((256,) * 8, gdense1=264))["present"] == -1


def test_taps_must_be_integral_and_between_one_and_eight():
    total = sum(NARROW["widths"])
    assert info_of(em.blob_enc(NARROW["widths"], **narrow_kw(bits_rows=3 * total - 1)))["present"] == -1          # K not integral
    assert info_of(em.blob_enc(NARROW["widths"], **narrow_kw(bits_rows=3 * total + total // 2)))["present"] == -1
    assert info_of(em.blob_enc(NARROW["widths"], **narrow_kw(taps=9)))["present"] == -1
    for k in (1, 8):
        assert info_of(em.blob_enc(NARROW["widths"], **narrow_kw(taps=k)))["taps"] == k


def test_enc_dense1_with_36_inputs_is_refused():
    assert info_of(em.blob_enc(NARROW["widths"], **narrow_kw(in_dim=36)))["present"] == -1


def test_sizes_that_do_not_fit_together_are_inconsistent():
    for name, edit in (("enc_dense3_bias", lambda b: b[:-1]),                      # a bias length that does not match its matrix
                       ("enc_dense2_bias", lambda b: b.reshape(-1)[:-6]),           # a GRU width that is no multiple of 8
                       ("gdense1_weights", lambda w: w[:-1]),                       # gdense1 does not take the whole buffer
                       ("gdense2_weights", lambda w: w[:-1])):
        info = info_of(edited(name, edit))
        assert (info["present"], info["servable"]) == (-1, 0), (name, info)


def test_arrays_placed_before_the_lpcnet_arrays_load_the_same():
    front, back = em.set_blob("narrow", first=True), em.set_blob("narrow")
    names = lambda blob: list(em.pm.blob_arrays(blob))
    assert names(front)[0] == "enc_dense1_weights" and names(back)[0] != "enc_dense1_weights" and sorted(names(front)) == sorted(names(back))
    assert info_of(front) == info_of(back) == expected(NARROW)


def test_the_decoders_info_is_unchanged_by_the_encoders_presence():
    both = em.set_blob("tf", with_dec=True)
    assert api.dred_model_info(both) == api.dred_model_info(dm.set_blob("mixed"))
    assert info_of(both) == expected(em.SETS["tf"])


def test_info_entry_returns_the_named_error_codes():
    import ctypes as C
    L = api.load_library()
    info = (C.c_int * 15)()
    assert L.lpcnet_hip_dred_enc_model_info(b"junk", 4, info) == -5 and api.last_error()
    assert L.lpcnet_hip_dred_enc_model_info(b"junk", 4, None) == -4


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
    for name in ("dred_enc_enable", "dred_enc_info", "dred_encode", "dred_encode_device", "dred_enc_form", "get_dred_enc_state", "set_dred_enc_state"):
        assert callable(getattr(api.LPCNetBatch, name)), name


def test_numpy_restatement_equals_the_reference_without_the_compiled_reference(golden):
    """the narrow set whole (every stream, states included); the training defaults on the two shortest streams, whose windows still hold zeros"""
    feat = em.inputs()
    assert np.uint32(zlib.crc32(feat.tobytes())) == golden["in_crc"]
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    net = em.DredEncNumpy(em.set_blob("narrow"))
    lat, init, states = net.encode_all(feat, em.COUNT)
    assert np.array_equal(bits(lat), bits(golden["lat_narrow"])) and np.array_equal(bits(init), bits(golden["init_narrow"]))
    assert np.array_equal(bits(states[:, :net.gru_floats]), bits(golden["gru_narrow"]))
    assert em.mem_crc(states, net.gru_floats).tolist() == golden["mem_crc_narrow"].tolist()
    assert np.array_equal(bits(states[0, net.gru_floats:]), bits(golden["mem_full_narrow"]))
    net = em.DredEncNumpy(em.set_blob("tf"))
    for s in (1, 3):
        c = int(em.COUNT[s])
        st = net.fresh()
        lat, init = net.encode(st, feat[s], c)
        assert c < net.taps and np.array_equal(bits(lat), bits(golden["lat_tf"][s, :c])) and np.array_equal(bits(init), bits(golden["init_tf"][s, :c]))
        assert np.array_equal(bits(st[:net.gru_floats]), bits(golden["gru_tf"][s])) and zlib.crc32(st[net.gru_floats:].tobytes()) == golden["mem_crc_tf"][s]


def test_fixture_crcs_match_the_seeded_generators(golden):
    for name in em.SETS:
        assert np.uint32(zlib.crc32(em.set_blob(name))) == golden["blob_crc_" + name], name
        s = em.SETS[name]
        assert golden["lat_" + name].shape == (em.N_STREAMS, em.N_DFRAMES, s["latent_dim"]) and golden["init_" + name].shape == (em.N_STREAMS, em.N_DFRAMES, s["state_dim"])
    assert np.uint32(zlib.crc32(em.set_blob("tf", with_dec=True))) == golden["blob_crc_rt"]
    assert np.uint32(zlib.crc32(em.long_inputs().tobytes())) == golden["long_in_crc"]
    s = em.LONG_FULL_STREAM
    assert golden["long_crc"].shape == (em.LONG_STREAMS,) and golden["long_lat"].shape == (em.LONG_DFRAMES, 80)
    assert golden["long_crc"][s] == zlib.crc32(golden["long_lat"][:int(em.LONG_COUNT[s])].tobytes() + golden["long_init"][:int(em.LONG_COUNT[s])].tobytes())
    assert golden["rt_feat"].shape == (len(em.RT_STREAMS), 4 * em.N_DFRAMES, 20)
    for name in ("lat_tf", "init_tf", "rt_feat"):
        assert np.isfinite(golden[name]).all()
