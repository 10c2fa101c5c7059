"""The DRED decoder's per-stream state at the C boundary, without a GPU: include/lpcnet_batch.h declares the entry points of
lpcnet_batch_dred_state_enable / dred_init / dred_step, the built library exports them, lpcnet_amd/api.py gives them argument types, and a batch
without a model is refused by every one of them."""
import ctypes as C
import os
import re
import subprocess

from lpcnet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i, fp = C.c_void_p, C.c_int, api._f32p
# name -> the argument types api.py must set (the batch first)
ENTRY = {
    "lpcnet_batch_dred_state_enable": [vp],
    "lpcnet_batch_dred_dec_state_size": [vp],
    "lpcnet_batch_get_dred_dec_state": [vp, i, fp],
    "lpcnet_batch_set_dred_dec_state": [vp, i, fp],
    "lpcnet_batch_dred_init": [vp, fp, vp],
    "lpcnet_batch_dred_init_device": [vp, vp, vp, vp],
    "lpcnet_batch_dred_init_device_shard": [vp, i, vp, vp, vp],
    "lpcnet_batch_dred_step": [vp, fp, vp, vp, fp],
    "lpcnet_batch_dred_step_device": [vp, vp, vp, vp, i, i, vp, vp],
    "lpcnet_batch_dred_step_device_shard": [vp, i, vp, vp, vp, i, i, vp, vp],
    "lpcnet_batch_dred_step_packed_device": [vp, vp, vp, vp, vp, vp, vp, vp],
    "lpcnet_batch_dred_step_packed_device_shard": [vp, i, vp, vp, vp, vp, vp, vp, vp],
}


def test_header_declares_every_entry_point():
    text = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, args in ENTRY.items():
        m = re.search(r"LPCNET_EXPORT\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(args) and re.match(r"(const\s+)?LPCNetBatch\s*\*\s*b$", params[0]), (name, params)
        for p, t in zip(params[1:], args[1:]):
            assert (t is i) == bool(re.match(r"int\s+\w+$", p)), (name, p)          # (ints by value where the binding passes ints, pointers elsewhere)
    assert re.search(r"#define\s+LPCNET_SNAP_DRED_DEC\s+21\b", text)
    # the sentence that said the pair does not exist is gone
    assert "not exposed" not in open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read().replace("\n *", "")


def test_library_exports_every_symbol(hip_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in ENTRY:
        assert n in exported, n
    assert not [s for s in exported if s.startswith("lpcn_")]      # (the engine's own entry points stay inside)


def test_python_binding_sets_the_argument_types(hip_lib):
    for name, args in ENTRY.items():
        assert getattr(hip_lib, name).argtypes == args, name
    for method in ("dred_state_enable", "dred_dec_state_size", "get_dred_dec_state", "set_dred_dec_state", "dred_init", "dred_init_device", "dred_step",
                   "dred_step_device", "dred_step_packed"):
        assert callable(getattr(api.LPCNetBatch, method)), method
    assert api.SNAP_SECTIONS[-1] == "DRED_DEC" and api.SNAP["DRED_DEC"] == 21 and api.SNAP["DRED_ENC"] == 20


def test_a_batch_without_a_model_is_refused_not_crashed(hip_lib):
    """NULL batch: every entry point answers LPCNET_HIP_E_MODEL with a message -- no device is touched"""
    import numpy as np
    f = np.zeros(4, np.float32)
    calls = {
        "lpcnet_batch_dred_state_enable": (), "lpcnet_batch_dred_dec_state_size": (), "lpcnet_batch_get_dred_dec_state": (0, f),
        "lpcnet_batch_set_dred_dec_state": (0, f), "lpcnet_batch_dred_init": (f, None), "lpcnet_batch_dred_init_device": (None, None, None),
        "lpcnet_batch_dred_init_device_shard": (0, None, None, None), "lpcnet_batch_dred_step": (f, None, None, f),
        "lpcnet_batch_dred_step_device": (None, None, None, 0, 1, None, None), "lpcnet_batch_dred_step_device_shard": (0, None, None, None, 0, 1, None, None),
        "lpcnet_batch_dred_step_packed_device": (None, None, None, None, None, None, None),
        "lpcnet_batch_dred_step_packed_device_shard": (0, None, None, None, None, None, None, None),
    }
    assert set(calls) == set(ENTRY)
    for name, rest in calls.items():
        assert getattr(hip_lib, name)(None, *rest) == -5, name
        assert "no model" in api.last_error(), name
