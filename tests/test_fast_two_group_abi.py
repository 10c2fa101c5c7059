"""The FAST two-group switch at the C boundary, without a GPU: the built library exports lpcnet_batch_set_fast_two_group /
lpcnet_batch_get_fast_two_group, include/lpcnet_batch.h declares them, and lpcnet_amd/api.py gives them argument types."""
import ctypes as C
import os
import re
import subprocess

from lpcnet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lpcnet_batch_set_fast_two_group", "lpcnet_batch_get_fast_two_group")


def test_header_declares_both_entry_points():
    text = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"LPCNET_EXPORT\s+int\s+lpcnet_batch_set_fast_two_group\s*\(\s*LPCNetBatch\s*\*\s*b\s*,\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"LPCNET_EXPORT\s+int\s+lpcnet_batch_get_fast_two_group\s*\(\s*const\s+LPCNetBatch\s*\*\s*b\s*\)\s*;", text)


def test_library_exports_both_symbols(hip_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert n in exported, n
    assert not [s for s in exported if s.startswith("lpcn_")]      # (the engine's own entry points of the switch stay inside)


def test_python_binding_sets_the_argument_types(hip_lib):
    assert hip_lib.lpcnet_batch_set_fast_two_group.argtypes == [C.c_void_p, C.c_int]
    assert hip_lib.lpcnet_batch_get_fast_two_group.argtypes == [C.c_void_p]
    prop = api.LPCNetBatch.fast_two_group
    assert isinstance(prop, property) and prop.fset is not None


def test_a_batch_without_a_model_is_refused_not_crashed(hip_lib):
    """NULL batch: the getter answers 0, the setter an error code -- no device is touched"""
    assert hip_lib.lpcnet_batch_get_fast_two_group(None) == 0
    assert hip_lib.lpcnet_batch_set_fast_two_group(None, 1) != 0
