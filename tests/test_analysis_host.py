"""Feature analysis (lpcnet_batch_analyze*), the parts that need no GPU: the generated window / band tables against the reference's
values, the host build of the analysis kernels' log10 against libm, the C-ABI surface, the Python surface, the seeded test audio,
and the compiler's resource figures of the three analysis kernels."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import zlib
from decimal import Decimal, getcontext

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tables  # noqa: E402
import kernel_resources  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

CSRC = os.path.join(ROOT, "lpcnet_amd", "csrc")
NEW_SYMBOLS = ("lpcnet_batch_analyze", "lpcnet_batch_analyze_float", "lpcnet_batch_analyze_device", "lpcnet_batch_analyze_device_shard",
               "lpcnet_batch_analysis_enable", "lpcnet_batch_analysis_reset", "lpcnet_batch_analysis_state_size",
               "lpcnet_batch_get_analysis_state", "lpcnet_batch_set_analysis_state")


# ---- tables ------------------------------------------------------------------------------------------------------------------
def test_window_and_band_tables_equal_the_reference_values():
    ref = np.load(os.path.join(ROOT, "tests", "golden", "ref_analysis_tables_v1.npz"))
    hw = gen_tables.half_window()
    assert hw.dtype == np.float32 and hw.size == 160 and np.array_equal(hw.view(np.uint32), ref["half_window"].view(np.uint32))
    assert np.array_equal(gen_tables.eband5ms(), ref["eband5ms"]) and ref["eband5ms"].size == 18


def test_generated_headers_are_in_sync_and_the_existing_two_do_not_move(tmp_path):
    text = open(os.path.join(CSRC, "lpcnet_analysis_tables_gen.h")).read()
    body = re.search(r"lpcn_half_window\[160\] = \{(.*?)\};", text, re.S).group(1)
    vals = np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fp.+-]+f", body)], np.float32)
    assert np.array_equal(vals.view(np.uint32), gen_tables.half_window().view(np.uint32))
    eb = [int(x) for x in re.search(r"lpcn_eband5ms\[18\] = \{(.*?)\};", text).group(1).split(",")]
    assert eb == gen_tables.eband5ms().tolist()
    # regenerating: all three headers byte-identical to the committed ones
    a, b, c = (str(tmp_path / n) for n in ("a.h", "b.h", "c.h"))
    gen_tables.emit("lpcn_", a); gen_tables.emit("orc_", b); gen_tables.emit_analysis(c)
    assert open(a).read() == open(os.path.join(CSRC, "lpcnet_tables_gen.h")).read()
    assert open(b).read() == open(os.path.join(ROOT, "oracle", "orc_tables_gen.h")).read()
    assert open(c).read() == text


# ---- log10 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def log10_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("log10") / "liblog10_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "log10_host.cpp"), "-o", out])
    L = C.CDLL(out)
    lp, dp = C.POINTER(C.c_long), C.POINTER(C.c_double)
    L.log10_sweep_random.argtypes = [C.c_uint64, C.c_long, lp, dp]
    L.log10_sweep_adjacent.argtypes = [C.c_int, lp, dp]
    L.log10_sweep_boundaries.argtypes = [C.c_int, C.c_int, C.c_int, lp, dp]
    L.log_unit_engine.restype = C.c_double
    L.log_unit_engine.argtypes = [C.c_double]
    return L


def test_log10_equals_libm_over_the_reachable_range(log10_lib):
    cnt, bad = (C.c_long * 2)(), (C.c_double * 64)()
    log10_lib.log10_sweep_random(20261015, 12_000_000, cnt, bad)            # log-uniform doubles over [1e-2, 1e12]
    assert cnt[0] >= 10_000_000 and cnt[1] == 0, (list(cnt), bad[0].hex())
    log10_lib.log10_sweep_adjacent(131, cnt, bad)                            # 1e-2 + float and both neighbouring doubles, every 131st float up to 1e12
    assert cnt[0] > 20_000_000 and cnt[1] == 0, (list(cnt), bad[0].hex())
    a = np.array([1e-2, 1.0, 0.5, 2.0, 10.0, 1e12, 0.99999999999999989, 1.0000000000000002, np.inf], np.float64)
    o, r = np.zeros(a.size, np.float32), np.zeros(a.size, np.float32)
    fp, dp = np.ctypeslib.ndpointer(np.float32), np.ctypeslib.ndpointer(np.float64)
    log10_lib.log10_engine.argtypes = [dp, fp, C.c_long]; log10_lib.log10_glibc.argtypes = [dp, fp, C.c_long]
    log10_lib.log10_engine(a, o, a.size); log10_lib.log10_glibc(a, r, a.size)
    assert np.array_equal(o.view(np.uint32), r.view(np.uint32))


def test_log10_next_to_float_rounding_boundaries_of_the_result(log10_lib):
    """Arguments whose log10 lies next to the midpoint of two floats: the nearest double to 10^midpoint and 1..4 doubles to either side
    (each step moves the result by ~0.1 ULP of a double), for every 997th float in [-2, 12].  libm's log10 is fdlibm's formula over
    libm's log, and the routine restates that formula over a correctly rounded log: the floats are identical wherever libm's log IS
    the correctly rounded double.  Where it is not (libm claims 0.52 ULP, not 0.5) the last bit of the double may decide the float here
    -- by construction -- so every differing argument must be exactly that case, shown with 80-digit arithmetic, and rare."""
    cnt, bad = (C.c_long * 2)(), (C.c_double * 64)()
    log10_lib.log10_sweep_boundaries(499, 5, 60, cnt, bad)                   # 0.5 .. 6 double-ULPs from the boundary: identical everywhere
    assert cnt[0] > 10_000_000 and cnt[1] <= 64
    far = [bad[k] for k in range(cnt[1])]
    log10_lib.log10_sweep_boundaries(997, 0, 4, cnt, bad)                    # (the harness keeps the first 64 differing arguments)
    assert cnt[0] > 1_000_000 and cnt[1] <= 64 and cnt[1] < cnt[0] * 1e-4, list(cnt)
    getcontext().prec = 80
    for a in far + [bad[k] for k in range(cnt[1])]:
        m, e = math.frexp(a)
        x = m * 2 if e - 1 >= 0 else m                                       # fdlibm's reduction: [1, 2) for a >= 1, [0.5, 1) below
        exact = Decimal(x).ln()
        assert log10_lib.log_unit_engine(x) == float(exact), a.hex()         # ours is the correctly rounded log
        assert math.log(x) != float(exact), a.hex()                          # libm's is not: the only source of a difference


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported_and_no_encoder_name_is(hip_lib):
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW_SYMBOLS:
        assert re.search(r"LPCNET_EXPORT int " + n + r"\(", header), n
        assert n in exported, n
    assert not [s for s in exported if s.startswith(("lpcnet_encoder_", "lpcnet_compute_", "lpcnet_encode"))]
    assert not [s for s in exported if s.startswith("lpcn_")]
    assert hip_lib.lpcnet_batch_analysis_state_size() == 4 * (160 + 1 + 1 + 16 + 1 + 576 + 224 + 1 + 1)
    # no new host C file, no environment switch on the analysis path
    assert "getenv" not in open(os.path.join(CSRC, "analysis_kernels.hip.h")).read()


def test_python_surface():
    for m in ("analyze", "analyze_device", "analyze_device_shard", "analysis_enable", "analysis_reset", "get_analysis_state", "set_analysis_state"):
        assert callable(getattr(api.LPCNetBatch, m)), m


def test_make_pcm_is_deterministic_and_reaches_the_hard_inputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_analysis_v1.npz"))
    T = g["features"].shape[1]
    assert g["features"].shape[0] >= 6 and T >= 200 and g["features"].shape[2] == 36
    for k, seed in enumerate(g["seeds"]):
        p = synth.make_pcm(int(seed), T)
        assert p.dtype == np.int16 and p.shape == (T * 160,)
        assert zlib.crc32(p.tobytes()) == int(g["pcm_crc32"][k])             # the audio the fixture was made from
        assert np.array_equal(p, synth.make_pcm(int(seed), T))
        zero_frames = (p.reshape(T, 160) == 0).all(axis=1).sum()
        assert zero_frames >= 2 and p.max() == 32767 and p.min() == -32768    # digital silence, full scale both ways
        assert abs(float(p.astype(np.float64).mean())) > 1.0                  # a DC offset
        pitch = g["features"][k, :, 18]
        assert (pitch == np.float32(.01) * np.float32(66 - 200)).any() and (pitch == np.float32(.01) * np.float32(510 - 200)).any()   # both clamps
    assert not np.array_equal(synth.make_pcm(1, 10), synth.make_pcm(2, 10))
    assert np.array_equal(synth.make_pcm(5, 20)[:160 * 3].shape, (480,))


# ---- kernels -----------------------------------------------------------------------------------------------------------------
def test_analysis_kernels_compile_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources.engine_kernel_resources(asm_path=str(tmp_path / "engine.s"))
    assert set(res) == {"analysis_spectrum_kernel", "analysis_xcorr_kernel", "analysis_pitch_kernel"}
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] % 64 == 0 and r["vgpr"] <= 128 and r["lds"] <= 32768, (name, r)
