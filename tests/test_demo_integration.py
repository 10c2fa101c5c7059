"""The reference's OWN demo program (src/lpcnet_demo.c, unmodified) on the HIP engine: BASELINE.json configs 0 -> 1.

CPU part (`-m "not gpu"`): where a reference tree is present, build() runs `make -C integration`, which compiles
src/lpcnet_demo.c in place against the reference's headers and links it with liblpcnet_hip.so +
integration/stubs_unused_modes.c; the tests here look at what that left under oracle/_ref/ and read nothing outside
the repository.  GPU part: the resulting binary (it travels to the GPU box like the other build outputs under oracle/_ref/) runs
`-synthesis` on the 10-second / 1000-frame feature file and must write, byte for byte, what the reference's own
generic-C binaries wrote (tests/golden/golden_demo_v1.npz, made by tests/tools/make_golden_demo.py from
oracle/_ref/lpcnet_demo_gf / _gi; compared directly as well where those binaries are present), and `-decode`,
which the reference's demo can only run on a compiled-in model (src/lpcnet_demo.c:176-188), on the process-default
model and codebooks."""
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

from lpcnet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "oracle", "_ref", "lpcnet_demo_hip")
PLC = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_plc_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_demo_v1.npz")


def test_reference_demo_links_against_the_engine(hip_lib):
    if not os.path.exists(DEMO):
        pytest.skip("oracle/_ref/lpcnet_demo_hip not built (needs the reference tree: make -C integration)")
    needed = subprocess.run(["ldd", DEMO], capture_output=True, text=True).stdout
    assert "liblpcnet_hip.so" in needed and "not found" not in needed.split("liblpcnet_hip.so")[1].split("\n")[0]
    syms = subprocess.run(["nm", "-D", "--undefined-only", DEMO], capture_output=True, text=True).stdout
    for s in ("lpcnet_create", "lpcnet_load_model", "lpcnet_synthesize", "lpcnet_destroy", "lpcnet_decoder_create", "lpcnet_decode"):
        assert s in syms                                   # resolved by liblpcnet_hip.so, not by the stubs
    # the modes outside the engine's scope stop with a message instead of doing nothing
    r = subprocess.run([DEMO, "-features", "/dev/null", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 2 and "not part of the LPCNet HIP engine" in r.stderr


def test_unmodified_reference_plc_compiles_and_links_against_the_engine(hip_lib):
    """SURVEY.md section 8f N3 / VERDICT r2: src/lpcnet_plc.c, the one reference file that looks INSIDE LPCNetState
    (src/lpcnet_plc.c:176-180) and embeds it by value, builds untouched against the engine's state layout
    (include/lpcnet_hip_state.h through the forced include integration/lpcnet_private_hip.h) and links with
    -Wl,--no-undefined (integration/Makefile; the library exists only if that link succeeded): every LPCNet symbol it needs
    resolves to liblpcnet_hip.so."""
    if not os.path.exists(PLC):
        pytest.skip("oracle/_ref/liblpcnet_plc_hip.so not built (needs the reference tree: make -C integration plc)")
    lib = PLC
    needed = subprocess.run(["ldd", lib], capture_output=True, text=True).stdout
    assert "liblpcnet_hip.so" in needed
    und = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True).stdout
    for sym in ("lpcnet_init", "lpcnet_load_model", "lpcnet_reset", "lpcnet_reset_signal", "lpcnet_synthesize_impl",
                "lpcnet_synthesize_tail_impl", "run_frame_network_deferred", "run_frame_network_flush"):
        assert (" U " + sym) in und, sym                   # taken from the engine, not from a CPU copy of src/lpcnet.c
    dfn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    assert " T lpcnet_plc_update" in dfn and " T lpcnet_plc_conceal" in dfn
    # the PLC state embeds the ENGINE's state: its size follows the engine's lpcnet_get_size()
    import ctypes
    from lpcnet_amd import api
    plc = ctypes.CDLL(lib)
    eng = api.load_library()
    ref_state = 0
    gf = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")
    if os.path.exists(gf):
        r = ctypes.CDLL(gf)
        ref_state = r.lpcnet_plc_get_size() - r.lpcnet_get_size()          # everything but the embedded LPCNetState
        assert abs(plc.lpcnet_plc_get_size() - eng.lpcnet_get_size() - ref_state) <= 8      # (alignment padding)
    assert plc.lpcnet_plc_get_size() > eng.lpcnet_get_size() == 8724


def _run_demo(tmp_path, flavour, args, extra_files=()):
    d = str(tmp_path)
    with open(os.path.join(d, "weights_blob.bin"), "wb") as f:
        f.write(synth.blob_bytes(synth.make_model(flavour=flavour)))
    for name, data in extra_files:
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    r = subprocess.run([DEMO] + args, cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return np.fromfile(os.path.join(d, args[-1]), np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("fl,flavour", [("gf", "float"), ("gi", "int8")])
def test_demo_synthesis_10s_file_equals_reference_binary(tmp_path, fl, flavour, hip_lib):
    """`lpcnet_demo_hip -synthesis` on the 1000-frame file == lpcnet_demo_gf / lpcnet_demo_gi (reference, generic C)."""
    if not os.path.exists(DEMO):
        pytest.skip("oracle/_ref/lpcnet_demo_hip not built (needs the reference tree: make -C integration)")
    g = np.load(GOLDEN)
    T = int(g["n_frames"])
    feats = synth.make_features(int(g["seed"]), T)
    pcm = _run_demo(tmp_path, flavour, ["-synthesis", "feat.f32", "out.pcm"], [("feat.f32", feats.astype(np.float32).tobytes())])
    assert pcm.size == T * 160
    crc = np.array([zlib.crc32(f.tobytes()) for f in pcm.reshape(-1, 160)], np.uint32)
    bad = np.nonzero(crc != g[f"{fl}_crc"])[0]
    assert bad.size == 0, f"first diverging frame {bad[0]} of {T}"
    assert np.array_equal(np.frombuffer(hashlib.sha256(pcm.tobytes()).digest(), np.uint8), g[f"{fl}_sha256"])
    assert np.array_equal(pcm[:480], g[f"{fl}_head"]) and np.array_equal(pcm[-160:], g[f"{fl}_tail"])
    ref_exe = os.path.join(ROOT, "oracle", "_ref", f"lpcnet_demo_{fl}")
    if os.path.exists(ref_exe):                            # the reference binary itself, side by side (`cmp`)
        d = str(tmp_path)
        subprocess.check_call([ref_exe, "-synthesis", "feat.f32", "ref.pcm"], cwd=d)
        assert open(os.path.join(d, "ref.pcm"), "rb").read() == open(os.path.join(d, "out.pcm"), "rb").read()


@pytest.mark.gpu
def test_demo_decode_on_default_model_and_codebooks(tmp_path, golden, hip_lib):
    """`lpcnet_demo_hip -decode`: the demo never hands the decoder a model (src/lpcnet_demo.c:176-188); the engine binds
    ./weights_blob.bin and ./ceps_codebooks.bin as process defaults.  Expected PCM = the real reference's lpcnet_decode
    on the same packets (golden `packet_pcm_gf`, generated through oracle/_ref)."""
    if not os.path.exists(DEMO):
        pytest.skip("oracle/_ref/lpcnet_demo_hip not built")
    cbs = synth.make_codebooks(5)
    cb_bytes = b"".join(np.ascontiguousarray(c, np.float32).tobytes() for c in cbs)
    packets = np.ascontiguousarray(golden["packets"], np.uint8)
    pcm = _run_demo(tmp_path, "float", ["-decode", "pk.bin", "out.pcm"], [("pk.bin", packets.tobytes()), ("ceps_codebooks.bin", cb_bytes)])
    assert np.array_equal(pcm, golden["packet_pcm_gf"].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("options", [0, 4, 2], ids=["causal", "causal+dc-filter", "codec"])
def test_unmodified_reference_plc_runs_on_the_engine_bit_exact(options, hip_lib):
    """SURVEY.md section 8f N3, end to end: the reference's packet-loss concealment (src/lpcnet_plc.c, compiled UNMODIFIED against
    the engine's state layout, oracle/_ref/liblpcnet_plc_hip.so) drives the HIP engine through the internal entry points --
    by-value state snapshots and rollbacks (src/lpcnet_plc.c:223-231,384-414), teacher forcing, deferred frame-network
    queue, direct clearing of state members (:176-180) -- over a signal with lost frames, and must return sample for
    sample what the reference's own generic-C build returns (oracle/_ref/liblpcnet_ref_gf.so: same PLC network, same
    feature extraction, its own CPU LPCNet).  The PLC network is a seeded synthetic one (tests/tools/plc_synth.py)."""
    import ctypes as C
    import sys
    ref_path = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")
    plc_path = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_plc_hip.so")
    if not (os.path.exists(ref_path) and os.path.exists(plc_path)):
        pytest.skip("oracle/_ref/liblpcnet_plc_hip.so / liblpcnet_ref_gf.so not built (needs the reference tree)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import plc_synth
    from lpcnet_amd import api
    blob = synth.blob_bytes(plc_synth.make_model_with_plc())
    # the signal: 60 frames synthesised by the engine itself (speech-like), every 7th..9th frame lost
    feats = synth.make_features(4242, 64)
    b = api.LPCNetBatch(1, blob)
    signal = b.synthesize(feats[None])[0, 4 * 160:]
    b.close()
    T = signal.size // 160
    lost = [(t % 9) in (6, 7) or t in (20, 21, 22, 23) for t in range(T)]

    def run(path):
        lib = C.CDLL(path)
        lib.lpcnet_plc_create.restype = C.c_void_p
        lib.lpcnet_plc_create.argtypes = [C.c_int]
        lib.lpcnet_plc_load_model.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lib.lpcnet_plc_update.argtypes = [C.c_void_p, C.c_void_p]
        lib.lpcnet_plc_conceal.argtypes = [C.c_void_p, C.c_void_p]
        lib.lpcnet_plc_destroy.argtypes = [C.c_void_p]
        buf = C.create_string_buffer(blob, len(blob))         # must outlive the state (the reference keeps pointers into it)
        st = lib.lpcnet_plc_create(options)
        assert lib.lpcnet_plc_load_model(st, buf, len(blob)) == 0
        out = np.zeros(T * 160, np.int16)
        for t in range(T):
            frame = np.ascontiguousarray(signal[t * 160:(t + 1) * 160]).copy()
            if lost[t]:
                lib.lpcnet_plc_conceal(st, frame.ctypes.data)
            else:
                lib.lpcnet_plc_update(st, frame.ctypes.data)
            out[t * 160:(t + 1) * 160] = frame
        lib.lpcnet_plc_destroy(st)
        return out

    want = run(ref_path)
    got = run(plc_path)
    concealed = np.concatenate([want[t * 160:(t + 1) * 160] for t in range(T) if lost[t]])
    assert np.abs(concealed.astype(np.int32)).max() > 50      # the concealment really synthesised something
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (int(bad[0]) // 160, int(bad[0]) % 160, int(bad.size))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,min_per_pass", [("burst", 2.5), ("staggered", 1.2)])
def test_threaded_plc_server_combines_the_plc_facing_entry_points(pattern, min_per_pass, hip_lib):
    """a packet-loss-concealment server with one thread per stream.  32 threads each run the reference's UNMODIFIED
    src/lpcnet_plc.c on the engine through their own loss pattern; the entry points it calls -- run_frame_network (through the deferred
    queue), lpcnet_synthesize_impl, lpcnet_synthesize_tail_impl (src/lpcnet_private.h:125-132, src/lpcnet_plc.c:216-239,378-421) -- are
    combined into multi-stream passes like lpcnet_synthesize.  Every thread must return, sample for sample, what the reference's own
    generic-C build returns for its signal and losses.  Calls combine when they have the same shape (entry point, N, preload) at the
    same time: `burst` = the same frames are lost on every stream (a network outage), where the threads fall into step and the 32
    together are served at many times one thread's rate; `staggered` = every stream has its own loss times, where only the calls
    that happen to coincide share a pass.  What is asserted is the combining itself (calls served per device pass, from the dispatcher's own
    counters) -- the wall-clock ratio is printed, but it depends on the box's host cores (3.7 x .. 9 x seen for `burst`)."""
    import ctypes as C
    import sys
    import threading
    import time
    ref_path = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")
    plc_path = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_plc_hip.so")
    if not (os.path.exists(ref_path) and os.path.exists(plc_path)):
        pytest.skip("oracle/_ref/liblpcnet_plc_hip.so / liblpcnet_ref_gf.so not built (needs the reference tree)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import plc_synth
    from lpcnet_amd import api
    blob = synth.blob_bytes(plc_synth.make_model_with_plc())
    NT, T = 32, 36
    feats = np.stack([synth.make_features(4300 + i, T + 4) for i in range(NT)])
    b = api.LPCNetBatch(NT, blob)
    signals = b.synthesize(feats)[:, 4 * 160:]
    b.close()
    if pattern == "burst":
        lost = [[t % 9 in (6, 7) or t in (20, 21, 22) for t in range(T)] for i in range(NT)]
    else:
        lost = [[(t + 2 * i) % 9 in (6, 7) or (t in (20, 21, 22) and i % 3 == 0) for t in range(T)] for i in range(NT)]

    def bind(path):
        lib = C.CDLL(path)
        lib.lpcnet_plc_create.restype = C.c_void_p
        lib.lpcnet_plc_create.argtypes = [C.c_int]
        lib.lpcnet_plc_load_model.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lib.lpcnet_plc_update.argtypes = [C.c_void_p, C.c_void_p]
        lib.lpcnet_plc_conceal.argtypes = [C.c_void_p, C.c_void_p]
        lib.lpcnet_plc_destroy.argtypes = [C.c_void_p]
        return lib

    buf = C.create_string_buffer(blob, len(blob))             # must outlive the states (the reference keeps pointers into it)

    def run_one(lib, i, out):
        st = lib.lpcnet_plc_create(0)
        assert lib.lpcnet_plc_load_model(st, buf, len(blob)) == 0
        for t in range(T):
            frame = np.ascontiguousarray(signals[i, t * 160:(t + 1) * 160]).copy()
            (lib.lpcnet_plc_conceal if lost[i][t] else lib.lpcnet_plc_update)(st, frame.ctypes.data)
            out[t * 160:(t + 1) * 160] = frame
        lib.lpcnet_plc_destroy(st)

    ref, eng = bind(ref_path), bind(plc_path)
    want = np.zeros((NT, T * 160), np.int16)
    for i in range(NT):
        run_one(ref, i, want[i])
    api.clear_error()
    warm = np.zeros(T * 160, np.int16)
    run_one(eng, 0, warm)                                     # model upload, kernel load
    assert np.array_equal(warm, want[0])
    t0 = time.perf_counter()
    alone = np.zeros(T * 160, np.int16)
    run_one(eng, 1, alone)
    t_one = time.perf_counter() - t0
    got = np.zeros((NT, T * 160), np.int16)
    ths = [threading.Thread(target=run_one, args=(eng, i, got[i])) for i in range(NT)]
    api.dispatch_stats(reset=True)
    t0 = time.perf_counter()
    for th in ths: th.start()
    for th in ths: th.join()
    t_all = time.perf_counter() - t0
    bad = [i for i in range(NT) if not np.array_equal(got[i], want[i])]
    assert not bad, bad
    assert np.array_equal(alone, want[1])
    calls, passes, largest = api.dispatch_stats()
    speedup = NT * t_one / t_all
    print(f"threaded PLC ({pattern}): one stream {t_one * 1e3:.0f} ms, {NT} threads {t_all * 1e3:.0f} ms -> {speedup:.1f} x one thread's rate; "
          f"{calls} calls in {passes} device passes ({calls / max(passes, 1):.1f} per pass, largest {largest})")
    assert calls >= NT * T and calls / passes >= min_per_pass and largest >= (8 if pattern == "burst" else 2), (calls, passes, largest)
    assert speedup >= 1.0, (t_one, t_all)                         # (32 threads are never slower than one thread doing all the work in turn)
