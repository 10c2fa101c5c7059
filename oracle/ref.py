"""TEST INFRASTRUCTURE ONLY: ctypes front-end to oracle/_ref/liblpcnet_ref_<flavour>.so,
i.e. to the *real reference* compiled by oracle/Makefile (plus oracle/ref_harness.c accessors).
Imported only by tests/, bench.py's cpu_baseline leg and tools that generate golden fixtures.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_i16p = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


# the variant flavours of oracle/Makefile: name -> (LPC_GAMMA, END2END) the library was compiled with
VARIANTS = {"gg": (0.9, False), "ge": (1.0, True), "gx": (0.95, True)}


def available(flavour="gf") -> bool:
    return os.path.exists(os.path.join(REF_DIR, f"liblpcnet_ref_{flavour}.so"))


class RefLib:
    """One loaded flavour of the compiled reference (gf, gi, af, ai, or a variant build: gg, ge, gx)."""

    def __init__(self, flavour="gf"):
        path = os.path.join(REF_DIR, f"liblpcnet_ref_{flavour}.so")
        self.flavour = flavour
        self.lib = lib = C.CDLL(path)
        vp = C.c_void_p
        lib.lpcnet_create.restype = vp
        lib.lpcnet_destroy.argtypes = [vp]
        lib.lpcnet_get_size.restype = C.c_int
        lib.lpcnet_reset.argtypes = [vp]
        lib.lpcnet_load_model.argtypes = [vp, C.c_char_p, C.c_int]
        lib.lpcnet_load_model.restype = C.c_int
        lib.lpcnet_synthesize.argtypes = [vp, _f32p, _i16p, C.c_int]
        lib.lpcnet_decoder_create.restype = vp
        lib.lpcnet_decoder_destroy.argtypes = [vp]
        lib.lpcnet_decode.argtypes = [vp, _u8p, _i16p]
        lib.ref_flavour.restype = C.c_int
        lib.ref_set_codebooks.argtypes = [_f32p] * 4
        lib.ref_get_nnet_state.argtypes = [vp, _f32p, _f32p, _f32p, _f32p]
        lib.ref_set_gru_state.argtypes = [vp, _f32p, _f32p]
        lib.ref_get_frame_products.argtypes = [vp, _f32p, _f32p, _f32p]
        lib.ref_get_signal_state.argtypes = [vp, _f32p, C.POINTER(C.c_int), C.POINTER(C.c_float),
                                             C.POINTER(C.c_int), _u32p]
        lib.ref_get_logit_table.argtypes = [vp, _f32p]
        lib.ref_synthesize_impl.argtypes = [vp, _f32p, _i16p, C.c_int, C.c_int]
        if hasattr(lib, "ref_synthesize_tail"):          # (absent from a library built before the hook existed)
            lib.ref_synthesize_tail.argtypes = [vp, _f32p, _f32p, _f32p, _i16p, C.c_int, C.c_int]
            lib.ref_synthesize_tail.restype = None
        lib.ref_run_frame_network.argtypes = [vp, _f32p, _f32p, _f32p, _f32p]
        lib.ref_run_sample_network.argtypes = [vp, _f32p, _f32p, C.c_int, C.c_int, C.c_int]
        lib.ref_run_sample_network.restype = C.c_int
        lib.ref_gru_a_input.argtypes = [vp, _f32p, _f32p, C.c_int, C.c_int, C.c_int]
        lib.ref_sparse_gru_a.argtypes = [vp, _f32p, _f32p]
        lib.ref_gru_b.argtypes = [vp, _f32p, _f32p, _f32p]
        lib.ref_sample_mdense.argtypes = [vp, _f32p, _u32p]
        lib.ref_sample_mdense.restype = C.c_int
        lib.ref_mdense_logits.argtypes = [vp, _f32p, _f32p]
        lib.ref_lin2ulaw.argtypes = [C.c_float]
        lib.ref_lin2ulaw.restype = C.c_int
        lib.ref_ulaw2lin.argtypes = [C.c_float]
        lib.ref_ulaw2lin.restype = C.c_float
        lib.ref_vec_tanh.argtypes = [_f32p, _f32p, C.c_int]
        lib.ref_vec_sigmoid.argtypes = [_f32p, _f32p, C.c_int]
        lib.ref_lpc_from_cepstrum.argtypes = [_f32p, _f32p]
        lib.ref_lpc_from_cepstrum.restype = C.c_float
        lib.ref_lpc_weighting.argtypes = [_f32p, C.c_float]
        lib.ref_decode_packet.argtypes = [_f32p, _f32p, _u8p]
        if hasattr(lib, "ref_plc_get_state"):            # (absent from a library built before the PLC accessors existed)
            lib.lpcnet_plc_create.restype = vp
            lib.lpcnet_plc_create.argtypes = [C.c_int]
            lib.lpcnet_plc_destroy.argtypes = [vp]
            lib.lpcnet_plc_load_model.argtypes = [vp, C.c_char_p, C.c_int]
            lib.lpcnet_plc_update.argtypes = [vp, _i16p]
            lib.lpcnet_plc_conceal.argtypes = [vp, _i16p]
            lib.lpcnet_plc_fec_add.argtypes = [vp, vp]
            lib.lpcnet_plc_fec_clear.argtypes = [vp]
            lib.ref_plc_lpcnet.restype = vp
            lib.ref_plc_lpcnet.argtypes = [vp]
            lib.ref_plc_enc.restype = vp
            lib.ref_plc_enc.argtypes = [vp]
            lib.ref_plc_net_units.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
            lib.ref_plc_get_state.argtypes = [vp, vp, vp, vp, vp, vp, vp]
            lib.ref_get_deferred_state.argtypes = [vp, _f32p, _f32p]
            lib.ref_enc_get_state.argtypes = [vp, vp]
            lib.ref_enc_get_state.restype = C.c_int
        lib.kiss99_srand.argtypes = [_u32p, C.c_char_p, C.c_int]
        lib.kiss99_rand.argtypes = [_u32p]
        lib.kiss99_rand.restype = C.c_uint32

    # -- synthesis states ---------------------------------------------------------------
    def new_state(self, blob: bytes) -> "RefState":
        return RefState(self, blob)

    def synthesize_file(self, blob: bytes, features: np.ndarray) -> np.ndarray:
        """What `lpcnet_demo -synthesis` does (src/lpcnet_demo.c:202-219)."""
        st = self.new_state(blob)
        return st.synthesize(features)


class RefState:
    def __init__(self, ref: RefLib, blob: bytes):
        self.ref = ref
        self.lib = ref.lib
        self._blob = C.create_string_buffer(blob, len(blob))   # must outlive the state
        self.p = self.lib.lpcnet_create()
        ret = self.lib.lpcnet_load_model(self.p, self._blob, len(blob))
        if ret != 0:
            raise RuntimeError("reference lpcnet_load_model failed")

    def __del__(self):
        try:
            self.lib.lpcnet_destroy(self.p)
        except Exception:
            pass

    def synthesize(self, features: np.ndarray, preload_pcm: np.ndarray | None = None) -> np.ndarray:
        """features (T,>=20) -> int16 (T*160,).  With preload_pcm the loop is teacher-forced
        (src/lpcnet.c:256-259): the given samples are fed back instead of the sampled ones."""
        T = features.shape[0]
        out = np.zeros(T * 160, np.int16)
        for t in range(T):
            f = np.ascontiguousarray(features[t, :20], np.float32)
            frame = out[t * 160:(t + 1) * 160]
            if preload_pcm is None:
                self.lib.lpcnet_synthesize(self.p, f, frame, 160)
            else:
                frame[:] = preload_pcm[t * 160:(t + 1) * 160]
                self.lib.ref_synthesize_impl(self.p, f, frame, 160, 160)
        return out

    def frame_products(self):
        lpc = np.zeros(16, np.float32)
        ca = np.zeros(1152, np.float32)
        cb = np.zeros(48, np.float32)
        self.lib.ref_get_frame_products(self.p, lpc, ca, cb)
        return lpc, ca, cb

    def nnet_state(self):
        c1 = np.zeros(168, np.float32)
        c2 = np.zeros(256, np.float32)
        ga = np.zeros(384, np.float32)
        gb = np.zeros(16, np.float32)
        self.lib.ref_get_nnet_state(self.p, c1, c2, ga, gb)
        return c1, c2, ga, gb

    def signal_state(self):
        ls = np.zeros(16, np.float32)
        le = C.c_int()
        dm = C.c_float()
        fc = C.c_int()
        rng = np.zeros(4, np.uint32)
        self.lib.ref_get_signal_state(self.p, ls, C.byref(le), C.byref(dm), C.byref(fc), rng)
        return ls, le.value, dm.value, fc.value, rng


class _LpcnetView(RefState):
    """the LPCNetState embedded in an LPCNetPLCState: RefState's readers on a pointer this object does not own"""

    def __init__(self, lib, p):
        self.lib, self.p = lib, p

    def __del__(self):
        pass


class RefPlc:
    """One LPCNetPLCState of the compiled reference (lpcnet_plc_create / _load_model / _update / _conceal / _fec_add / _fec_clear), with the
    accessors of oracle/ref_harness.c: ctl() the nine control ints, snapshot() every member a stream's state is made of."""

    def __init__(self, ref: RefLib, blob: bytes, options: int):
        self.lib = ref.lib
        self._blob = C.create_string_buffer(blob, len(blob))   # must outlive the state
        self.p = self.lib.lpcnet_plc_create(options)
        if self.lib.lpcnet_plc_load_model(self.p, self._blob, len(blob)) != 0:
            raise RuntimeError("reference lpcnet_plc_load_model failed")
        g1, g2 = C.c_int(), C.c_int()
        self.lib.ref_plc_net_units(C.byref(g1), C.byref(g2))
        self.g = (g1.value, g2.value)
        self.lpcnet = _LpcnetView(self.lib, self.lib.ref_plc_lpcnet(self.p))

    def __del__(self):
        try:
            self.lib.lpcnet_plc_destroy(self.p)
        except Exception:
            pass

    def fec_add(self, features=None):
        if features is None:
            self.lib.lpcnet_plc_fec_add(self.p, None)
        else:
            v = np.ascontiguousarray(features, np.float32)
            assert v.shape == (20,)
            self.lib.lpcnet_plc_fec_add(self.p, v.ctypes.data)

    def fec_clear(self):
        self.lib.lpcnet_plc_fec_clear(self.p)

    def step(self, frame: np.ndarray, lost) -> np.ndarray:
        """one frame: lpcnet_plc_conceal when lost (the input is ignored), else lpcnet_plc_update -> the frame as the reference leaves it"""
        out = np.zeros(160, np.int16) if lost else np.ascontiguousarray(frame, np.int16).copy()
        (self.lib.lpcnet_plc_conceal if lost else self.lib.lpcnet_plc_update)(self.p, out)
        return out

    def ctl(self) -> np.ndarray:
        c = np.zeros(9, np.int32)
        self.lib.ref_plc_get_state(self.p, c.ctypes.data, None, None, None, None, None)
        return c

    def snapshot(self) -> dict:
        """every member of the state, as the reference's own arrays (the names of tests/tools/plc_state_map.SNAP_FIELDS)"""
        s = dict(ctl=np.zeros(9, np.int32), pcm=np.zeros(560, np.int16), features=np.zeros(20, np.float32),
                 net=np.zeros((4, sum(self.g)), np.float32), dc=np.zeros(2, np.float64), fec=np.zeros((100, 20), np.float32))
        self.lib.ref_plc_get_state(self.p, *(s[k].ctypes.data for k in ("ctl", "pcm", "features", "net", "dc", "fec")))
        s["conv1"], s["conv2"], s["gru_a"], s["gru_b"] = self.lpcnet.nnet_state()
        ls, le, dm, fc, rng = self.lpcnet.signal_state()
        s.update(last_sig=ls, last_exc=np.int32(le), deemph_mem=np.float32(dm), frame_count=np.int32(fc), rng=rng)
        s["lpc"], s["cond_a"], s["cond_b"] = self.lpcnet.frame_products()
        s["old_lpc"], s["feature_buffer"] = np.zeros((2, 16), np.float32), np.zeros(80, np.float32)
        self.lib.ref_get_deferred_state(self.lpcnet.p, s["old_lpc"], s["feature_buffer"])
        enc = self.lib.ref_plc_enc(self.p)
        buf = C.create_string_buffer(self.lib.ref_enc_get_state(enc, None))
        self.lib.ref_enc_get_state(enc, buf)
        s["enc"] = np.frombuffer(buf.raw, np.uint8).copy()
        s["g"] = np.array(self.g, np.int32)
        return s
