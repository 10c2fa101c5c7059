"""Python mirror of the C API in include/lpcnet.h + include/lpcnet_batch.h (ctypes over the
C-ABI of liblpcnet_hip.so).  Same names and argument meaning as the reference's
include/lpcnet.h so that tests read like the reference's own driver (src/lpcnet_demo.c:202-219,
src/test_lpcnet.c:55-64).

There is no CPU fallback: importing works anywhere, but every entry point needs the HIP library
and a GPU, and fails loudly otherwise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LPCNET_HIP_LIB") or os.path.join(_HERE, "liblpcnet_hip.so")

NB_FEATURES = 20
NB_TOTAL_FEATURES = 36
LPCNET_FRAME_SIZE = 160
LPCNET_COMPRESSED_SIZE = 8
LPCNET_PACKET_SAMPLES = 640

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_i16p = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")

_lib = None


class LPCNetError(RuntimeError):
    pass


PLC_CAUSAL, PLC_NONCAUSAL, PLC_CODEC, PLC_DC_FILTER = 0, 1, 2, 4      # include/lpcnet_batch.h
PLC_SUMMARY = 10


def plc_plan(options: int, ctl: np.ndarray, lost, fec_op=None):
    """The PLC's host planner alone (no device): advances ctl [n][9] int32 in place by one step, returns the step's summary [n][10]"""
    L = load_library()
    assert ctl.dtype == np.int32 and ctl.ndim == 2 and ctl.shape[1] == 9 and ctl.flags.c_contiguous
    n = ctl.shape[0]
    lost = np.ascontiguousarray(lost, np.uint8)
    op = None if fec_op is None else np.ascontiguousarray(fec_op, np.uint8)
    out = np.zeros((n, PLC_SUMMARY), np.int32)
    rc = L.lpcnet_hip_plc_plan(options, n, ctl.ctypes.data, lost, None if op is None else op.ctypes.data, out.ctypes.data)
    if rc:
        raise LPCNetError("plc_plan failed (%d): %s" % (rc, last_error()))
    return out


def plc_pred_form_table(n_records: int, cus: int, d1: int, g1: int, g2: int, int8: bool = False, pinned: int = 0) -> int:
    """The PLC prediction kernels' form rule alone (no device): the streams per workgroup (1, 2, 4, 8) a launch over n_records records runs with on a
    device of `cus` compute units, for a network of widths d1 / g1 / g2 (float or int8).  pinned = 0: the table's choice, else the pinned value;
    either way halved until the form's LDS fits"""
    L = load_library()
    rc = L.lpcnet_hip_plc_pred_form(n_records, cus, d1, g1, g2, 1 if int8 else 0, pinned)
    if rc < 0:
        raise LPCNetError("plc_pred_form_table failed (%d): %s" % (rc, last_error()))
    return rc


def encode_plan(n: int, active: int, count: int, analysis: bool = False):
    """The launches of one encode call of `count` packets (or, analysis=True, one analyze call of `count` frames) on a batch of capacity n with
    `active` streams running, by the engine's own chunk and items-per-wavefront rules (no device): a list with one dict per launch -- packets (or
    frames), items, and for the encoder ipw_end, ipw_mid, wg_end, last_end, wg_mid, last_mid (workgroups of either VQ kernel and the items in the
    last one).  compute_features runs the encoder's chunks without the VQ kernels"""
    L = load_library()
    k = L.lpcnet_hip_encode_plan(n, active, count, 1 if analysis else 0, None, 0)
    if k < 0:
        raise LPCNetError("encode_plan failed (%d): %s" % (k, last_error()))
    out = np.zeros((max(k, 1), 8), np.int32)
    k = L.lpcnet_hip_encode_plan(n, active, count, 1 if analysis else 0, out.ctypes.data, out.shape[0])
    if analysis:
        return [dict(frames=int(r[0]), items=int(r[1])) for r in out[:k]]
    names = ("packets", "items", "ipw_end", "ipw_mid", "wg_end", "last_end", "wg_mid", "last_mid")
    return [dict(zip(names, (int(x) for x in r))) for r in out[:k]]


PLC_LANES_REC = 10


def plc_plan_lanes(options: int, ctl: np.ndarray, lost, lanes: int, fec_op=None):
    """The PLC's host planner with lanes (no device): advances ctl [n][9] int32 in place by one step and returns (summary [n][10], launches [k][10]:
    type, op, lane, slot, cnt, offset of its records in the lists, ints per record, kind, N, preload; the control lists)"""
    L = load_library()
    assert ctl.dtype == np.int32 and ctl.ndim == 2 and ctl.shape[1] == 9 and ctl.flags.c_contiguous
    n = ctl.shape[0]
    lost = np.ascontiguousarray(lost, np.uint8)
    op = None if fec_op is None else np.ascontiguousarray(fec_op, np.uint8)
    out = np.zeros((n, PLC_SUMMARY), np.int32)
    launch = np.zeros((128, PLC_LANES_REC), np.int32)
    lists = np.zeros(64 * n + 64, np.int32)
    k = L.lpcnet_hip_plc_plan_lanes(options, n, lanes, ctl.ctypes.data, lost, None if op is None else op.ctypes.data, out.ctypes.data,
                                    launch.ctypes.data, launch.shape[0], lists.ctypes.data, lists.size)
    if k < 0:
        raise LPCNetError("plc_plan_lanes failed (%d): %s" % (k, last_error()))
    used = max([0] + [int(r[5] + r[4] * r[6]) for r in launch[:k]])
    return out, launch[:k].copy(), lists[:used].copy()


PLC_FEED_REC = 8


def plc_fec_feed_plan(ctl: np.ndarray, count, skip=None, clear=None):
    """plc_fec_feed's host planner alone (no device): advances the ring positions of ctl [n][9] int32 in place and returns (records [k][8]: stream,
    first row of the packed vectors, rows a, their ring row, first ring row moved to the front, rows moved, rows b, their ring row; dropped [n])"""
    L = load_library()
    assert ctl.dtype == np.int32 and ctl.ndim == 2 and ctl.shape[1] == 9 and ctl.flags.c_contiguous
    n = ctl.shape[0]
    count, skip, clear = _feed_args(n, count, skip, clear)
    rec = np.zeros((n, PLC_FEED_REC), np.int32)
    dropped = np.zeros(n, np.int32)
    rc = L.lpcnet_hip_plc_fec_feed_plan(n, ctl.ctypes.data, count.ctypes.data, None if skip is None else skip.ctypes.data,
                                        None if clear is None else clear.ctypes.data, rec.ctypes.data, dropped.ctypes.data)
    if rc < 0:
        raise LPCNetError("plc_fec_feed_plan failed (%d): %s" % (rc, last_error()))
    return rec[:rc].copy(), dropped


def _feed_args(n, count, skip, clear):
    count = np.ascontiguousarray(count, np.int32)
    skip = None if skip is None else np.ascontiguousarray(skip, np.int32)
    clear = None if clear is None else np.ascontiguousarray(clear, np.uint8)
    assert count.shape == (n,) and (skip is None or skip.shape == (n,)) and (clear is None or clear.shape == (n,))
    return count, skip, clear


# ---- stream snapshots (include/lpcnet_batch.h: lpcnet_batch_snapshot) ----
SNAP_META = 10
SNAP_SECTIONS = ("SYNTH", "DEC_VQ", "AN", "ENC_VQ", "KEEP_A", "KEEP_B", "KEEP_LPC", "KEEP_FLAG", "PLC_Q", "PLC_FEAT", "PLC_NET", "PLC_DC", "PLC_DELTA",
                 "PLC_FEC", "PLC_FBUF", "PLC_LP", "PLC_BURG", "PLC_AN", "PLC_CTL", "DRED_ENC", "DRED_DEC")
SNAP = {name: i + 1 for i, name in enumerate(SNAP_SECTIONS)}      # section ids (LPCNET_SNAP_*)
_SNAP_LAYOUT_INTS = 92


def _snap_config(config):
    """a configuration as the ten ints of LPCNET_SNAP_CONFIG, from a dict (missing keys: off / 0) or a sequence"""
    if isinstance(config, dict):
        keys = ("int8", "analysis", "encoder", "keep", "plc", "plc_options", "g1", "g2", "dred_enc_floats", "dred_enc_dframes")
        unknown = set(config) - set(keys)
        if unknown:
            raise ValueError(f"unknown configuration keys {sorted(unknown)}")
        config = [int(config.get(k, 0)) for k in keys]
    cfg = np.ascontiguousarray(config, np.int32)
    assert cfg.shape == (10,)
    return cfg


def snapshot_layout(config):
    """The snapshot record of a configuration, without a device: config = dict(int8, analysis, encoder, keep, plc, plc_options, g1, g2,
    dred_enc_floats, dred_enc_dframes) -> dict(sections [(id, bytes per stream, offset)], record_bytes)."""
    L = load_library()
    cfg = _snap_config(config)
    out = np.zeros(_SNAP_LAYOUT_INTS, np.int32)
    k = L.lpcnet_hip_snapshot_layout(cfg.ctypes.data, out.ctypes.data, out.size)
    if k < 0:
        raise LPCNetError("snapshot_layout failed (%d): %s" % (k, last_error()))
    return dict(sections=[tuple(int(x) for x in out[3 * i:3 * i + 3]) for i in range(k)], record_bytes=int(out[3 * k]))


def snapshot_info(blob: bytes):
    """The header and layout of a snapshot blob: dict(version, m, record_bytes, int8, plc, plc_options, g1, g2, dred_enc_floats, dred_enc_dframes,
    state_size, analysis_state_size, plc_state_size, model_hash, sections [(id, bytes, offset)]).  LPCNetError for anything that is not a blob."""
    L = load_library()
    info = np.zeros(4 + _SNAP_LAYOUT_INTS, np.int32)
    n = L.lpcnet_hip_snapshot_info(bytes(blob), len(blob), info.ctypes.data, info.size)
    if n < 0:
        raise LPCNetError("snapshot_info failed (%d): %s" % (n, last_error()))
    keys = ("version", "m", "record_bytes", "n_sections", "int8", "plc", "plc_options", "g1", "g2", "dred_enc_floats", "dred_enc_dframes", "state_size",
            "analysis_state_size", "plc_state_size")
    d = {k: int(v) for k, v in zip(keys, info)}
    d["model_hash"] = (int(info[14]) & 0xffffffff) | ((int(info[15]) & 0xffffffff) << 32)
    d["sections"] = [tuple(int(x) for x in info[16 + 3 * i:19 + 3 * i]) for i in range(d.pop("n_sections"))]
    return d


def snapshot_match(config_snap, config_batch, enqueue_only: bool = False):
    """Would a snapshot of one configuration restore into a batch of another?  (code, section id): 0 yes, 1 yes in the host form (which enables the
    missing subsystem first), LPCNET_HIP_E_MODEL (-5) no -- last_error() says why and the section is the one it names."""
    L = load_library()
    a, b = _snap_config(config_snap), _snap_config(config_batch)
    sec = C.c_int(0)
    rc = L.lpcnet_hip_snapshot_match(a.ctypes.data, b.ctypes.data, 1 if enqueue_only else 0, C.byref(sec))
    return rc, sec.value


def load_library():
    """dlopen liblpcnet_hip.so (built by `python -m lpcnet_amd.build`).  Raises if it is absent:
    the product path never falls back to a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LPCNetError(f"{LIB_PATH} not built: run `python -m lpcnet_amd.build` (needs hipcc)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.lpcnet_get_size.restype = C.c_int
    L.lpcnet_init.argtypes = [vp]
    L.lpcnet_reset.argtypes = [vp]
    L.lpcnet_create.restype = vp
    L.lpcnet_destroy.argtypes = [vp]
    L.lpcnet_synthesize.argtypes = [vp, _f32p, _i16p, C.c_int]
    L.lpcnet_synthesize.restype = None
    L.lpcnet_load_model.argtypes = [vp, C.c_char_p, C.c_int]
    # the reference's internal entry points (src/lpcnet_private.h:125-132)
    L.lpcnet_reset_signal.argtypes = [vp]
    L.lpcnet_reset_signal.restype = None
    L.run_frame_network.argtypes = [vp, _f32p, _f32p, _f32p, _f32p]
    L.run_frame_network.restype = None
    L.run_frame_network_deferred.argtypes = [vp, _f32p]
    L.run_frame_network_deferred.restype = None
    L.run_frame_network_flush.argtypes = [vp]
    L.run_frame_network_flush.restype = None
    L.lpcnet_synthesize_tail_impl.argtypes = [vp, _i16p, C.c_int, C.c_int]
    L.lpcnet_synthesize_tail_impl.restype = None
    L.lpcnet_synthesize_impl.argtypes = [vp, _f32p, _i16p, C.c_int, C.c_int]
    L.lpcnet_synthesize_impl.restype = None
    L.lpcnet_decoder_get_size.restype = C.c_int
    L.lpcnet_decoder_init.argtypes = [vp]
    L.lpcnet_decoder_create.restype = vp
    L.lpcnet_decoder_destroy.argtypes = [vp]
    L.lpcnet_decode.argtypes = [vp, _u8p, _i16p]
    L.lpcnet_hip_last_error.restype = C.c_char_p
    L.lpcnet_hip_set_codebooks.argtypes = [_f32p] * 4
    L.lpcnet_hip_set_codebooks.restype = None
    L.lpcnet_hip_shutdown.restype = None
    L.lpcnet_hip_set_default_model.argtypes = [C.c_char_p, C.c_int]
    L.lpcnet_hip_decoder_load_model.argtypes = [vp, C.c_char_p, C.c_int]
    L.lpcnet_hip_set_device.argtypes = [C.c_int]
    L.lpcnet_batch_create_sharded.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    L.lpcnet_batch_create_sharded.restype = vp
    L.lpcnet_batch_shards.argtypes = [vp]
    L.lpcnet_batch_shard_info.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lpcnet_batch_synthesize_device_shard.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]
    L.lpcnet_hip_check_model.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_batch_create.argtypes = [C.c_int, C.c_int]
    L.lpcnet_batch_create.restype = vp
    L.lpcnet_batch_destroy.argtypes = [vp]
    L.lpcnet_batch_streams.argtypes = [vp]
    L.lpcnet_batch_load_model.argtypes = [vp, C.c_char_p, C.c_int]
    L.lpcnet_batch_reset.argtypes = [vp, C.c_int, C.c_int]
    L.lpcnet_batch_synthesize.argtypes = [vp, _f32p, C.c_int, _i16p, C.c_int]
    L.lpcnet_batch_synthesize_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    L.lpcnet_batch_sync.argtypes = [vp]
    L.lpcnet_batch_synthesize_preload.argtypes = [vp, _f32p, C.c_int, _i16p, C.c_int, C.c_int]
    L.lpcnet_batch_synthesize_step.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.lpcnet_batch_decode.argtypes = [vp, _u8p, _i16p, C.c_int]
    L.lpcnet_batch_decode_device.argtypes = [vp, vp, vp, C.c_int, vp]
    L.lpcnet_batch_set_lpc_gamma.argtypes = [vp, C.c_float]
    L.lpcnet_batch_set_end2end.argtypes = [vp, C.c_int]
    L.lpcnet_batch_set_fast.argtypes = [vp, C.c_int]
    L.lpcnet_batch_analyze.argtypes = [vp, _i16p, _f32p, C.c_int, C.c_int]
    L.lpcnet_batch_analyze_float.argtypes = [vp, _f32p, _f32p, C.c_int, C.c_int]
    L.lpcnet_batch_analyze_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, vp]
    L.lpcnet_batch_analyze_device_shard.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp]
    L.lpcnet_batch_analysis_enable.argtypes = [vp, C.c_int]
    L.lpcnet_batch_analysis_reset.argtypes = [vp, C.c_int, C.c_int]
    L.lpcnet_batch_get_analysis_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_set_analysis_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_plc_enable.argtypes = [vp, C.c_int]
    L.lpcnet_batch_plc_flavour.argtypes = [vp]
    L.lpcnet_batch_plc_reset.argtypes = [vp, C.c_int, C.c_int]
    L.lpcnet_batch_plc_step.argtypes = [vp, _i16p, _u8p]
    L.lpcnet_batch_plc_step_device.argtypes = [vp, vp, _u8p, vp]
    L.lpcnet_batch_plc_step_device_shard.argtypes = [vp, C.c_int, vp, _u8p, vp]
    L.lpcnet_batch_plc_fec_add.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_plc_fec_clear.argtypes = [vp, C.c_int]
    L.lpcnet_batch_plc_fec_feed.argtypes = [vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_plc_fec_feed_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_plc_fec_feed_device_shard.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.lpcnet_hip_plc_fec_feed_plan.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_get_plc_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_set_plc_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_plc_burg.argtypes = [vp, _f32p, _f32p]
    L.lpcnet_batch_plc_pred.argtypes = [vp, _f32p, _f32p]
    L.lpcnet_hip_plc_plan.argtypes = [C.c_int, C.c_int, vp, _u8p, vp, vp]
    L.lpcnet_hip_plc_plan_lanes.argtypes = [C.c_int, C.c_int, C.c_int, vp, _u8p, vp, vp, vp, C.c_int, vp, C.c_int]
    L.lpcnet_batch_set_group_schedule.argtypes = [vp, C.c_int, C.c_int]
    L.lpcnet_batch_get_group_schedule.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lpcnet_batch_group_form.argtypes = [vp, C.c_int]
    L.lpcnet_batch_last_groups.argtypes = [vp, vp, C.c_int]
    L.lpcnet_hip_plc_model_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_hip_dred_model_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_batch_dred_enable.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_decode.argtypes = [vp, _f32p, _f32p, vp, _f32p]
    L.lpcnet_batch_dred_decode_device.argtypes = [vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_dred_decode_device_shard.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.lpcnet_batch_dred_decode_packed_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_dred_decode_packed_device_shard.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_dred_info.argtypes = [vp, C.POINTER(C.c_int)]
    L.lpcnet_batch_dred_state_enable.argtypes = [vp]
    L.lpcnet_batch_dred_dec_state_size.argtypes = [vp]
    L.lpcnet_batch_get_dred_dec_state.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_set_dred_dec_state.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_dred_init.argtypes = [vp, _f32p, vp]
    L.lpcnet_batch_dred_init_device.argtypes = [vp, vp, vp, vp]
    L.lpcnet_batch_dred_init_device_shard.argtypes = [vp, C.c_int, vp, vp, vp]
    L.lpcnet_batch_dred_step.argtypes = [vp, _f32p, vp, vp, _f32p]
    L.lpcnet_batch_dred_step_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.lpcnet_batch_dred_step_device_shard.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.lpcnet_batch_dred_step_packed_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_dred_step_packed_device_shard.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.lpcnet_batch_dred_flavour.argtypes = [vp]
    L.lpcnet_batch_plc_set_pred_form.argtypes = [vp, C.c_int]
    L.lpcnet_batch_plc_get_pred_form.argtypes = [vp, C.c_int]
    L.lpcnet_hip_plc_pred_form.argtypes = [C.c_int] * 7
    L.lpcnet_hip_encode_plan.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int]
    L.lpcnet_batch_dred_set_form.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_get_form.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_set_fast.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_get_fast.argtypes = [vp]
    L.lpcnet_hip_dred_enc_model_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_batch_dred_enc_enable.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_enc_info.argtypes = [vp, C.POINTER(C.c_int)]
    L.lpcnet_batch_dred_enc_flavour.argtypes = [vp]
    L.lpcnet_batch_dred_encode.argtypes = [vp, _f32p, C.c_int, vp, _f32p, _f32p]
    L.lpcnet_batch_dred_encode_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.lpcnet_batch_dred_encode_device_shard.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.lpcnet_batch_dred_enc_get_state.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_dred_enc_set_state.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_dred_enc_set_form.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_enc_get_form.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_enc_set_fast.argtypes = [vp, C.c_int]
    L.lpcnet_batch_dred_enc_get_fast.argtypes = [vp]
    L.lpcnet_batch_encode.argtypes = [vp, _i16p, _u8p, C.c_int]
    L.lpcnet_batch_encode_device.argtypes = [vp, vp, vp, C.c_int, vp]
    L.lpcnet_batch_encode_device_shard.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
    L.lpcnet_batch_compute_features.argtypes = [vp, _i16p, _f32p, C.c_int, C.c_int]
    L.lpcnet_batch_compute_features_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    L.lpcnet_batch_encoder_enable.argtypes = [vp, C.c_int]
    L.lpcnet_batch_get_encoder_vq_mem.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_set_encoder_vq_mem.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_get_decoder_vq_mem.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_set_decoder_vq_mem.argtypes = [vp, C.c_int, _f32p]
    L.lpcnet_batch_set_active.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.lpcnet_batch_get_active.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.lpcnet_batch_active_streams.argtypes = [vp]
    L.lpcnet_batch_copy_streams.argtypes = [vp, vp, vp, C.c_int, vp]
    L.lpcnet_batch_snapshot_layout.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_batch_snapshot_bytes.argtypes = [vp, C.c_int]
    L.lpcnet_batch_snapshot_bytes.restype = C.c_size_t
    L.lpcnet_batch_snapshot.argtypes = [vp, vp, C.c_int, vp, C.c_size_t]
    L.lpcnet_batch_restore.argtypes = [vp, vp, C.c_int, C.c_char_p, C.c_size_t]
    L.lpcnet_batch_snapshot_device.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.lpcnet_batch_restore_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.lpcnet_batch_snapshot_device_shard.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.lpcnet_batch_restore_device_shard.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.lpcnet_batch_copy_streams_to.argtypes = [vp, vp, vp, vp, C.c_int]
    L.lpcnet_hip_snapshot_layout.argtypes = [vp, vp, C.c_int]
    L.lpcnet_hip_snapshot_info.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_int]
    L.lpcnet_hip_snapshot_match.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_batch_export_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_import_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_set_streams_per_workgroup.argtypes = [vp, C.c_int]
    L.lpcnet_batch_get_streams_per_workgroup.argtypes = [vp]
    L.lpcnet_batch_set_twelve_waves.argtypes = [vp, C.c_int]
    L.lpcnet_batch_get_twelve_waves.argtypes = [vp]
    L.lpcnet_batch_set_two_group_streaming.argtypes = [vp, C.c_int]
    L.lpcnet_batch_get_two_group_streaming.argtypes = [vp]
    L.lpcnet_batch_set_fast_two_group.argtypes = [vp, C.c_int]
    L.lpcnet_batch_get_fast_two_group.argtypes = [vp]
    L.lpcnet_hip_x2_wide_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.lpcnet_hip_x3_image_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lpcnet_batch_tune.argtypes = [vp]
    L.lpcnet_batch_enable_timing.argtypes = [vp, C.c_int]
    L.lpcnet_batch_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.lpcnet_batch_last_error.restype = C.c_char_p
    L.lpcnet_batch_run_tail.argtypes = [vp, _f32p, _f32p, _f32p, _i16p, C.c_int, C.c_int]
    L.lpcnet_batch_run_frames.argtypes = [vp, _f32p, C.c_int, vp, vp, vp, C.c_int]
    L.lpcnet_batch_run_decode.argtypes = [vp, _u8p, _f32p, C.c_int]
    L.lpcnet_hip_packet_features.argtypes = [_u8p, _f32p, _f32p]
    L.lpcnet_batch_state_size.restype = C.c_int
    L.lpcnet_batch_get_raw_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_set_raw_state.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_debug_trace.argtypes = [vp, C.c_int, vp]
    L.lpcnet_batch_profile.argtypes = [vp, vp]
    _u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    L.lpcnet_hip_arith_identities_device.argtypes = [_f32p, _f32p, _u32p, _u32p, _u32p, _u32p, C.c_int]
    L.lpcnet_hip_quant_sweep_device.argtypes = [C.POINTER(C.c_ulonglong)]
    L.lpcnet_hip_status.restype = C.c_int
    L.lpcnet_hip_clear_error.restype = None
    L.lpcnet_hip_model_status.argtypes = [vp, C.c_int]
    L.lpcnet_hip_build_info.restype = C.c_char_p
    L.lpcnet_hip_dispatch_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    _lib = L
    return L


def check_model(blob: bytes):
    """Host-only validation of a DNNw blob: returns (code, info[6]); see include/lpcnet.h."""
    info = (C.c_int * 6)()
    rc = load_library().lpcnet_hip_check_model(blob, len(blob), info)
    return rc, list(info)


def plc_model_info(blob: bytes):
    """Host-only view of a blob's PLC network: dict(present, servable, d1, g1, g2, nb1, nb2); see include/lpcnet_batch.h."""
    info = (C.c_int * 7)()
    if load_library().lpcnet_hip_plc_model_info(blob, len(blob), info) != 0:
        raise LPCNetError("plc_model_info: " + last_error())
    return dict(zip(("present", "servable", "d1", "g1", "g2", "nb1", "nb2"), list(info)))


def dred_model_info(blob: bytes):
    """Host-only view of a blob's DRED decoder: dict(present, servable, latent_dim, state_dim, widths[8]); see include/lpcnet_batch.h."""
    info = (C.c_int * 12)()
    if load_library().lpcnet_hip_dred_model_info(blob, len(blob), info) != 0:
        raise LPCNetError("dred_model_info: " + last_error())
    v = list(info)
    return dict(present=v[0], servable=v[1], latent_dim=v[2], state_dim=v[3], widths=v[4:12])


def dred_enc_model_info(blob: bytes):
    """Host-only view of a blob's DRED encoder: dict(present, servable, latent_dim, state_dim, taps, gdense1, state_floats, widths[8]); see
    include/lpcnet_batch.h."""
    info = (C.c_int * 15)()
    if load_library().lpcnet_hip_dred_enc_model_info(blob, len(blob), info) != 0:
        raise LPCNetError("dred_enc_model_info: " + last_error())
    v = list(info)
    return dict(present=v[0], servable=v[1], latent_dim=v[2], state_dim=v[3], taps=v[4], gdense1=v[5], state_floats=v[6], widths=v[7:15])


def packet_features(packet: np.ndarray, vq_mem: np.ndarray) -> np.ndarray:
    """Host-only: lpcnet_decode's unpacker on one 8-byte packet; vq_mem (18,) float32 advances in place; returns features (4, 36)."""
    assert vq_mem.dtype == np.float32 and vq_mem.shape == (18,) and vq_mem.flags.c_contiguous
    feat = np.zeros((4, NB_TOTAL_FEATURES), np.float32)
    rc = load_library().lpcnet_hip_packet_features(np.ascontiguousarray(packet, np.uint8).reshape(8), vq_mem, feat.reshape(-1))
    if rc:
        raise LPCNetError("packet_features failed (%d): %s" % (rc, last_error()))
    return feat


def x3_image_info(blob: bytes):
    """Host-only view of a blob's twelve-wave image: (have, desc[12][5][4], rows[12][5][64], selftest); see include/lpcnet.h."""
    desc, rows, st = (C.c_int * (12 * 5 * 4))(), (C.c_int * (12 * 5 * 64))(), C.c_int(-1)
    have = load_library().lpcnet_hip_x3_image_info(blob, len(blob), desc, rows, C.byref(st))
    return have, np.array(desc, np.int32).reshape(12, 5, 4), np.array(rows, np.int32).reshape(12, 5, 64), st.value


def x2_wide_info(blob: bytes):
    """Host-only view of a blob's wide two-group image (the streamed variants of the two-group kernel; include/lpcnet.h): dict(fits -- 1, 0, or -1
    for a malformed blob --, items, variant, resident, selftest, b3[8], head[8])."""
    info = (C.c_int * 21)()
    rc = load_library().lpcnet_hip_x2_wide_info(blob, len(blob), info)
    v = list(info)
    return dict(fits=rc, items=v[1], variant=v[2], resident=v[3], selftest=v[4], b3=v[5:13], head=v[13:21])


def last_error() -> str:
    return load_library().lpcnet_hip_last_error().decode()


def status() -> int:
    """Sticky per-thread status of the void entry points (0 = no failure since clear_error())."""
    return load_library().lpcnet_hip_status()


def clear_error() -> None:
    load_library().lpcnet_hip_clear_error()


def build_info() -> dict:
    """{'src': hash of every source the library was built from, 'dev': hash of the device sources alone}"""
    txt = load_library().lpcnet_hip_build_info().decode()
    return dict(kv.split("=", 1) for kv in txt.split())


def dispatch_stats(reset=False):
    """(calls served, device passes, calls in the largest pass) of the combining dispatcher behind the per-state entry points"""
    out = (C.c_ulonglong * 3)()
    load_library().lpcnet_hip_dispatch_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1]), int(out[2])


def quant_sweep():
    """(mismatches over all finite |t| < 2^31, mismatches with |t| <= 127.5, a mismatching bit pattern) of v_cvt_rpi_i32_f32 vs floor(.5 + (double)t)"""
    out = (C.c_ulonglong * 3)()
    rc = load_library().lpcnet_hip_quant_sweep_device(out)
    if rc:
        raise LPCNetError(f"lpcnet_hip_quant_sweep_device failed ({rc}): " + last_error())
    return int(out[0]), int(out[1]), int(out[2])


def arith_identities(a: np.ndarray, b: np.ndarray):
    """Bit patterns of (mfma products, v_mul products, packed mul/add halves, scalar mul/add) for operand arrays a, b (float32, len % 64 == 0)."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    n = a.size
    outs = [np.empty((n, 4), np.uint32) for _ in range(4)]
    rc = load_library().lpcnet_hip_arith_identities_device(a, b, *outs, n)
    if rc:
        raise LPCNetError(f"lpcnet_hip_arith_identities_device failed ({rc}): " + last_error())
    return outs


class StreamState(C.Structure):
    """Raw per-stream record = struct lpcn_stream_state (lpcnet_amd/csrc/lpcnet_engine.h)."""
    _fields_ = [("gru_a", C.c_float * 384), ("gru_b", C.c_float * 16),
                ("conv1_mem", C.c_float * 168), ("conv2_mem", C.c_float * 256),
                ("old_lpc", C.c_float * 32), ("last_sig", C.c_float * 16),
                ("deemph_mem", C.c_float), ("last_exc", C.c_int32), ("frame_count", C.c_int32),
                ("rng", C.c_uint32 * 4), ("lpc", C.c_float * 16), ("pad", C.c_int32 * 3)]


class LPCNetState:
    """lpcnet_create / lpcnet_load_model / lpcnet_synthesize / lpcnet_destroy (include/lpcnet.h)."""

    def __init__(self, blob: bytes | None = None):
        self.L = load_library()
        self.p = self.L.lpcnet_create()
        self._blob = None
        if blob is not None:
            self.load_model(blob)

    def load_model(self, blob: bytes) -> int:
        self._blob = blob
        ret = self.L.lpcnet_load_model(self.p, blob, len(blob))
        if ret != 0:
            raise LPCNetError("lpcnet_load_model failed: " + last_error())
        return ret

    def reset(self):
        self.L.lpcnet_reset(self.p)

    def synthesize(self, features: np.ndarray, n: int = LPCNET_FRAME_SIZE) -> np.ndarray:
        out = np.zeros(n, np.int16)
        self.L.lpcnet_synthesize(self.p, np.ascontiguousarray(features[:NB_FEATURES], np.float32), out, n)
        return out

    # ---- the reference's internal entry points (PLC-facing, src/lpcnet_private.h:125-132)
    def reset_signal(self):
        self.L.lpcnet_reset_signal(self.p)

    def run_frame_network(self, features: np.ndarray):
        ga, gb, lpc = np.zeros(1152, np.float32), np.zeros(48, np.float32), np.zeros(16, np.float32)
        self.L.run_frame_network(self.p, ga, gb, lpc, np.ascontiguousarray(features[:NB_FEATURES], np.float32))
        return ga, gb, lpc

    def run_frame_network_deferred(self, features: np.ndarray):
        self.L.run_frame_network_deferred(self.p, np.ascontiguousarray(features[:NB_FEATURES], np.float32))

    def run_frame_network_flush(self):
        self.L.run_frame_network_flush(self.p)

    def synthesize_tail_impl(self, n: int = LPCNET_FRAME_SIZE, preload_pcm=None) -> np.ndarray:
        out = np.zeros(n, np.int16)
        k = 0 if preload_pcm is None else len(preload_pcm)
        out[:k] = preload_pcm if k else 0
        self.L.lpcnet_synthesize_tail_impl(self.p, out, n, k)
        return out

    def synthesize_impl(self, features: np.ndarray, n: int = LPCNET_FRAME_SIZE, preload_pcm=None) -> np.ndarray:
        out = np.zeros(n, np.int16)
        k = 0 if preload_pcm is None else len(preload_pcm)
        out[:k] = preload_pcm if k else 0
        self.L.lpcnet_synthesize_impl(self.p, np.ascontiguousarray(features[:NB_FEATURES], np.float32), out, n, k)
        return out

    def raw_bytes(self) -> bytes:
        return C.string_at(self.p, self.L.lpcnet_get_size())

    def load_raw_bytes(self, raw: bytes):
        C.memmove(self.p, raw, self.L.lpcnet_get_size())

    def __del__(self):
        try:
            self.L.lpcnet_destroy(self.p)
        except Exception:
            pass


class LPCNetDecState:
    """lpcnet_decoder_create / lpcnet_decode; blob=None: the process-default model (what the reference's demo relies on)."""

    def __init__(self, blob: bytes | None = None):
        self.L = load_library()
        self.p = self.L.lpcnet_decoder_create()
        self._blob = blob
        if blob is not None and self.L.lpcnet_hip_decoder_load_model(self.p, blob, len(blob)) != 0:
            raise LPCNetError("lpcnet_hip_decoder_load_model failed: " + last_error())

    def decode(self, packet: np.ndarray) -> np.ndarray:
        pcm = np.zeros(LPCNET_PACKET_SAMPLES, np.int16)
        if self.L.lpcnet_decode(self.p, np.ascontiguousarray(packet, np.uint8), pcm) != 0:
            raise LPCNetError("lpcnet_decode failed: " + last_error())
        return pcm

    def __del__(self):
        try:
            self.L.lpcnet_decoder_destroy(self.p)
        except Exception:
            pass


def set_default_model(blob: bytes):
    if load_library().lpcnet_hip_set_default_model(blob, len(blob)) != 0:
        raise LPCNetError("lpcnet_hip_set_default_model failed: " + last_error())


def shutdown():
    load_library().lpcnet_hip_shutdown()


def set_codebooks(cb1, cb2, cb3, cbd):
    load_library().lpcnet_hip_set_codebooks(*[np.ascontiguousarray(x, np.float32).reshape(-1) for x in (cb1, cb2, cb3, cbd)])


class LPCNetBatch:
    """n independent streams on one GPU, or sharded over `devices` (include/lpcnet_batch.h)."""

    def __init__(self, n_streams: int, blob: bytes, device: int = 0, devices=None):
        self.L = load_library()
        self.n = n_streams
        if devices is None:
            self.p = self.L.lpcnet_batch_create(n_streams, device)
        else:
            arr = (C.c_int * len(devices))(*devices)
            self.p = self.L.lpcnet_batch_create_sharded(n_streams, arr, len(devices))
        if not self.p:
            raise LPCNetError("lpcnet_batch_create failed: " + last_error())
        if self.L.lpcnet_batch_load_model(self.p, blob, len(blob)) != 0:
            err = last_error()
            self.L.lpcnet_batch_destroy(self.p)
            self.p = None
            raise LPCNetError("lpcnet_batch_load_model failed: " + err)

    def _chk(self, rc, what):
        if rc != 0:
            raise LPCNetError(f"{what} failed ({rc}): " + last_error())

    def close(self):
        if getattr(self, "p", None):
            self.L.lpcnet_batch_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, first=0, count=None):
        self._chk(self.L.lpcnet_batch_reset(self.p, first, self.n - first if count is None else count), "reset")

    def synthesize(self, features: np.ndarray, preload_pcm: np.ndarray | None = None, preload: int = 160) -> np.ndarray:
        """features (n, T, stride>=20) float32 -> pcm (n, T*160) int16."""
        n, T, stride = features.shape
        assert n == self.n
        f = np.ascontiguousarray(features, np.float32)
        if preload_pcm is None:
            pcm = np.zeros((n, T * 160), np.int16)
            self._chk(self.L.lpcnet_batch_synthesize(self.p, f.reshape(-1), stride, pcm.reshape(-1), T), "synthesize")
        else:
            pcm = np.ascontiguousarray(preload_pcm, np.int16).copy()
            self._chk(self.L.lpcnet_batch_synthesize_preload(self.p, f.reshape(-1), stride, pcm.reshape(-1), T, preload), "synthesize_preload")
        return pcm

    def synthesize_step(self, features: np.ndarray, pcm: np.ndarray, n_samples, preload, mode) -> np.ndarray:
        """one frame step with per-stream (mode, n_samples, preload): include/lpcnet_batch.h lpcnet_batch_synthesize_step;
        features (n, >=20), pcm (n, 160) int16 (in: the imposed samples; out: the synthesised ones)."""
        f = np.ascontiguousarray(features, np.float32)
        out = np.ascontiguousarray(pcm, np.int16).copy()
        ns, pr, md = (np.ascontiguousarray(x, np.int32) for x in (n_samples, preload, mode))
        assert f.shape[0] == self.n and out.shape == (self.n, LPCNET_FRAME_SIZE) and ns.size == pr.size == md.size == self.n
        self._chk(self.L.lpcnet_batch_synthesize_step(self.p, f.ctypes.data_as(C.c_void_p), f.shape[1], out.ctypes.data_as(C.c_void_p),
                                                      ns.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), md.ctypes.data_as(C.c_void_p)),
                  "lpcnet_batch_synthesize_step")
        return out

    def synthesize_device(self, d_features_ptr: int, stride: int, d_pcm_ptr: int, n_frames: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_synthesize_device(self.p, d_features_ptr, stride, d_pcm_ptr, n_frames, hip_stream or None), "synthesize_device")

    def sync(self):
        self._chk(self.L.lpcnet_batch_sync(self.p), "sync")

    @property
    def shards(self):
        """[(first, count, device)] of every shard"""
        out = []
        for k in range(self.L.lpcnet_batch_shards(self.p)):
            a, b, c = C.c_int(), C.c_int(), C.c_int()
            self._chk(self.L.lpcnet_batch_shard_info(self.p, k, C.byref(a), C.byref(b), C.byref(c)), "shard_info")
            out.append((a.value, b.value, c.value))
        return out

    def synthesize_device_shard(self, shard: int, d_features_ptr: int, stride: int, d_pcm_ptr: int, n_frames: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_synthesize_device_shard(self.p, shard, d_features_ptr, stride, d_pcm_ptr, n_frames, hip_stream or None),
                  "synthesize_device_shard")

    # ---- feature analysis (lpcnet_compute_single_frame_features per stream and frame; include/lpcnet_batch.h) ----
    def analyze(self, pcm: np.ndarray) -> np.ndarray:
        """pcm (n, T*160) int16 or float32 -> features (n, T, 36) float32: cepstrum [0..17], pitch [18], pitch correlation [19], LPC [20..35]."""
        pcm = np.asarray(pcm)
        n, ns = pcm.shape
        assert n == self.n and ns % LPCNET_FRAME_SIZE == 0 and ns > 0
        T = ns // LPCNET_FRAME_SIZE
        feat = np.zeros((n, T, NB_TOTAL_FEATURES), np.float32)
        if pcm.dtype == np.float32:
            self._chk(self.L.lpcnet_batch_analyze_float(self.p, np.ascontiguousarray(pcm).reshape(-1), feat.reshape(-1), NB_TOTAL_FEATURES, T), "analyze_float")
        else:
            assert pcm.dtype == np.int16, "pcm must be int16 or float32"
            self._chk(self.L.lpcnet_batch_analyze(self.p, np.ascontiguousarray(pcm).reshape(-1), feat.reshape(-1), NB_TOTAL_FEATURES, T), "analyze")
        return feat

    def analyze_device(self, d_pcm_ptr: int, pcm_is_float: bool, d_features_ptr: int, stride: int, n_frames: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_analyze_device(self.p, d_pcm_ptr, int(bool(pcm_is_float)), d_features_ptr, stride, n_frames, hip_stream or None),
                  "analyze_device")

    def analyze_device_shard(self, shard: int, d_pcm_ptr: int, pcm_is_float: bool, d_features_ptr: int, stride: int, n_frames: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_analyze_device_shard(self.p, shard, d_pcm_ptr, int(bool(pcm_is_float)), d_features_ptr, stride, n_frames,
                                                           hip_stream or None), "analyze_device_shard")

    def analysis_enable(self, max_frames: int = 1):
        """allocate the analysis state and the kernels' scratch for calls of up to max_frames frames (needed before a graph capture)"""
        self._chk(self.L.lpcnet_batch_analysis_enable(self.p, max_frames), "analysis_enable")

    def analysis_reset(self, first=0, count=None):
        self._chk(self.L.lpcnet_batch_analysis_reset(self.p, first, self.n - first if count is None else count), "analysis_reset")

    def get_analysis_state(self, stream: int) -> bytes:
        buf = C.create_string_buffer(self.L.lpcnet_batch_analysis_state_size())
        self._chk(self.L.lpcnet_batch_get_analysis_state(self.p, stream, buf), "get_analysis_state")
        return buf.raw

    def set_analysis_state(self, stream: int, raw: bytes):
        assert len(raw) == self.L.lpcnet_batch_analysis_state_size()
        self._chk(self.L.lpcnet_batch_set_analysis_state(self.p, stream, C.create_string_buffer(raw, len(raw))), "set_analysis_state")

    # ---- packet-loss concealment (lpcnet_plc_update / lpcnet_plc_conceal per stream, causal mode; include/lpcnet_batch.h) ----
    def plc_enable(self, options: int = PLC_CAUSAL):
        """PLC_CAUSAL or PLC_CODEC, optionally | PLC_DC_FILTER; resets every stream (PLC, synthesis and analysis state)"""
        self._chk(self.L.lpcnet_batch_plc_enable(self.p, options), "plc_enable")

    def plc_flavour(self) -> int:
        """0: the float PLC network runs, 1: the int8 one (the flavour of the batch's blob)"""
        rc = self.L.lpcnet_batch_plc_flavour(self.p)
        if rc < 0:
            self._chk(rc, "plc_flavour")
        return rc

    def plc_reset(self, first=0, count=None):
        self._chk(self.L.lpcnet_batch_plc_reset(self.p, first, self.n - first if count is None else count), "plc_reset")

    def plc_step(self, pcm: np.ndarray, lost) -> np.ndarray:
        """one 10-ms frame of every stream: pcm [n][160] int16 (received frames; rows of lost streams are ignored), lost [n] -> pcm [n][160]"""
        out = np.ascontiguousarray(pcm, np.int16).copy()
        lost = np.ascontiguousarray(lost, np.uint8)
        assert out.shape == (self.n, LPCNET_FRAME_SIZE) and lost.shape == (self.n,)
        self._chk(self.L.lpcnet_batch_plc_step(self.p, out, lost), "plc_step")
        return out

    def plc_step_device(self, d_pcm_ptr: int, lost, hip_stream: int = 0, shard=None):
        """enqueue only: d_pcm [n][160] int16 on the device, in and out; lost stays a host array"""
        lost = np.ascontiguousarray(lost, np.uint8)
        if shard is None:
            assert lost.shape == (self.n,)
            self._chk(self.L.lpcnet_batch_plc_step_device(self.p, d_pcm_ptr, lost, hip_stream), "plc_step_device")
        else:
            self._chk(self.L.lpcnet_batch_plc_step_device_shard(self.p, shard, d_pcm_ptr, lost, hip_stream), "plc_step_device_shard")

    def plc_fec_add(self, stream: int, features=None) -> int:
        """lpcnet_plc_fec_add: 20 features, or None for one skip; returns 1 when the ring was full and the vector was dropped"""
        if features is None:
            rc = self.L.lpcnet_batch_plc_fec_add(self.p, stream, None)
        else:
            f = np.ascontiguousarray(features, np.float32)
            assert f.shape == (20,)
            rc = self.L.lpcnet_batch_plc_fec_add(self.p, stream, f.ctypes.data)
        if rc < 0:
            self._chk(rc, "plc_fec_add")
        return rc

    def plc_fec_clear(self, stream: int):
        self._chk(self.L.lpcnet_batch_plc_fec_clear(self.p, stream), "plc_fec_clear")

    def plc_fec_feed(self, features, count, skip=None, clear=None) -> np.ndarray:
        """every stream's FEC traffic in one call: per stream lpcnet_plc_fec_clear if clear[s], skip[s] skips, then its count[s] vectors.  features is
        [sum(count)][20] float32, stream 0's vectors first, or a list of per-stream [k][20] arrays.  Returns dropped [n]: how many of each stream's
        vectors (the last ones) found the ring full"""
        count, skip, clear = _feed_args(self.n, count, skip, clear)
        if isinstance(features, (list, tuple)):
            assert len(features) == self.n
            rows = [np.asarray(f, np.float32).reshape(-1, 20) for f in features]
            assert [len(r) for r in rows] == count.tolist()
            features = np.concatenate(rows) if rows else np.zeros((0, 20), np.float32)
        f = np.ascontiguousarray(features, np.float32).reshape(-1, 20)
        assert (count < 0).any() or f.shape[0] == int(count.sum())
        dropped = np.zeros(self.n, np.int32)
        rc = self.L.lpcnet_batch_plc_fec_feed(self.p, f.ctypes.data, count.ctypes.data, None if skip is None else skip.ctypes.data,
                                              None if clear is None else clear.ctypes.data, dropped.ctypes.data)
        if rc < 0:
            self._chk(rc, "plc_fec_feed")
        return dropped

    def plc_fec_feed_device(self, d_features_ptr: int, count, skip=None, clear=None, hip_stream: int = 0, shard=None) -> np.ndarray:
        """enqueue only: d_features [sum(count)][20] float32 on the device; count, skip, clear stay host arrays (of the shard's streams with shard=k).
        Returns dropped, as plc_fec_feed does"""
        n = self.n if shard is None else self.shards[shard][1]
        count, skip, clear = _feed_args(n, count, skip, clear)
        dropped = np.zeros(n, np.int32)
        args = (d_features_ptr, count.ctypes.data, None if skip is None else skip.ctypes.data, None if clear is None else clear.ctypes.data,
                dropped.ctypes.data, hip_stream)
        rc = self.L.lpcnet_batch_plc_fec_feed_device(self.p, *args) if shard is None else self.L.lpcnet_batch_plc_fec_feed_device_shard(self.p, shard, *args)
        if rc < 0:
            self._chk(rc, "plc_fec_feed_device")
        return dropped

    # ---- DRED decoder (DRED_rdovae_decode_all per stream; include/lpcnet_batch.h) ----
    def dred_enable(self, max_latents: int):
        """upload the blob's DRED decoder and size the scratch for calls of up to max_latents latents per stream.  The decoder is served in its
        blob's own flavour: float arrays beside a float LPCNet model, int8 GRU arrays beside an int8 one"""
        self._chk(self.L.lpcnet_batch_dred_enable(self.p, max_latents), "dred_enable")

    def dred_flavour(self) -> int:
        """0: the float DRED decoder runs, 1: the int8 one (the flavour of the batch's blob)"""
        rc = self.L.lpcnet_batch_dred_flavour(self.p)
        if rc < 0:
            self._chk(rc, "dred_flavour")
        return rc

    def dred_info(self):
        """(max_latents, latent_dim, state_dim): the row lengths of dred_decode's arrays"""
        info = (C.c_int * 3)()
        self._chk(self.L.lpcnet_batch_dred_info(self.p, info), "dred_info")
        return tuple(info)

    def dred_form(self, S=None, n_streams=None) -> int:
        """S given: pin the streams a workgroup carries (1, 2, 4, 8; 0 = the engine's table).  Returns what a launch over n_streams (default: the
        batch's) streams runs with; the output bits are the same in every form"""
        if S is not None:
            self._chk(self.L.lpcnet_batch_dred_set_form(self.p, S), "dred_form")
        rc = self.L.lpcnet_batch_dred_get_form(self.p, self.n if n_streams is None else n_streams)
        if rc < 0:
            self._chk(rc, "dred_form")
        return rc

    @property
    def dred_fast(self) -> int:
        """the DRED decoder's arithmetic: 0 PARITY (the default: the bits of the reference's generic-C build), 1 FAST at the engine's tile, 16 or 32 FAST
        pinned to that many streams per workgroup (the same bits in either).  FAST is the fma-chain arithmetic of the reference's AVX2 float build on the fp32 matrix pipe; every
        dred_decode* call follows the switch.  Float decoders only"""
        rc = self.L.lpcnet_batch_dred_get_fast(self.p)
        if rc < 0:
            self._chk(rc, "dred_fast")
        return rc

    @dred_fast.setter
    def dred_fast(self, mode):
        self._chk(self.L.lpcnet_batch_dred_set_fast(self.p, int(mode)), "dred_fast")

    def dred_decode(self, state: np.ndarray, latents: np.ndarray, count, features: np.ndarray | None = None) -> np.ndarray:
        """state (n, state_dim), latents (n, max_latents, latent_dim) float32, count [n] -> features (n, 4 * max_latents, 20) float32: stream s's rows
        [0, 4 * count[s]) are DRED_rdovae_decode_all's output, the newest frame first; its other rows keep what `features` held (zeros without it)"""
        ml, ld, sd = self.dred_info()
        st, la = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(latents, np.float32)
        count = np.ascontiguousarray(count, np.int32)
        assert st.shape == (self.n, sd) and la.shape == (self.n, ml, ld) and count.shape == (self.n,)
        out = np.zeros((self.n, 4 * ml, 20), np.float32) if features is None else features
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (self.n, 4 * ml, 20)
        self._chk(self.L.lpcnet_batch_dred_decode(self.p, st.reshape(-1), la.reshape(-1), count.ctypes.data, out.reshape(-1)), "dred_decode")
        return out

    def dred_decode_device(self, d_state_ptr: int, d_latents_ptr: int, count, d_features_ptr: int, hip_stream: int = 0, shard=None):
        """enqueue only: device pointers laid out as dred_decode's arrays; count stays a host array (of the shard's streams with shard=k)"""
        n = self.n if shard is None else self.shards[shard][1]
        count = np.ascontiguousarray(count, np.int32)
        assert count.shape == (n,)
        args = (d_state_ptr, d_latents_ptr, count.ctypes.data, d_features_ptr, hip_stream or None)
        rc = self.L.lpcnet_batch_dred_decode_device(self.p, *args) if shard is None else self.L.lpcnet_batch_dred_decode_device_shard(self.p, shard, *args)
        self._chk(rc, "dred_decode_device")

    def dred_decode_packed(self, d_state_ptr: int, d_latents_ptr: int, count, first, take, hip_stream: int = 0, shard=None):
        """enqueue only: decode as dred_decode_device does and write rows first[s] .. first[s] + take[s] - 1 of every stream, the oldest frame first,
        into one packed [sum(take)][20] float32 array on the device -- a torch tensor, returned, whose data_ptr() plc_fec_feed_device takes with
        count = take.  count, first, take stay host arrays (of the shard's streams with shard=k)"""
        import torch
        n = self.n if shard is None else self.shards[shard][1]
        count, first, take = (np.ascontiguousarray(x, np.int32) for x in (count, first, take))
        assert count.shape == first.shape == take.shape == (n,)
        device = self.shards[0 if shard is None else shard][2]
        rows = int(take.clip(min=0).sum())                # (a negative take is the C call's to refuse)
        out = torch.empty((max(rows, 1), 20), dtype=torch.float32, device="cuda:%d" % device)[:rows]
        args = (d_state_ptr, d_latents_ptr, count.ctypes.data, first.ctypes.data, take.ctypes.data, out.data_ptr(), hip_stream or None)
        rc = self.L.lpcnet_batch_dred_decode_packed_device(self.p, *args) if shard is None else self.L.lpcnet_batch_dred_decode_packed_device_shard(self.p, shard, *args)
        self._chk(rc, "dred_decode_packed")
        return out

    # ---- the DRED decoder as a per-stream state (DRED_rdovae_dec_init_states / DRED_rdovae_decode_qframe per stream; include/lpcnet_batch.h) ----
    def dred_state_enable(self):
        """after dred_enable: allocate every stream's decoder record (dense2_state, dense4_state, dense6_state; all zero is DRED_rdovae_init_decoder).
        reset clears it, copy_streams / copy_streams_to / the roster carry it, snapshots hold it as section DRED_DEC"""
        self._chk(self.L.lpcnet_batch_dred_state_enable(self.p), "dred_state_enable")

    def dred_dec_state_size(self) -> int:
        """floats of one stream's three decoder states"""
        rc = self.L.lpcnet_batch_dred_dec_state_size(self.p)
        if rc < 0:
            self._chk(rc, "dred_dec_state_size")
        return rc

    def get_dred_dec_state(self, stream: int) -> np.ndarray:
        """one stream's decoder state in the reference's member order: dense2_state, dense4_state, dense6_state"""
        out = np.zeros(self.dred_dec_state_size(), np.float32)
        self._chk(self.L.lpcnet_batch_get_dred_dec_state(self.p, stream, out), "get_dred_dec_state")
        return out

    def set_dred_dec_state(self, stream: int, state: np.ndarray):
        st = np.ascontiguousarray(state, np.float32)
        assert st.shape == (self.dred_dec_state_size(),)
        self._chk(self.L.lpcnet_batch_set_dred_dec_state(self.p, stream, st), "set_dred_dec_state")

    def _dred_flags(self, which, n):
        if which is None:
            return None
        which = np.ascontiguousarray(which, np.int32)
        assert which.shape == (n,)
        return which

    def dred_init(self, state: np.ndarray, which=None):
        """state (n, state_dim) float32: dred_rdovae_dec_init_states into the record of every active stream with which[s] != 0 (None: every active
        stream); the other records keep their bits"""
        sd = self.dred_info()[2]
        st = np.ascontiguousarray(state, np.float32)
        assert st.shape == (self.n, sd)
        which = self._dred_flags(which, self.n)
        self._chk(self.L.lpcnet_batch_dred_init(self.p, st.reshape(-1), None if which is None else which.ctypes.data), "dred_init")

    def dred_init_device(self, d_state_ptr: int, which=None, hip_stream: int = 0, shard=None):
        """enqueue only: a device pointer laid out as dred_init's state; which stays a host array (of the shard's streams with shard=k) or None, the
        uniform form, which a capturing stream accepts"""
        n = self.n if shard is None else self.shards[shard][1]
        which = self._dred_flags(which, n)
        args = (d_state_ptr, None if which is None else which.ctypes.data, hip_stream or None)
        rc = self.L.lpcnet_batch_dred_init_device(self.p, *args) if shard is None else self.L.lpcnet_batch_dred_init_device_shard(self.p, shard, *args)
        self._chk(rc, "dred_init_device")

    def dred_step(self, latents: np.ndarray, start, count, features: np.ndarray | None = None) -> np.ndarray:
        """latents (n, max_latents, latent_dim) float32, start [n], count [n] -> features (n, 4 * max_latents, 20): stream s runs decode_qframe on
        latents start[s] .. start[s] + count[s] - 1 from its record and writes rows [4 * start[s], 4 * (start[s] + count[s])); its other rows keep
        what `features` held (zeros without it)"""
        ml, ld, _ = self.dred_info()
        la = np.ascontiguousarray(latents, np.float32)
        start, count = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(count, np.int32)
        assert la.shape == (self.n, ml, ld) and start.shape == count.shape == (self.n,)
        out = np.zeros((self.n, 4 * ml, 20), np.float32) if features is None else features
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (self.n, 4 * ml, 20)
        self._chk(self.L.lpcnet_batch_dred_step(self.p, la.reshape(-1), start.ctypes.data, count.ctypes.data, out.reshape(-1)), "dred_step")
        return out

    def dred_step_device(self, d_latents_ptr: int, start, count, d_features_ptr: int, hip_stream: int = 0, shard=None, first_latent: int = 0, n_latents: int = 0):
        """enqueue only: device pointers laid out as dred_step's arrays; start / count stay host arrays (of the shard's streams with shard=k).
        start=None, count=None: the uniform form -- latents first_latent .. first_latent + n_latents - 1 of every active stream -- which depends
        on nothing on the host and which a capturing stream accepts"""
        n = self.n if shard is None else self.shards[shard][1]
        assert (start is None) == (count is None)
        if start is not None:
            start, count = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(count, np.int32)
            assert start.shape == count.shape == (n,)
        args = (d_latents_ptr, None if start is None else start.ctypes.data, None if count is None else count.ctypes.data, int(first_latent), int(n_latents),
                d_features_ptr, hip_stream or None)
        rc = self.L.lpcnet_batch_dred_step_device(self.p, *args) if shard is None else self.L.lpcnet_batch_dred_step_device_shard(self.p, shard, *args)
        self._chk(rc, "dred_step_device")

    def dred_step_packed(self, d_latents_ptr: int, start, count, first, take, hip_stream: int = 0, shard=None):
        """enqueue only: step as dred_step_device does and write rows first[s] .. first[s] + take[s] - 1 of every stream -- the stream's own row
        numbers, inside the rows this call decodes -- the oldest frame first, into one packed [sum(take)][20] float32 array on the device: a torch
        tensor, returned, whose data_ptr() plc_fec_feed_device takes with count = take"""
        import torch
        n = self.n if shard is None else self.shards[shard][1]
        start, count, first, take = (np.ascontiguousarray(x, np.int32) for x in (start, count, first, take))
        assert start.shape == count.shape == first.shape == take.shape == (n,)
        device = self.shards[0 if shard is None else shard][2]
        rows = int(take.clip(min=0).sum())                # (a negative take is the C call's to refuse)
        out = torch.empty((max(rows, 1), 20), dtype=torch.float32, device="cuda:%d" % device)[:rows]
        args = (d_latents_ptr, start.ctypes.data, count.ctypes.data, first.ctypes.data, take.ctypes.data, out.data_ptr(), hip_stream or None)
        rc = self.L.lpcnet_batch_dred_step_packed_device(self.p, *args) if shard is None else self.L.lpcnet_batch_dred_step_packed_device_shard(self.p, shard, *args)
        self._chk(rc, "dred_step_packed")
        return out

    # ---- DRED encoder (DRED_rdovae_encode_dframe per stream and double frame; include/lpcnet_batch.h) ----
    def dred_enc_enable(self, max_dframes: int):
        """upload the blob's DRED encoder, allocate every stream's state (zero) and size the calls to up to max_dframes double frames per stream.
        The encoder is served in its blob's own flavour, like the decoder"""
        self._chk(self.L.lpcnet_batch_dred_enc_enable(self.p, max_dframes), "dred_enc_enable")

    def dred_enc_flavour(self) -> int:
        """0: the float DRED encoder runs, 1: the int8 one (the flavour of the batch's blob)"""
        rc = self.L.lpcnet_batch_dred_enc_flavour(self.p)
        if rc < 0:
            self._chk(rc, "dred_enc_flavour")
        return rc

    def dred_enc_info(self):
        """(max_dframes, 40, latent_dim, state_dim, taps, sum of the widths, floats of one stream's state)"""
        info = (C.c_int * 7)()
        self._chk(self.L.lpcnet_batch_dred_enc_info(self.p, info), "dred_enc_info")
        return tuple(info)

    def dred_enc_form(self, S=None, n_streams=None) -> int:
        """S given: pin the streams a workgroup carries (1, 2, 4, 8 where the buffers fit; 0 = the engine's table).  Returns what a launch over
        n_streams (default: the batch's) streams runs with; the output bits are the same in every form"""
        if S is not None:
            self._chk(self.L.lpcnet_batch_dred_enc_set_form(self.p, S), "dred_enc_form")
        rc = self.L.lpcnet_batch_dred_enc_get_form(self.p, self.n if n_streams is None else n_streams)
        if rc < 0:
            self._chk(rc, "dred_enc_form")
        return rc

    @property
    def dred_enc_fast(self) -> int:
        """the DRED encoder's arithmetic: 0 PARITY (the default: the bits of the reference's generic-C build), 1 FAST at the engine's tile, 16 or 32 FAST
        pinned to that many streams per workgroup (the same bits in either).  FAST is the fma-chain arithmetic of the reference's AVX2 float build on the
        fp32 matrix pipe; every dred_encode* call follows the switch, and the per-stream state is the same record in both.  Float encoders only"""
        rc = self.L.lpcnet_batch_dred_enc_get_fast(self.p)
        if rc < 0:
            self._chk(rc, "dred_enc_fast")
        return rc

    @dred_enc_fast.setter
    def dred_enc_fast(self, mode):
        self._chk(self.L.lpcnet_batch_dred_enc_set_fast(self.p, int(mode)), "dred_enc_fast")

    def dred_encode(self, features: np.ndarray, count, latents: np.ndarray | None = None, initial_state: np.ndarray | None = None):
        """features (n, 2 * max_dframes, stride >= 20) float32, count [n] -> (latents (n, max_dframes, latent_dim), initial_state (n, max_dframes,
        state_dim)): stream s's rows [0, count[s]) are DRED_rdovae_encode_dframe's outputs for its double frames in order; its other rows keep what
        the given arrays held (zeros without them).  Every stream's encoder state advances by its count"""
        md, _, ld, sd = self.dred_enc_info()[:4]
        f = np.ascontiguousarray(features, np.float32)
        count = np.ascontiguousarray(count, np.int32)
        assert f.ndim == 3 and f.shape[:2] == (self.n, 2 * md) and count.shape == (self.n,)
        lat = np.zeros((self.n, md, ld), np.float32) if latents is None else latents
        ini = np.zeros((self.n, md, sd), np.float32) if initial_state is None else initial_state
        for a, shape in ((lat, (self.n, md, ld)), (ini, (self.n, md, sd))):
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape
        self._chk(self.L.lpcnet_batch_dred_encode(self.p, f.reshape(-1), f.shape[2], count.ctypes.data, lat.reshape(-1), ini.reshape(-1)), "dred_encode")
        return lat, ini

    def dred_encode_device(self, d_features_ptr: int, stride: int, count, d_latents_ptr: int, d_initial_ptr: int, hip_stream: int = 0, shard=None):
        """enqueue only: device pointers laid out as dred_encode's arrays.  count: a host array (of the shard's streams with shard=k), or an int:
        that many double frames for every active stream -- the form a graph capture accepts"""
        n = self.n if shard is None else self.shards[shard][1]
        if isinstance(count, (int, np.integer)):
            cp, nd = None, int(count)
        else:
            count = np.ascontiguousarray(count, np.int32)
            assert count.shape == (n,)
            cp, nd = count.ctypes.data, 0
        args = (d_features_ptr, stride, cp, nd, d_latents_ptr, d_initial_ptr, hip_stream or None)
        rc = self.L.lpcnet_batch_dred_encode_device(self.p, *args) if shard is None else self.L.lpcnet_batch_dred_encode_device_shard(self.p, shard, *args)
        self._chk(rc, "dred_encode_device")

    def get_dred_enc_state(self, stream: int) -> np.ndarray:
        """one stream's encoder state: dense2_state, dense4_state, dense6_state, bits_dense_state (oldest tap first)"""
        out = np.zeros(self.dred_enc_info()[6], np.float32)
        self._chk(self.L.lpcnet_batch_dred_enc_get_state(self.p, stream, out), "get_dred_enc_state")
        return out

    def set_dred_enc_state(self, stream: int, state: np.ndarray):
        st = np.ascontiguousarray(state, np.float32)
        assert st.shape == (self.dred_enc_info()[6],)
        self._chk(self.L.lpcnet_batch_dred_enc_set_state(self.p, stream, st), "set_dred_enc_state")

    def get_plc_state(self, stream: int) -> bytes:
        buf = C.create_string_buffer(self.L.lpcnet_batch_plc_state_size())
        self._chk(self.L.lpcnet_batch_get_plc_state(self.p, stream, buf), "get_plc_state")
        return buf.raw

    def set_plc_state(self, stream: int, raw: bytes):
        assert len(raw) == self.L.lpcnet_batch_plc_state_size()
        self._chk(self.L.lpcnet_batch_set_plc_state(self.p, stream, C.create_string_buffer(raw, len(raw))), "set_plc_state")

    def plc_burg(self, x: np.ndarray) -> np.ndarray:
        """parity seam: burg_cepstral_analysis of one frame per stream, x [n][160] holding int16 values -> [n][36]"""
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.n, LPCNET_FRAME_SIZE)
        out = np.empty((self.n, 36), np.float32)
        self._chk(self.L.lpcnet_batch_plc_burg(self.p, x, out), "plc_burg")
        return out

    def plc_pred(self, in57: np.ndarray) -> np.ndarray:
        """parity seam: compute_plc_pred on every stream's network state (which advances), in57 [n][57] -> [n][20]"""
        x = np.ascontiguousarray(in57, np.float32)
        assert x.shape == (self.n, 57)
        out = np.empty((self.n, 20), np.float32)
        self._chk(self.L.lpcnet_batch_plc_pred(self.p, x, out), "plc_pred")
        return out

    def plc_pred_form(self, S=None, n_streams=None) -> int:
        """S given: pin the streams a workgroup of the PLC network's kernels carries (1, 2, 4, 8; 0 = the engine's table).  Returns what a prediction
        launch over n_streams (default: the batch's) streams runs with; the output bits are the same in every form"""
        if S is not None:
            self._chk(self.L.lpcnet_batch_plc_set_pred_form(self.p, S), "plc_pred_form")
        rc = self.L.lpcnet_batch_plc_get_pred_form(self.p, self.n if n_streams is None else n_streams)
        if rc < 0:
            self._chk(rc, "plc_pred_form")
        return rc

    def encode(self, pcm: np.ndarray) -> np.ndarray:
        """pcm (n, P*640) int16 -> packets (n, P, 8) uint8: lpcnet_encode per stream and packet (codebooks: set_codebooks)"""
        pcm = np.asarray(pcm)
        n, ns = pcm.shape
        assert n == self.n and ns % 640 == 0 and ns > 0 and pcm.dtype == np.int16
        P = ns // 640
        packets = np.zeros((n, P, 8), np.uint8)
        self._chk(self.L.lpcnet_batch_encode(self.p, np.ascontiguousarray(pcm).reshape(-1), packets.reshape(-1), P), "encode")
        return packets

    def encode_device(self, d_pcm_ptr: int, d_packets_ptr: int, n_packets: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_encode_device(self.p, d_pcm_ptr, d_packets_ptr, n_packets, hip_stream or None), "encode_device")

    def encode_device_shard(self, shard: int, d_pcm_ptr: int, d_packets_ptr: int, n_packets: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_encode_device_shard(self.p, shard, d_pcm_ptr, d_packets_ptr, n_packets, hip_stream or None), "encode_device_shard")

    def compute_features(self, pcm: np.ndarray) -> np.ndarray:
        """pcm (n, P*640) int16 -> features (n, 4P, 36) float32: lpcnet_compute_features per stream and packet"""
        pcm = np.asarray(pcm)
        n, ns = pcm.shape
        assert n == self.n and ns % 640 == 0 and ns > 0 and pcm.dtype == np.int16
        P = ns // 640
        feat = np.zeros((n, 4 * P, NB_TOTAL_FEATURES), np.float32)
        self._chk(self.L.lpcnet_batch_compute_features(self.p, np.ascontiguousarray(pcm).reshape(-1), feat.reshape(-1), NB_TOTAL_FEATURES, P), "compute_features")
        return feat

    def compute_features_device(self, d_pcm_ptr: int, d_features_ptr: int, stride: int, n_packets: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_compute_features_device(self.p, d_pcm_ptr, d_features_ptr, stride, n_packets, hip_stream or None), "compute_features_device")

    def encoder_enable(self, max_packets: int = 1):
        """allocate the analysis state, the encoder's vq_mem and the scratch for calls of up to max_packets packets (needed before a graph capture)"""
        self._chk(self.L.lpcnet_batch_encoder_enable(self.p, max_packets), "encoder_enable")

    def get_encoder_vq_mem(self, stream: int) -> np.ndarray:
        out = np.zeros(18, np.float32)
        self._chk(self.L.lpcnet_batch_get_encoder_vq_mem(self.p, stream, out), "get_encoder_vq_mem")
        return out

    def set_encoder_vq_mem(self, stream: int, mem: np.ndarray):
        mem = np.ascontiguousarray(mem, np.float32)
        assert mem.shape == (18,)
        self._chk(self.L.lpcnet_batch_set_encoder_vq_mem(self.p, stream, mem), "set_encoder_vq_mem")

    def get_decoder_vq_mem(self, stream: int) -> np.ndarray:
        out = np.zeros(18, np.float32)
        self._chk(self.L.lpcnet_batch_get_decoder_vq_mem(self.p, stream, out), "get_decoder_vq_mem")
        return out

    def set_decoder_vq_mem(self, stream: int, mem: np.ndarray):
        mem = np.ascontiguousarray(mem, np.float32)
        assert mem.shape == (18,)
        self._chk(self.L.lpcnet_batch_set_decoder_vq_mem(self.p, stream, mem), "set_decoder_vq_mem")

    # ---- streams that come and go (include/lpcnet_batch.h: lpcnet_batch_set_active, lpcnet_batch_copy_streams; lpcnet_amd/roster.py keeps the book) ----
    @property
    def active(self):
        """the active prefix: an int for an unsharded batch, a list with one count per shard otherwise.  Calls that advance streams work on the
        first `active` streams of every shard; array shapes stay (n, ...) and the other rows are neither read nor written"""
        k = self.L.lpcnet_batch_shards(self.p)
        arr = (C.c_int * k)()
        rc = self.L.lpcnet_batch_get_active(self.p, arr, k)
        if rc < 0:
            self._chk(rc, "get_active")
        return arr[0] if k == 1 else list(arr)

    @active.setter
    def active(self, counts):
        counts = [int(counts)] if np.isscalar(counts) else [int(c) for c in counts]
        arr = (C.c_int * len(counts))(*counts)
        self._chk(self.L.lpcnet_batch_set_active(self.p, arr, len(counts)), "set_active")

    @property
    def active_streams(self) -> int:
        rc = self.L.lpcnet_batch_active_streams(self.p)
        if rc < 0:
            self._chk(rc, "active_streams")
        return rc

    def copy_streams(self, src, dst, hip_stream: int = 0):
        """stream src[i] -> stream dst[i]: everything the batch keeps per stream, on the device (one launch per shard, only enqueued; pairs across
        shards: a gather, a transfer and a scatter per shard pair, only enqueued too).  All dst distinct, no stream in both lists"""
        src, dst = np.ascontiguousarray(src, np.int32).reshape(-1), np.ascontiguousarray(dst, np.int32).reshape(-1)
        assert src.size == dst.size
        self._chk(self.L.lpcnet_batch_copy_streams(self.p, src.ctypes.data, dst.ctypes.data, int(src.size), hip_stream or None), "copy_streams")

    # ---- stream snapshots (include/lpcnet_batch.h: lpcnet_batch_snapshot) ----
    def snapshot_layout(self):
        """the batch's present record: dict(sections [(id, bytes per stream, offset)], record_bytes)"""
        sec = np.zeros((_SNAP_LAYOUT_INTS // 3, 3), np.int32)
        rb = C.c_int(0)
        k = self.L.lpcnet_batch_snapshot_layout(self.p, sec.ctypes.data, sec.shape[0], C.byref(rb))
        if k < 0:
            self._chk(k, "snapshot_layout")
        return dict(sections=[tuple(int(x) for x in row) for row in sec[:k]], record_bytes=rb.value)

    def snapshot(self, streams) -> bytes:
        """the complete records of `streams` (distinct, any stream of the capacity) as one blob; copies out and synchronises"""
        st = np.ascontiguousarray(streams, np.int32).reshape(-1)
        buf = np.zeros((self.L.lpcnet_batch_snapshot_bytes(self.p, int(st.size)) + 3) // 4, np.int32)      # (4-byte aligned)
        self._chk(self.L.lpcnet_batch_snapshot(self.p, st.ctypes.data, int(st.size), buf.ctypes.data, buf.nbytes), "snapshot")
        return buf.tobytes()

    def restore(self, streams, blob: bytes):
        """record i of the blob -> stream streams[i] (the first len(streams) records); the blob's layout must match the batch"""
        st = np.ascontiguousarray(streams, np.int32).reshape(-1)
        self._chk(self.L.lpcnet_batch_restore(self.p, st.ctypes.data, int(st.size), bytes(blob), len(blob)), "restore")

    def snapshot_device(self, streams, d_records_ptr: int, hip_stream: int = 0, shard=None) -> np.ndarray:
        """enqueue only: the records of `streams` to device memory (len(streams) * record_bytes, 16-byte aligned).  Returns meta (m, 10) int32: the
        host halves, taken when the call is made.  shard: the shard's own indices and device"""
        st = np.ascontiguousarray(streams, np.int32).reshape(-1)
        meta = np.zeros((st.size, SNAP_META), np.int32)
        args = (st.ctypes.data, int(st.size), d_records_ptr, meta.ctypes.data, hip_stream or None)
        rc = self.L.lpcnet_batch_snapshot_device(self.p, *args) if shard is None else self.L.lpcnet_batch_snapshot_device_shard(self.p, shard, *args)
        self._chk(rc, "snapshot_device")
        return meta

    def restore_device(self, streams, d_records_ptr: int, meta, sections, hip_stream: int = 0, shard=None):
        """enqueue only: record i at d_records_ptr -> stream streams[i]; meta as snapshot_device returned it, sections as snapshot_layout()["sections"]
        of the batch the records came from"""
        st = np.ascontiguousarray(streams, np.int32).reshape(-1)
        meta = np.ascontiguousarray(meta, np.int32)
        sec = np.ascontiguousarray(sections, np.int32).reshape(-1, 3)
        assert meta.shape == (st.size, SNAP_META)
        args = (st.ctypes.data, int(st.size), d_records_ptr, meta.ctypes.data, sec.ctypes.data, sec.shape[0], hip_stream or None)
        rc = self.L.lpcnet_batch_restore_device(self.p, *args) if shard is None else self.L.lpcnet_batch_restore_device_shard(self.p, shard, *args)
        self._chk(rc, "restore_device")

    def copy_streams_to(self, src, other: "LPCNetBatch", dst):
        """stream src[i] of this batch -> stream dst[i] of `other`: gather, transfer, scatter on the device, only enqueued; this batch is unchanged"""
        src, dst = np.ascontiguousarray(src, np.int32).reshape(-1), np.ascontiguousarray(dst, np.int32).reshape(-1)
        assert src.size == dst.size
        self._chk(self.L.lpcnet_batch_copy_streams_to(self.p, src.ctypes.data, other.p, dst.ctypes.data, int(src.size)), "copy_streams_to")

    def set_lpc_gamma(self, gamma: float):
        self._chk(self.L.lpcnet_batch_set_lpc_gamma(self.p, gamma), "set_lpc_gamma")

    def set_end2end(self, on: bool = True):
        self._chk(self.L.lpcnet_batch_set_end2end(self.p, int(on)), "set_end2end")

    def set_fast(self, on=True):
        """FAST arithmetic (FMA / int32 accumulation); default is PARITY (bit-exact).  on = 2: FAST with the dual FC in fp16."""
        self._chk(self.L.lpcnet_batch_set_fast(self.p, int(on)), "set_fast")

    def decode_device(self, d_packets_ptr: int, d_pcm_ptr: int, n_packets: int, hip_stream: int = 0):
        self._chk(self.L.lpcnet_batch_decode_device(self.p, d_packets_ptr, d_pcm_ptr, n_packets, hip_stream or None), "decode_device")

    def decode(self, packets: np.ndarray) -> np.ndarray:
        n, P, _ = packets.shape
        pcm = np.zeros((n, P * 640), np.int16)
        self._chk(self.L.lpcnet_batch_decode(self.p, np.ascontiguousarray(packets, np.uint8).reshape(-1), pcm.reshape(-1), P), "decode")
        return pcm

    def run_tail(self, cond_a, cond_b, lpc, preload_pcm=None, preload=0) -> np.ndarray:
        n, T, _ = cond_a.shape
        pcm = np.zeros((n, T * 160), np.int16) if preload_pcm is None else np.ascontiguousarray(preload_pcm, np.int16).copy()
        self._chk(self.L.lpcnet_batch_run_tail(self.p, np.ascontiguousarray(cond_a, np.float32).reshape(-1),
                                               np.ascontiguousarray(cond_b, np.float32).reshape(-1),
                                               np.ascontiguousarray(lpc, np.float32).reshape(-1), pcm.reshape(-1), T, preload), "run_tail")
        return pcm

    def run_frames(self, features: np.ndarray):
        n, T, stride = features.shape
        ca = np.zeros((n, T, 1152), np.float32)
        cb = np.zeros((n, T, 48), np.float32)
        lpc = np.zeros((n, T, 16), np.float32)
        self._chk(self.L.lpcnet_batch_run_frames(self.p, np.ascontiguousarray(features, np.float32).reshape(-1), stride,
                                                 ca.ctypes.data, cb.ctypes.data, lpc.ctypes.data, T), "run_frames")
        return ca, cb, lpc

    def run_decode(self, packets: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
        """parity seam: the packet unpacker alone, packets (n, P, 8) uint8 -> features (n, 4P, 20) float32; only the decoder's VQ memory advances.
        `out` (C-contiguous float32, at least n * 4P * 20 floats) receives the rows instead of a fresh array: the rows of inactive streams stay"""
        n, P, _ = packets.shape
        assert n == self.n
        feat = np.zeros((n, 4 * P, NB_FEATURES), np.float32) if out is None else out
        assert feat.dtype == np.float32 and feat.flags.c_contiguous and feat.size >= n * 4 * P * NB_FEATURES
        self._chk(self.L.lpcnet_batch_run_decode(self.p, np.ascontiguousarray(packets, np.uint8).reshape(-1), feat.reshape(-1), P), "run_decode")
        return feat

    def get_state(self, stream: int) -> StreamState:
        st = StreamState()
        assert C.sizeof(st) == self.L.lpcnet_batch_state_size()
        self._chk(self.L.lpcnet_batch_get_raw_state(self.p, stream, C.byref(st)), "get_state")
        return st

    def set_state(self, stream: int, st: StreamState):
        self._chk(self.L.lpcnet_batch_set_raw_state(self.p, stream, C.byref(st)), "set_state")

    def tune(self):
        """measure the streams per workgroup now, on the engine's own stream (the enqueue-only device-pointer calls never do)"""
        self._chk(self.L.lpcnet_batch_tune(self.p), "tune")

    @property
    def streams_per_workgroup(self):
        return self.L.lpcnet_batch_get_streams_per_workgroup(self.p)

    @streams_per_workgroup.setter
    def streams_per_workgroup(self, s):
        self._chk(self.L.lpcnet_batch_set_streams_per_workgroup(self.p, s), "set_streams_per_workgroup")

    @property
    def twelve_waves(self):
        return self.L.lpcnet_batch_get_twelve_waves(self.p)

    @twelve_waves.setter
    def twelve_waves(self, mode):
        self._chk(self.L.lpcnet_batch_set_twelve_waves(self.p, int(mode)), "set_twelve_waves")

    @property
    def two_group_streaming(self):
        """the two-group kernel's streamed variants for this batch (models of 33 .. 96 items per lane; include/lpcnet_batch.h); off by default"""
        return bool(self.L.lpcnet_batch_get_two_group_streaming(self.p))

    @two_group_streaming.setter
    def two_group_streaming(self, on):
        self._chk(self.L.lpcnet_batch_set_two_group_streaming(self.p, 1 if on else 0), "set_two_group_streaming")

    @property
    def fast_two_group(self):
        """the two-group kernel under FAST fp32 arithmetic for this batch (set_fast(1); include/lpcnet_batch.h); off by default"""
        return bool(self.L.lpcnet_batch_get_fast_two_group(self.p))

    @fast_two_group.setter
    def fast_two_group(self, on):
        self._chk(self.L.lpcnet_batch_set_fast_two_group(self.p, 1 if on else 0), "set_fast_two_group")

    @property
    def group_schedule(self):
        """(form, lanes): how the compacted groups of a PLC step / synthesize_step launch (include/lpcnet_batch.h); (0, 1) = off"""
        f, l = C.c_int(), C.c_int()
        self._chk(self.L.lpcnet_batch_get_group_schedule(self.p, C.byref(f), C.byref(l)), "get_group_schedule")
        return f.value, l.value

    @group_schedule.setter
    def group_schedule(self, form_lanes):
        form, lanes = form_lanes
        self._chk(self.L.lpcnet_batch_set_group_schedule(self.p, int(form), int(lanes)), "set_group_schedule")

    def group_form(self, cnt: int) -> int:
        """streams per workgroup a group of cnt streams launches with under the present settings"""
        rc = self.L.lpcnet_batch_group_form(self.p, int(cnt))
        if rc < 0:
            self._chk(rc, "group_form")
        return rc

    def last_groups(self) -> np.ndarray:
        """[k][8] int32 {lane, slot, cnt, kind, N, preload, streams per workgroup, workgroups}: the groups of the most recent plc_step / synthesize_step of shard 0"""
        k = self.L.lpcnet_batch_last_groups(self.p, None, 0)
        if k < 0:
            self._chk(k, "last_groups")
        out = np.zeros((k, 8), np.int32)
        if k:
            self.L.lpcnet_batch_last_groups(self.p, out.ctypes.data, k)
        return out

    def enable_timing(self, on=True):
        self._chk(self.L.lpcnet_batch_enable_timing(self.p, int(on)), "enable_timing")

    def last_timing(self):
        a, b = C.c_float(), C.c_float()
        self._chk(self.L.lpcnet_batch_last_timing(self.p, C.byref(a), C.byref(b)), "last_timing")
        return a.value, b.value

    def debug_trace_alloc(self, n_samples):
        self._chk(self.L.lpcnet_batch_debug_trace(self.p, n_samples, None), "debug_trace")

    def debug_trace_fetch(self, n_samples):
        out = np.zeros((n_samples, 1600), np.float32)
        self._chk(self.L.lpcnet_batch_debug_trace(self.p, n_samples, out.ctypes.data), "debug_trace")
        return out

    def profile_reset(self):
        self._chk(self.L.lpcnet_batch_profile(self.p, None), "profile")

    def profile_fetch(self):
        out = np.zeros(96, np.uint64)
        self._chk(self.L.lpcnet_batch_profile(self.p, out.ctypes.data), "profile")
        return out
