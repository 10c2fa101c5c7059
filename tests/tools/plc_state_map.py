"""TEST TOOLING shared by tests/tools/make_golden_plc_state.py, tests/test_plc_state_host.py and tests/test_gpu_plc_state.py: the one translator
between the reference's LPCNetPLCState (src/lpcnet_private.h:28-106, read through the accessors of oracle/ref_harness.c) and the three records a
stream of the engine is made of -- lpcn_plc_state_rec (get / set_plc_state), lpcn_stream_state (get / set_raw_state) and lpcn_analysis_state
(get / set_analysis_state), lpcnet_amd/csrc/lpcnet_engine.h.

  from_reference(snapshot) -> (plc_rec, raw, an) bytes: what the three set_* calls take.  `snapshot` is a dict of the reference's own arrays
                              (SNAP_FIELDS below; what oracle.ref.RefPlc.snapshot returns and what the fixture's snap_* arrays hold).
  fields(plc_rec, raw, an) -> {name: bytes}: every compared field, cut to its LIVE EXTENT by the control ints of the record itself.  Both sides of
                              every comparison go through it: the engine's export directly, the reference's state through from_reference first.

FIELD_TABLE is the classification of every member of the three records (repeated in DESIGN.md §4.4)."""
import zlib

import numpy as np

f32 = np.float32
MAX_UNITS, MAX_FEC, NB_FEAT, QUEUE, FBUF = 512, 100, 20, 560, 4
EXC_LIVE = 416            # PITCH_MAX_PERIOD + FRAME_SIZE: what compute_frame_features carries over in exc_buf (src/lpcnet_enc.c)
CTL_NAMES = ("pcm_fill", "skip_analysis", "blend", "loss_count", "fec_fill", "fec_keep", "fec_read", "fec_skip", "fbuf_fill")

PLC_REC = np.dtype([("ctl", "<i4", 9), ("g1", "<i4"), ("g2", "<i4"), ("delta", "<i4"), ("dc", "<f8", 2), ("q", "<i2", QUEUE), ("feat", "<f4", NB_FEAT),
                    ("net", "<f4", (4, 2 * MAX_UNITS)), ("fec", "<f4", (MAX_FEC, NB_FEAT)), ("fbuf", "<f4", (FBUF, NB_FEAT)),
                    ("keep_a", "<f4", 1152), ("keep_b", "<f4", 48), ("keep_lpc", "<f4", 16)], align=True)
RAW = np.dtype([("gru_a", "<f4", 384), ("gru_b", "<f4", 16), ("conv1_mem", "<f4", 168), ("conv2_mem", "<f4", 256), ("old_lpc", "<f4", (2, 16)),
                ("last_sig", "<f4", 16), ("deemph_mem", "<f4"), ("last_exc", "<i4"), ("frame_count", "<i4"), ("rng", "<u4", 4), ("lpc", "<f4", 16),
                ("pad", "<i4", 3)])
AN = np.dtype([("analysis_mem", "<f4", 160), ("mem_preemph", "<f4"), ("pcount", "<i4"), ("pitch_mem", "<f4", 16), ("pitch_filt", "<f4"),
               ("exc_buf", "<f4", 576), ("pitch_max_path", "<f4", 224), ("pitch_max_path_all", "<f4"), ("best_i", "<i4")])

# The reference's arrays a snapshot is made of: name -> (dtype, shape); `net` is [4][g1 + g2] (plc_net, plc_copy[0..2]; each the gru1 then the
# gru2 state), `enc` the LPCNetEncState members of ref_enc_get_state, i.e. one AN record.
SNAP_FIELDS = {
    "ctl": (np.int32, (9,)), "pcm": (np.int16, (QUEUE,)), "features": (f32, (NB_FEAT,)), "net": (f32, (4, -1)), "dc": (np.float64, (2,)),
    "fec": (f32, (MAX_FEC, NB_FEAT)), "conv1": (f32, (168,)), "conv2": (f32, (256,)), "gru_a": (f32, (384,)), "gru_b": (f32, (16,)),
    "last_sig": (f32, (16,)), "last_exc": (np.int32, ()), "deemph_mem": (f32, ()), "frame_count": (np.int32, ()), "rng": (np.uint32, (4,)),
    "lpc": (f32, (16,)), "cond_a": (f32, (1152,)), "cond_b": (f32, (48,)), "old_lpc": (f32, (2, 16)), "feature_buffer": (f32, (FBUF * NB_FEAT,)),
    "enc": (np.uint8, (AN.itemsize,)), "g": (np.int32, (2,)),
}

# record member -> (reference member, class, note).  compared: the bytes of the live extent must equal the reference's.  derived: compared as
# well; the engine recomputes it from another field.  not kept: the engine does not keep the member like the reference, for the stated reason;
# from_reference still puts the reference's value there, and the import test (tests/test_gpu_plc_state.py) must pass with it.
FIELD_TABLE = (
    ("plc.ctl",            "pcm_fill .. fec_skip, lpcnet.feature_buffer_fill", "compared", "nine ints, the host half"),
    ("plc.g1, g2",         "sizeof plc_gru1_state / plc_gru2_state",           "compared", "part of the record's header; import refuses other widths"),
    ("plc.delta",          "-",                                                "scratch",  "the local `delta` of lpcnet_plc_update_causal, dead between steps"),
    ("plc.dc[0], dc[1]",   "dc_mem, syn_dc",                                   "compared", "doubles"),
    ("plc.q",              "pcm[560]",                                         "compared", "samples [0, pcm_fill)"),
    ("plc.feat",           "features[0..20)",                                  "compared", ""),
    ("plc.net[0..3]",      "plc_net, plc_copy[0], [1], [2]",                   "compared", "g1 + g2 floats each, one field per slot"),
    ("plc.fec",            "fec[100][20]",                                     "compared", "rows [0, fec_fill)"),
    ("plc.fbuf",           "lpcnet.feature_buffer",                            "compared", "rows [0, fbuf_fill)"),
    ("plc.keep_a, keep_b", "lpcnet.gru_a_condition, gru_b_condition",          "compared", ""),
    ("plc.keep_lpc",       "lpcnet.lpc",                                       "compared", ""),
    ("raw.gru_a .. conv2", "lpcnet.nnet",                                      "compared", ""),
    ("raw.old_lpc",        "lpcnet.old_lpc[2][16]",                            "compared", ""),
    ("raw.last_sig, deemph_mem, last_exc, frame_count, rng", "the same members of lpcnet", "compared", ""),
    ("raw.lpc",            "lpcnet.lpc",                                       "compared", "the second copy of keep_lpc"),
    ("an.analysis_mem, mem_preemph, pitch_filt, pitch_max_path, pitch_max_path_all, best_i", "the same members of enc", "compared",
     "pitch_max_path is row 0, cells [0, 224)"),
    ("an.pcount",          "enc.pcount",                                       "compared", "0 after every PLC step on both sides"),
    ("an.pitch_mem",       "enc.pitch_mem",                                    "derived",  "= analysis_mem[79 - j]; the kernels read analysis_mem"),
    ("an.exc_buf",         "enc.exc_buf[576]",                                 "compared", "cells [0, 416); no code on either side writes the rest"),
)


def _arr(snapshot, name):
    dt, shape = SNAP_FIELDS[name]
    return np.asarray(snapshot[name], dt).reshape(shape)


def from_reference(snapshot):
    """the reference's arrays -> (lpcn_plc_state_rec, lpcn_stream_state, lpcn_analysis_state) as bytes"""
    g1, g2 = (int(x) for x in _arr(snapshot, "g"))
    G = g1 + g2
    p = np.zeros((), PLC_REC)
    p["ctl"] = _arr(snapshot, "ctl")
    p["g1"], p["g2"] = g1, g2
    p["dc"] = _arr(snapshot, "dc")
    p["q"] = _arr(snapshot, "pcm")
    p["feat"] = _arr(snapshot, "features")
    net = _arr(snapshot, "net")
    assert net.shape == (4, G)
    p["net"][:, :G] = net
    p["fec"] = _arr(snapshot, "fec")
    p["fbuf"] = _arr(snapshot, "feature_buffer").reshape(FBUF, NB_FEAT)
    p["keep_a"], p["keep_b"], p["keep_lpc"] = _arr(snapshot, "cond_a"), _arr(snapshot, "cond_b"), _arr(snapshot, "lpc")
    r = np.zeros((), RAW)
    r["gru_a"], r["gru_b"] = _arr(snapshot, "gru_a"), _arr(snapshot, "gru_b")
    r["conv1_mem"], r["conv2_mem"] = _arr(snapshot, "conv1"), _arr(snapshot, "conv2")
    r["old_lpc"], r["last_sig"] = _arr(snapshot, "old_lpc"), _arr(snapshot, "last_sig")
    r["deemph_mem"], r["last_exc"], r["frame_count"] = _arr(snapshot, "deemph_mem"), _arr(snapshot, "last_exc"), _arr(snapshot, "frame_count")
    r["rng"], r["lpc"] = _arr(snapshot, "rng"), _arr(snapshot, "lpc")
    an = _arr(snapshot, "enc").tobytes()
    return p.tobytes(), r.tobytes(), an


def fields(plc_rec, raw, an):
    """-> {name: bytes} of every compared field, each cut to its live extent by the record's own control ints"""
    p = np.frombuffer(plc_rec, PLC_REC)[0]
    r = np.frombuffer(raw, RAW)[0]
    a = np.frombuffer(an, AN)[0]
    ctl = dict(zip(CTL_NAMES, (int(x) for x in p["ctl"])))
    G = int(p["g1"]) + int(p["g2"])
    clip = lambda v, hi: max(0, min(hi, v))
    out = {"ctl": p["ctl"], "units": np.array([p["g1"], p["g2"]], "<i4"), "dc_mem": p["dc"][0:1], "syn_dc": p["dc"][1:2],
           "pcm": p["q"][:clip(ctl["pcm_fill"], QUEUE)], "features": p["feat"],
           "plc_net": p["net"][0, :G], "plc_copy0": p["net"][1, :G], "plc_copy1": p["net"][2, :G], "plc_copy2": p["net"][3, :G],
           "fec": p["fec"][:clip(ctl["fec_fill"], MAX_FEC)], "feature_buffer": p["fbuf"][:clip(ctl["fbuf_fill"], FBUF)],
           "gru_a_condition": p["keep_a"], "gru_b_condition": p["keep_b"], "lpc": p["keep_lpc"]}
    for k in ("gru_a", "gru_b", "conv1_mem", "conv2_mem", "old_lpc", "last_sig"):
        out[k] = r[k]
    # (the scalars of a record are one entry: the fixture holds a CRC per entry, stream and checkpoint)
    out["deemph_exc_count_rng"] = b"".join(r[k].tobytes() for k in ("deemph_mem", "last_exc", "frame_count", "rng"))
    out["raw_lpc"] = r["lpc"]
    for k in ("analysis_mem", "pitch_mem", "pitch_max_path"):
        out["enc_" + k] = a[k]
    out["enc_scalars"] = b"".join(a[k].tobytes() for k in ("mem_preemph", "pcount", "pitch_filt", "pitch_max_path_all", "best_i"))
    out["enc_exc_buf"] = a["exc_buf"][:EXC_LIVE]
    return {k: v if isinstance(v, bytes) else np.ascontiguousarray(v).tobytes() for k, v in out.items()}


FIELD_NAMES = tuple(fields(np.zeros((), PLC_REC).tobytes(), np.zeros((), RAW).tobytes(), np.zeros((), AN).tobytes()))


def crcs(plc_rec, raw, an):
    """[len(FIELD_NAMES)] uint32: CRC-32 of every fields() entry, in FIELD_NAMES order"""
    f = fields(plc_rec, raw, an)
    return np.array([zlib.crc32(f[k]) for k in FIELD_NAMES], np.uint32)


def differing(got_crc, want_crc):
    """names of the fields whose CRCs differ"""
    return [FIELD_NAMES[i] for i in np.flatnonzero(np.asarray(got_crc) != np.asarray(want_crc))]


def diff_report(got, want):
    """the differing entries of two fields() dicts, one line each: the name, the sizes, how many bytes differ and where the first one is"""
    lines = []
    for k in FIELD_NAMES:
        g, w = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
        if g.size != w.size:
            lines.append("%s: %d bytes against %d" % (k, g.size, w.size))
        elif not np.array_equal(g, w):
            d = np.flatnonzero(g != w)
            lines.append("%s: %d of %d bytes differ, the first at byte %d" % (k, d.size, g.size, int(d[0])))
    return lines
