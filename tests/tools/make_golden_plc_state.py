#!/usr/bin/env python3
"""Generate tests/golden/golden_plc_state_v1.npz from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so, the generic-C float build, and
liblpcnet_ref_gi.so, the generic-C int8 build; `make -C oracle ref`): the STATE of every LPCNetPLCState over the replays of
tests/tools/plc_state_replays.py, read through the accessors of oracle/ref_harness.c.  Data only:

  replays, field_names        the names the arrays below are indexed by
  ctl_<replay>   [T][n][9] int16   the reference's nine control ints after every frame, for every stream
  ckpt_<replay>  [K]               frames processed at each checkpoint
  crc_<replay>   [K][n][F] uint32  CRC-32 of every plc_state_map.fields() entry of every stream at every checkpoint
  snap_replay / snap_stream / snap_at [N], snap_why [N] (the predicates a snapshot was taken for, ';'-joined), snap_crc [N][F],
  snap_<member>  [N][...]          full snapshots (plc_state_map.SNAP_FIELDS), snap_cont [N][20][160] the reference's next 20 output frames
  blob_crc [2]                     CRC-32 of the float and of the int8 model blob

The generator asserts that the ints equal plc_model.PlcControl's, that `summary` / `fec_summary` and the PCM CRCs of golden_plc_v1.npz (and the
int8 fixture's) are reproduced, and it refuses to write unless the snapshots cover every predicate of PREDICATES.

    python tests/tools/make_golden_plc_state.py [OUT.npz]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
import plc_state_map as sm  # noqa: E402
import plc_state_replays as rp  # noqa: E402
from lpcnet_amd import synth  # noqa: E402
from oracle import ref as oref  # noqa: E402

GOLD = os.path.join(pm.ROOT, "tests", "golden")
MAX_BYTES = 350 * 1000
C = {k: i for i, k in enumerate(sm.CTL_NAMES)}


def blobs():
    return {"float": synth.blob_bytes(plc_synth.make_model_with_plc()), "int8": synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))}


def ref_crcs(st):
    return sm.crcs(*sm.from_reference(st.snapshot()))


def run_stream(lib, blob, ev, s, t_end, at=None):
    """stream s of a replay through the reference for t_end frames -> (out [t_end][160], ctl [t_end][9], {checkpoint: crcs}, snapshot at `at`),
    with plc_model.PlcControl run beside it: (ints [t_end][9], summaries [t_end][10])"""
    st = oref.RefPlc(lib, blob, ev.options)
    model = pm.PlcControl(ev.options)
    out = np.zeros((t_end, 160), np.int16)
    ctl = np.zeros((t_end, 9), np.int32)
    mctl = np.zeros((t_end, 9), np.int32)
    msum = np.zeros((t_end, 10), np.int32)
    crc, snap = {}, None
    for t in range(t_end):
        if t == at:
            snap = st.snapshot()
        ev.feed_ref(st, t, s)
        if ev.clear[t, s]:
            model.fec_clear()
        for _ in range(int(ev.skip[t, s])):
            model.fec_add(True)
        for _ in range(int(ev.count[t, s])):
            model.fec_add(False)
        out[t] = st.step(ev.frame(t, s), int(ev.lost[s, t]))
        msum[t] = model.step(int(ev.lost[s, t]))
        ctl[t] = st.ctl()
        mctl[t] = (model.pcm_fill, model.skip_analysis, model.blend, model.loss_count, model.fec_fill, model.fec_keep, model.fec_read,
                   model.fec_skip, model.fbuf)
        if t + 1 in ev.checkpoints:
            crc[t + 1] = ref_crcs(st)
    return out, ctl, crc, snap, mctl, msum


# name -> (replays it may come from, predicate on (ctl ints after `at` frames, next frame lost))
PREDICATES = {
    "mid_outage":             (("causal",), lambda c, nl: c[C["blend"]] == 1 and c[C["loss_count"]] >= 2),
    "long_outage_dc":         (("causal_dc",), lambda c, nl: c[C["loss_count"]] > 10),
    "before_received_causal": (("causal",), lambda c, nl: c[C["blend"]] == 1 and not nl),
    "before_received_codec":  (("codec",), lambda c, nl: c[C["blend"]] == 1 and not nl),
    "queue_pending":          (("codec_dc",), lambda c, nl: c[C["pcm_fill"]] in (80, 240) and nl),
    "fec_unread":             (("fec",), lambda c, nl: c[C["fec_fill"]] > c[C["fec_read"]] > 0 and nl),
    "fec_skip":               (("script", "fec"), lambda c, nl: c[C["fec_skip"]] > 0 and c[C["fec_fill"]] > c[C["fec_read"]] and nl),
    "fec_full":               (("script", "fec"), lambda c, nl: c[C["fec_fill"]] == 100),
    "fbuf_full":              (("codec_dc",), lambda c, nl: c[C["fbuf_fill"]] == 4 and nl),
    "i8_mid_outage":          (("i8",), lambda c, nl: c[C["blend"]] == 1 and c[C["loss_count"]] >= 2),
    "i8_before_received":     (("i8",), lambda c, nl: c[C["blend"]] == 1 and not nl),
}


def holds(name, ctl_row, next_lost):
    return bool(PREDICATES[name][1](ctl_row, next_lost))


def continuation_ok(ev, out, s, at):
    """the next 20 frames hold a lost frame, the concealed samples are not silence and no sample sits on +-32767"""
    lost = ev.lost[s, at:at + rp.CONT].astype(bool)
    c = out[s, at:at + rp.CONT]
    return bool(lost.any()) and (c[lost] != 0).mean() > 0.5 and np.abs(c.astype(np.int32)).max() < 32767


def choose(evs, ctls, outs):
    """one (replay, stream, at) per predicate, `at` + 20 on a checkpoint where the replay has such a triple and a continuation that proves something"""
    picked = {}
    for name, (replays, pred) in PREDICATES.items():
        found = None
        if any(r in replays and pred(ctls[r][at - 1, s], bool(evs[r].lost[s, at])) for r, s, at in picked):
            continue          # (a snapshot chosen for an earlier predicate covers this one)
        for r in replays:
            ev, ctl = evs[r], ctls[r]
            order = [c - rp.CONT for c in ev.checkpoints if c - rp.CONT > 0]
            order += [a for a in range(1, ev.T - rp.CONT) if a not in order]
            for at in order:
                for s in range(ev.n):
                    if pred(ctl[at - 1, s], bool(ev.lost[s, at])) and (r, s, at) not in picked and continuation_ok(ev, outs[r], s, at):
                        found = (r, s, at)
                        break
                if found:
                    break
            if found:
                break
        if found is None:
            raise SystemExit("no (replay, stream, frame) satisfies predicate %s: nothing written" % name)
        picked[found] = [name]
    for key in picked:          # ... and what else a chosen snapshot happens to cover
        r, s, at = key
        for name, (replays, pred) in PREDICATES.items():
            if r in replays and name not in picked[key] and pred(ctls[r][at - 1, s], bool(evs[r].lost[s, at])):
                picked[key].append(name)
    return picked


def main():
    libs = {"float": oref.RefLib("gf"), "int8": oref.RefLib("gi")}
    blob = blobs()
    gold = np.load(os.path.join(GOLD, "golden_plc_v1.npz"))
    gold_i8 = np.load(os.path.join(GOLD, "golden_plc_i8_v1.npz"))
    evs = {r: rp.Events(r) for r in rp.REPLAYS}
    save, ctls, outs = {}, {}, {}
    for r, ev in evs.items():
        res = [run_stream(libs[ev.flavour], blob[ev.flavour], ev, s, ev.T) for s in range(ev.n)]
        out = np.stack([x[0] for x in res])
        ctl = np.stack([x[1] for x in res], axis=1)
        assert np.array_equal(ctl, np.stack([x[4] for x in res], axis=1)), "%s: plc_model.PlcControl's ints differ from the reference's" % r
        msum = np.stack([x[5] for x in res], axis=1)
        if r in ("causal", "codec", "causal_dc", "codec_dc"):
            k = pm.OPTION_SETS.index(ev.options)
            assert np.array_equal(msum, gold["summary"][k % 2]) and np.array_equal(pm.block_crc(out), gold["pcm_crc"][k])
        elif r == "fec":
            assert np.array_equal(msum, gold["fec_summary"][:, :ev.n]) and np.array_equal(pm.block_crc(out), gold["fec_crc"][:ev.n])
        elif r == "i8":
            assert np.array_equal(pm.block_crc(out), gold_i8["pcm_crc"][pm.OPTION_SETS.index(ev.options)][:ev.n, :ev.T // pm.BLOCK])
        assert ctl.min() >= 0 and ctl.max() < 32768
        ctls[r], outs[r] = ctl, out
        save["ctl_" + r] = ctl.astype(np.int16)
        save["ckpt_" + r] = np.array(ev.checkpoints, np.int32)
        save["crc_" + r] = np.stack([np.stack([x[2][c] for x in res]) for c in ev.checkpoints])
        print(r, "lost frames", int(ev.lost.sum()), "checkpoints", ev.checkpoints, flush=True)
    picked = choose(evs, ctls, outs)
    snaps, cont, crc = [], [], []
    for (r, s, at), why in picked.items():
        ev = evs[r]
        out, _, _, snap, _, _ = run_stream(libs[ev.flavour], blob[ev.flavour], ev, s, at + rp.CONT, at=at)
        assert np.array_equal(out, outs[r][s, :at + rp.CONT]) and np.array_equal(snap["ctl"], ctls[r][at - 1, s])
        c = out[at:]
        assert continuation_ok(ev, outs[r], s, at), "a continuation without a lost frame, concealed to silence or with a sample on +-32767"
        if ev.options & 4 and snap["ctl"][C["blend"]] == 1:
            assert snap["dc"][0] != 0 and snap["dc"][1] != 0
            why.append("dc_nonzero")
        snaps.append(snap); cont.append(c); crc.append(sm.crcs(*sm.from_reference(snap)))
        print("snapshot", r, "stream", s, "after", at, "frames:", ";".join(why), "ctl", snap["ctl"].tolist(), flush=True)
    covered = {w for why in picked.values() for w in why}
    missing = (set(PREDICATES) | {"dc_nonzero"}) - covered
    if missing:
        raise SystemExit("predicates not covered: %s -- nothing written" % sorted(missing))
    n_f = sum(evs[k[0]].flavour == "float" for k in picked)
    assert n_f >= 8 and len(picked) - n_f >= 2
    names = list(rp.REPLAYS)
    save.update(replays=np.array(names), field_names=np.array(sm.FIELD_NAMES), snap_replay=np.array([names.index(k[0]) for k in picked], np.int32),
                snap_stream=np.array([k[1] for k in picked], np.int32), snap_at=np.array([k[2] for k in picked], np.int32),
                snap_why=np.array([";".join(w) for w in picked.values()]), snap_crc=np.stack(crc), snap_cont=np.stack(cont),
                blob_crc=np.array([zlib.crc32(blob["float"]), zlib.crc32(blob["int8"])], np.uint32))
    for k, (dt, _) in sm.SNAP_FIELDS.items():
        save["snap_" + k] = np.stack([np.asarray(s[k], dt) for s in snaps])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "golden_plc_state_v1.npz")
    tmp = out_path + ".tmp.npz"
    np.savez_compressed(tmp, **save)
    size = os.path.getsize(tmp)
    if size > MAX_BYTES:
        os.remove(tmp)
        import io
        for k, v in save.items():
            buf = io.BytesIO()
            np.savez_compressed(buf, x=v)
            print("  %-20s %7d bytes compressed" % (k, buf.getbuffer().nbytes))
        raise SystemExit("the fixture would be %d bytes (limit %d): nothing written" % (size, MAX_BYTES))
    os.replace(tmp, out_path)
    print("wrote", out_path, size, "bytes;", len(picked), "snapshots")


if __name__ == "__main__":
    main()
