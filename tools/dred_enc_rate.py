#!/usr/bin/env python3
"""Device time of one DRED encode (lpcnet_batch_dred_encode_device) of a large batch, in every form of the kernel.

    python tools/dred_enc_rate.py OUT.json       (profiles/dred_enc_rate.json when run for the record)
    python tools/dred_enc_rate.py --int8 OUT.json       (profiles/dred_enc_i8_rate.json: the int8 encoder beside the float one)
    python tools/dred_enc_rate.py --fast OUT.json       (profiles/dred_enc_fast_rate.json: the FAST flavour beside PARITY)

For 256, 2 048 and 8 192 streams at the widths of the training defaults, at two operating points -- one double frame per call (two 10-ms
frames: the 20-ms real-time step) and 50 double frames per call (one second) -- the time of one call (HIP events around the enqueue-only device-pointer call in its uniform form, on
a caller's stream) with the streams per workgroup pinned to 1, 2, 4, 8 and left to the engine's table.  The forms alternate call by call inside
one process and one batch, so that every form sees the same clocks; per form two warm-up calls, then the median, the extremes and the 10th /
90th percentiles of at least 20 timed calls.  `spread_ms` of a row is the widest 10th-to-90th range among its forms: what a difference between
two medians has to beat.  Every form's output from a freshly reset state is compared with form 1's, bit for bit.  Where oracle/_ref exists the
tool also times one stream on the reference's AVX2 + FMA float build (liblpcnet_ref_af.so), the encoder chained from its layer functions as
tests/tools/make_golden_dred_enc.py chains it, on one core: the CPU yardstick.  One process; the tool stops at the first failure.  Run it under a
time limit.
--int8: the same widths as an int8 (DOT_PROD) blob (tests/tools/dred_i8_model.py) on a second batch beside the float one; flavours and forms
alternate call by call in the one process, so that int8 and float see the same clocks.  `rows` holds the int8 rows, `float_rows` the float rows
of the same session, `int8_over_float` the ratio of the medians per row at the table's form and at each flavour's best pinned form; the CPU
yardstick is the reference's AVX2 int8 build (liblpcnet_ref_ai.so).
--fast (profiles/dred_enc_fast_rate.json): PARITY at the table's form beside the FAST flavour (lpcnet_batch_dred_enc_set_fast) pinned to every tile
that is built and at the engine's tile (mode 1), on one batch: the four alternate call by call in rotating order, the same protocol and rows.  A
row's `spread_ms` is the widest 10th-to-90th range among its four columns; the three FAST columns' outputs from a freshly reset state are compared bit
for bit, and the largest |FAST - PARITY| is recorded.
    timeout -k 10 600 python tools/dred_enc_rate.py profiles/dred_enc_rate.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

FORMS = (1, 2, 4, 8, 0)
STREAMS = (256, 2048, 8192)
DFRAMES = (1, 50)
TIMED, WARMUP = 20, 2


def cpu_yardstick(blob, feat, int8=False):
    """one stream's chain on the reference's af build (int8: ai), best of three: ms per double frame"""
    path = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_ai.so" if int8 else "liblpcnet_ref_af.so")
    if not os.path.exists(path):
        return None
    import make_golden_dred_enc as mg
    enc = mg.RefEncoder(mg.load_ref(path), blob)
    n = feat.shape[0] // 2
    best = None
    for _ in range(3):
        st = np.zeros(enc.state_floats, np.float32)
        t0 = time.perf_counter()
        for d in range(n):
            enc.encode_dframe(st, np.concatenate([feat[2 * d], feat[2 * d + 1]]))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return dict(build="ai (AVX2, int8 GRUs)" if int8 else "af (AVX2 + FMA, float)", dframes=int(n), ms_per_dframe=1e3 * best / n,
                note="one stream, one core, through ctypes: two calls per layer, the window assembled in NumPy")


def form_rows(n, nd, ms, runs):
    """one (stream count, double frames per call) row from the timed calls of every form"""
    row = dict(streams=n, dframes=nd, table_form=runs[0], forms=[])
    for f in FORMS:
        v = np.array(ms[f])
        row["forms"].append(dict(form=f, streams_per_workgroup=runs[f], median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()),
                                 p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)),
                                 us_per_stream_dframe=float(1e3 * np.median(v) / (n * nd))))
    pinned = [r for r in row["forms"] if r["form"]]
    best = min(pinned, key=lambda r: r["median_ms"])
    row["spread_ms"] = max(r["p90_ms"] - r["p10_ms"] for r in row["forms"])
    row["best_pinned_form"] = best["form"]
    row["table_within_spread_of_best"] = bool(row["forms"][-1]["median_ms"] <= best["median_ms"] + row["spread_ms"])
    row["best_wide_form_gain_over_one_ms"] = float(pinned[0]["median_ms"] - min(r["median_ms"] for r in pinned[1:]))
    return row


def measure(out_path, int8=False):
    import torch
    import dred_enc_model as em
    from lpcnet_amd import api
    dev = torch.device("cuda:0")
    blobs = {"float": em.set_blob("tf")}
    if int8:
        import dred_i8_model as di
        blobs["int8"] = di.blob_enc("tf")
    main = "int8" if int8 else "float"
    info = api.dred_enc_model_info(blobs[main])
    base = em.inputs(64, max(DFRAMES), seed=0x2A7F)
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), flavour=main, widths=info["widths"], latent_dim=info["latent_dim"],
                  taps=info["taps"], timed_calls=TIMED, warmup_calls=WARMUP,
                  note="forms%s alternate call by call in one process; ms of one encode call by HIP events" % (" and flavours" if int8 else ""), rows=[])
    if int8:
        result["float_rows"], result["int8_over_float"] = [], []
    s = torch.cuda.Stream()
    for n in STREAMS:
        for nd in DFRAMES:
            batch = {}
            for fl, blob in blobs.items():
                batch[fl] = api.LPCNetBatch(n, blob)
                batch[fl].dred_enc_enable(nd)
                assert batch[fl].dred_enc_flavour() == (fl == "int8")
            d_feat = torch.from_numpy(np.ascontiguousarray(np.tile(base[:, :2 * nd], (n // 64 + 1, 1, 1))[:n])).to(dev)
            d_lat = torch.zeros((n, nd, info["latent_dim"]), dtype=torch.float32, device=dev)
            d_init = torch.zeros((n, nd, info["state_dim"]), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ms = {fl: {f: [] for f in FORMS} for fl in blobs}
            runs = {fl: {} for fl in blobs}
            want = {fl: None for fl in blobs}
            with torch.cuda.stream(s):
                for k in range(WARMUP + TIMED):
                    for f in FORMS[k % len(FORMS):] + FORMS[:k % len(FORMS)]:      # (rotated: every form follows every other one equally often)
                        for fl, b in batch.items():
                            runs[fl][f] = b.dred_enc_form(f)
                            if k == 0:
                                b.reset()
                            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record(s)
                            b.dred_encode_device(d_feat.data_ptr(), 20, nd, d_lat.data_ptr(), d_init.data_ptr(), hip_stream=s.cuda_stream)
                            e.record(s)
                            e.synchronize()
                            if k >= WARMUP:
                                ms[fl][f].append(a.elapsed_time(e))
                            elif k == 0:
                                got = torch.cat([d_lat.reshape(n, -1), d_init.reshape(n, -1)], 1).clone()
                                if want[fl] is None:
                                    want[fl] = got
                                elif not torch.equal(got.view(torch.int32), want[fl].view(torch.int32)):
                                    raise SystemExit("%s: form %d differs from form 1 at %d streams" % (fl, f, n))
            for b in batch.values():
                b.dred_enc_form(0)
                b.close()
            rows = {fl: form_rows(n, nd, ms[fl], runs[fl]) for fl in blobs}
            print(json.dumps(rows), flush=True)
            result["rows"].append(rows[main])
            if int8:
                result["float_rows"].append(rows["float"])
                med = lambda row, form: [r for r in row["forms"] if r["form"] == form][0]["median_ms"]
                result["int8_over_float"].append(dict(streams=n, dframes=nd, table_form=med(rows["int8"], 0) / med(rows["float"], 0),
                                                      best_pinned_form=med(rows["int8"], rows["int8"]["best_pinned_form"]) / med(rows["float"], rows["float"]["best_pinned_form"]),
                                                      spread_ms=max(rows["int8"]["spread_ms"], rows["float"]["spread_ms"])))
    result["cpu_reference"] = cpu_yardstick(blobs[main], base[0, :20], int8)
    print(json.dumps(dict(cpu_reference=result["cpu_reference"], int8_over_float=result.get("int8_over_float"))), flush=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


FAST_TILES = (16, 32)           # every tile that is built (lpcnet_batch_dred_enc_set_fast)


def measure_fast(out_path):
    import torch
    import dred_enc_model as em
    from lpcnet_amd import api
    dev = torch.device("cuda:0")
    blob = em.set_blob("tf")
    info = api.dred_enc_model_info(blob)
    base = em.inputs(64, max(DFRAMES), seed=0x2A7F)
    modes = [("parity", 0)] + [("fast_T%d" % t, t) for t in FAST_TILES] + [("fast", 1)]
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), widths=info["widths"], latent_dim=info["latent_dim"], taps=info["taps"],
                  timed_calls=TIMED, warmup_calls=WARMUP,
                  note="PARITY (table form) and FAST alternate call by call, in rotating order, in one process; ms of one encode call by HIP events", rows=[])
    s = torch.cuda.Stream()
    for n in STREAMS:
        for nd in DFRAMES:
            b = api.LPCNetBatch(n, blob)
            b.dred_enc_enable(nd)
            d_feat = torch.from_numpy(np.ascontiguousarray(np.tile(base[:, :2 * nd], (n // 64 + 1, 1, 1))[:n])).to(dev)
            d_lat = torch.zeros((n, nd, info["latent_dim"]), dtype=torch.float32, device=dev)
            d_init = torch.zeros((n, nd, info["state_dim"]), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in modes}
            first = {}
            with torch.cuda.stream(s):
                for k in range(WARMUP + TIMED):
                    for name, mode in modes[k % len(modes):] + modes[:k % len(modes)]:      # (rotated: every column follows every other one equally often)
                        b.dred_enc_fast = mode
                        if k == 0:
                            b.reset()
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(s)
                        b.dred_encode_device(d_feat.data_ptr(), 20, nd, d_lat.data_ptr(), d_init.data_ptr(), hip_stream=s.cuda_stream)
                        e.record(s)
                        e.synchronize()
                        if k >= WARMUP:
                            ms[name].append(a.elapsed_time(e))
                        elif k == 0:
                            first[name] = torch.cat([d_lat.reshape(n, -1), d_init.reshape(n, -1)], 1).clone()
            tile = 16 if (n + 15) // 16 <= torch.cuda.get_device_properties(0).multi_processor_count else 32      # (the engine's rule for mode 1)
            b.dred_enc_fast = 0
            table_form = b.dred_enc_form()
            b.close()
            for name, mode in modes[2:]:
                if not torch.equal(first[name].view(torch.int32), first[modes[1][0]].view(torch.int32)):
                    raise SystemExit("%s differs from %s at %d streams" % (name, modes[1][0], n))
            row = dict(streams=n, dframes=nd, parity_table_form=table_form, mode1_tile=tile,
                       max_abs_fast_minus_parity=float((first["fast"] - first["parity"]).abs().max()), modes=[])
            for name, mode in modes:
                v = np.array(ms[name])
                row["modes"].append(dict(mode=name, set_fast=mode, median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()),
                                         p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)),
                                         us_per_stream_dframe=float(1e3 * np.median(v) / (n * nd))))
            med = {r["mode"]: r["median_ms"] for r in row["modes"]}
            spr = {r["mode"]: r["p90_ms"] - r["p10_ms"] for r in row["modes"]}
            row["spread_ms"] = max(spr.values())
            row["fast_gain_over_parity_ms"] = med["parity"] - med["fast"]
            row["fast_beats_parity_by_more_than_the_two_spreads"] = bool(row["fast_gain_over_parity_ms"] > spr["parity"] + spr["fast"])
            print(json.dumps(row), flush=True)
            result["rows"].append(row)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        raise SystemExit(__doc__)
    if "--fast" in sys.argv[1:]:
        measure_fast(args[0])
    else:
        measure(args[0], int8="--int8" in sys.argv[1:])
