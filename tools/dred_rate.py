#!/usr/bin/env python3
"""Device time of one DRED decode (lpcnet_batch_dred_decode_device) of a large batch, in every form of the kernel.

    python tools/dred_rate.py OUT.json [latents]       (profiles/dred_rate.json when run for the record)
    python tools/dred_rate.py --int8 OUT.json [latents]       (profiles/dred_i8_rate.json: the int8 decoder beside the float one)
    python tools/dred_rate.py --fast OUT.json [latents]       (profiles/dred_fast_rate.json: the FAST flavour beside PARITY)
    python tools/dred_rate.py --resume OUT.json [latents]     (profiles/dred_stream_rate.json: init + steps on a kept state beside the one-shot call)

For 256, 2 048 and 8 192 streams, 25 latents each (one second of redundancy) at the exported width of 256: the time of one call (HIP events
around the enqueue-only device-pointer call, on a caller's stream) with the streams per workgroup pinned to 1, 2, 4, 8 and left to the engine's
table.  The forms alternate call by call inside one process and one batch, so that every form sees the same clocks; per form two warm-up calls,
then the median, the extremes and the 10th / 90th percentiles of at least 20 timed calls.  `spread_ms` of a stream count is the widest
10th-to-90th range among its forms: what a difference between two medians has to beat.  Every form's output is compared with form 1's, bit for
bit.  Where oracle/_ref exists the tool also times one stream on the reference's AVX2 + FMA float build (liblpcnet_ref_af.so), the decoder
chained from its layer functions as tests/tools/make_golden_dred.py chains it, on one core: the CPU yardstick.  One process; the tool stops at
the first failure.
--int8: the same blob widths as an int8 (DOT_PROD) blob (tests/tools/dred_i8_model.py) on a second batch beside the float one; flavours and forms
alternate call by call in the one process, so that int8 and float see the same clocks.  `streams` holds the int8 rows, `float_streams` the float
rows of the same session, `int8_over_float` the ratio of the medians per stream count at the table's form and at each flavour's best pinned form;
the CPU yardstick is the reference's AVX2 int8 build (liblpcnet_ref_ai.so).
--fast (profiles/dred_fast_rate.json): PARITY at the table's form beside the FAST flavour (lpcnet_batch_dred_set_fast) pinned to every tile that is
built and at the engine's choice (mode 1), alternating call by call on one batch; the same protocol and stream counts.  FAST's output is compared with
the pinned tile's bit for bit and its largest deviation from PARITY's is recorded.
--resume (profiles/dred_stream_rate.json): the decoder as a per-stream state (lpcnet_batch_dred_init / _dred_step) beside the one-shot call, PARITY and
FAST, at the same stream counts and width: init + 25 uniform steps of one latent against one dred_decode of 25; "5, then 5 more" -- init + step(0, 5),
then step(5, 5) -- against dred_decode of 5 followed by dred_decode of 10; a captured replay of init + step(5) against the eager pair.  The scenarios
alternate inside one process and one batch; each is timed by HIP events around all of its calls.  The stepped features are compared with
dred_decode's bit for bit.  The `decode_25` column is the one-shot call's time in this session: what `--fast` reports as `parity` and `fast`.
Run it under a time limit:
    timeout -k 10 600 python tools/dred_rate.py profiles/dred_rate.json
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
TIMED, WARMUP = 20, 2


def cpu_yardstick(blob, state, latents, int8=False):
    """one stream's chain on the reference's af build (int8: ai), best of three: ms per latent"""
    path = os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_ai.so" if int8 else "liblpcnet_ref_af.so")
    if not os.path.exists(path):
        return None
    import make_golden_dred as mg
    dec = mg.RefDecoder(mg.load_ref(path), blob)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        dec.decode(state, latents, latents.shape[0])
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return dict(build="ai (AVX2, int8 GRUs)" if int8 else "af (AVX2 + FMA, float)", latents=int(latents.shape[0]), ms_per_latent=1e3 * best / latents.shape[0],
                note="one stream, one core, through ctypes: two calls per layer")


def form_rows(n, n_latents, ms, runs):
    """one stream count's row from the timed calls of every form"""
    row = dict(streams=n, table_form=runs[0], forms=[])
    for f in FORMS:
        v = np.array(ms[f])
        row["forms"].append(dict(form=f, streams_per_workgroup=runs[f], median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()),
                                 p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)),
                                 us_per_stream_latent=float(1e3 * np.median(v) / (n * n_latents))))
    pinned = [r for r in row["forms"] if r["form"]]
    best = min(pinned, key=lambda r: r["median_ms"])
    row["spread_ms"] = max(r["p90_ms"] - r["p10_ms"] for r in row["forms"])
    row["best_pinned_form"] = best["form"]
    row["table_within_spread_of_best"] = bool(row["forms"][-1]["median_ms"] <= best["median_ms"] + row["spread_ms"])
    row["best_wide_form_gain_over_one_ms"] = float(pinned[0]["median_ms"] - min(r["median_ms"] for r in pinned[1:]))
    return row


def measure(out_path, n_latents=25, int8=False):
    import torch
    import dred_model as dm
    from lpcnet_amd import api
    dev = torch.device("cuda:0")
    blobs = {"float": dm.set_blob("w256")}
    if int8:
        import dred_i8_model as di
        blobs["int8"] = di.blob_dec("w256")
    main = "int8" if int8 else "float"
    info = api.dred_model_info(blobs[main])
    base_state, base_lat = dm.inputs(info["latent_dim"], 64, n_latents, seed=0x2A7E)
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), flavour=main, widths=info["widths"], latent_dim=info["latent_dim"],
                  latents=n_latents, timed_calls=TIMED, warmup_calls=WARMUP,
                  note="forms%s alternate call by call in one process; ms of one decode call by HIP events" % (" and flavours" if int8 else ""), streams=[])
    if int8:
        result["float_streams"], result["int8_over_float"] = [], []
    s = torch.cuda.Stream()
    for n in STREAMS:
        batch = {}
        for fl, blob in blobs.items():
            batch[fl] = api.LPCNetBatch(n, blob)
            batch[fl].dred_enable(n_latents)
            assert batch[fl].dred_flavour() == (fl == "int8")
        reps = n // 64 + 1
        d_state = torch.from_numpy(np.ascontiguousarray(np.tile(base_state, (reps, 1))[:n])).to(dev)
        d_lat = torch.from_numpy(np.ascontiguousarray(np.tile(base_lat, (reps, 1, 1))[:n])).to(dev)
        d_out = torch.zeros((n, 4 * n_latents, 20), dtype=torch.float32, device=dev)
        count = np.full(n, n_latents, np.int32)
        torch.cuda.synchronize()
        ms = {fl: {f: [] for f in FORMS} for fl in blobs}
        runs = {fl: {} for fl in blobs}
        want = {fl: None for fl in blobs}
        with torch.cuda.stream(s):
            for k in range(WARMUP + TIMED):
                for f in FORMS:
                    for fl, b in batch.items():
                        runs[fl][f] = b.dred_form(f)
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(s)
                        b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), count, d_out.data_ptr(), hip_stream=s.cuda_stream)
                        e.record(s)
                        e.synchronize()
                        if k >= WARMUP:
                            ms[fl][f].append(a.elapsed_time(e))
                        elif k == 0:
                            got = d_out.clone()
                            if want[fl] is None:
                                want[fl] = got
                            elif not torch.equal(got.view(torch.int32), want[fl].view(torch.int32)):
                                raise SystemExit("%s: form %d differs from form 1 at %d streams" % (fl, f, n))
        for b in batch.values():
            b.dred_form(0)
            b.close()
        rows = {fl: form_rows(n, n_latents, ms[fl], runs[fl]) for fl in blobs}
        print(json.dumps(rows), flush=True)
        result["streams"].append(rows[main])
        if int8:
            result["float_streams"].append(rows["float"])
            med = lambda row, form: [r for r in row["forms"] if r["form"] == form][0]["median_ms"]
            result["int8_over_float"].append(dict(streams=n, table_form=med(rows["int8"], 0) / med(rows["float"], 0),
                                                  best_pinned_form=med(rows["int8"], rows["int8"]["best_pinned_form"]) / med(rows["float"], rows["float"]["best_pinned_form"]),
                                                  spread_ms=max(rows["int8"]["spread_ms"], rows["float"]["spread_ms"])))
    result["cpu_reference"] = cpu_yardstick(blobs[main], base_state[0], base_lat[0], int8)
    print(json.dumps(dict(cpu_reference=result["cpu_reference"], int8_over_float=result.get("int8_over_float"))), flush=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


FAST_TILES = (16, 32)           # every tile that is built (lpcnet_batch_dred_set_fast)


def measure_fast(out_path, n_latents=25):
    import torch
    import dred_model as dm
    from lpcnet_amd import api
    dev = torch.device("cuda:0")
    blob = dm.set_blob("w256")
    info = api.dred_model_info(blob)
    base_state, base_lat = dm.inputs(info["latent_dim"], 64, n_latents, seed=0x2A7E)
    modes = [("parity", 0)] + [("fast_T%d" % t, t) for t in FAST_TILES] + [("fast", 1)]
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), widths=info["widths"], latent_dim=info["latent_dim"], latents=n_latents,
                  timed_calls=TIMED, warmup_calls=WARMUP, note="PARITY (table form) and FAST alternate call by call in one process; ms of one decode call by HIP events",
                  streams=[])
    s = torch.cuda.Stream()
    for n in STREAMS:
        b = api.LPCNetBatch(n, blob)
        b.dred_enable(n_latents)
        reps = n // 64 + 1
        d_state = torch.from_numpy(np.ascontiguousarray(np.tile(base_state, (reps, 1))[:n])).to(dev)
        d_lat = torch.from_numpy(np.ascontiguousarray(np.tile(base_lat, (reps, 1, 1))[:n])).to(dev)
        d_out = torch.zeros((n, 4 * n_latents, 20), dtype=torch.float32, device=dev)
        count = np.full(n, n_latents, np.int32)
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in modes}
        first = {}
        with torch.cuda.stream(s):
            for k in range(WARMUP + TIMED):
                for name, mode in modes:
                    b.dred_fast = mode
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s)
                    b.dred_decode_device(d_state.data_ptr(), d_lat.data_ptr(), count, d_out.data_ptr(), hip_stream=s.cuda_stream)
                    e.record(s)
                    e.synchronize()
                    if k >= WARMUP:
                        ms[name].append(a.elapsed_time(e))
                    elif k == 0:
                        first[name] = d_out.clone()
        table_form = b.dred_form()
        b.dred_fast = 0
        b.close()
        for name, mode in modes[2:]:
            if not torch.equal(first[name].view(torch.int32), first[modes[1][0]].view(torch.int32)):
                raise SystemExit("%s differs from %s at %d streams" % (name, modes[1][0], n))
        row = dict(streams=n, parity_table_form=table_form, max_abs_fast_minus_parity=float((first["fast"] - first["parity"]).abs().max()), modes=[])
        for name, mode in modes:
            v = np.array(ms[name])
            row["modes"].append(dict(mode=name, set_fast=mode, median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()),
                                     p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)),
                                     us_per_stream_latent=float(1e3 * np.median(v) / (n * n_latents))))
        med = {r["mode"]: r["median_ms"] for r in row["modes"]}
        row["spread_ms"] = max(r["p90_ms"] - r["p10_ms"] for r in row["modes"])
        row["fast_gain_over_parity_ms"] = med["parity"] - med["fast"]
        row["fast_beats_parity_by_more_than_the_spread"] = bool(row["fast_gain_over_parity_ms"] > row["spread_ms"])
        print(json.dumps(row), flush=True)
        result["streams"].append(row)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def measure_resume(out_path, n_latents=25):
    import torch
    import dred_model as dm
    from lpcnet_amd import api
    dev = torch.device("cuda:0")
    blob = dm.set_blob("w256")
    info = api.dred_model_info(blob)
    base_state, base_lat = dm.inputs(info["latent_dim"], 64, n_latents, seed=0x2A7E)
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), widths=info["widths"], latent_dim=info["latent_dim"], latents=n_latents,
                  timed_calls=TIMED, warmup_calls=WARMUP,
                  note="scenarios and arithmetics alternate in one process and one batch; ms of all calls of a scenario by HIP events on a caller's stream", streams=[])
    s = torch.cuda.Stream()
    for n in STREAMS:
        b = api.LPCNetBatch(n, blob)
        b.dred_enable(n_latents)
        b.dred_state_enable()
        reps = n // 64 + 1
        d_state = torch.from_numpy(np.ascontiguousarray(np.tile(base_state, (reps, 1))[:n])).to(dev)
        d_lat = torch.from_numpy(np.ascontiguousarray(np.tile(base_lat, (reps, 1, 1))[:n])).to(dev)
        d_out = torch.zeros((n, 4 * n_latents, 20), dtype=torch.float32, device=dev)
        d_step = torch.zeros((n, 4 * n_latents, 20), dtype=torch.float32, device=dev)
        full, five, ten = (np.full(n, k, np.int32) for k in (n_latents, 5, 10))
        sp, lp = d_state.data_ptr(), d_lat.data_ptr()
        torch.cuda.synchronize()

        def decode(count, out=d_out):
            b.dred_decode_device(sp, lp, count, out.data_ptr(), hip_stream=s.cuda_stream)

        def init():
            b.dred_init_device(sp, hip_stream=s.cuda_stream)

        def step(first, k):
            b.dred_step_device(lp, None, None, d_step.data_ptr(), hip_stream=s.cuda_stream, first_latent=first, n_latents=k)

        def one_by_one():
            init()
            for l in range(n_latents):
                step(l, 1)

        def resume():
            init()
            step(0, 5)
            step(5, 5)

        def again():
            decode(five)
            decode(ten)

        def pair():
            init()
            step(0, 5)

        graphs = {}
        row = dict(streams=n, modes=[])
        with torch.cuda.stream(s):
            for mode in (0, 1):                        # a graph per arithmetic: the launch is chosen when it is captured
                b.dred_fast = mode
                pair()
                s.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    b.dred_init_device(sp, hip_stream=torch.cuda.current_stream().cuda_stream)
                    b.dred_step_device(lp, None, None, d_step.data_ptr(), hip_stream=torch.cuda.current_stream().cuda_stream, first_latent=0, n_latents=5)
                graphs[mode] = g
            scen = [("decode_25", lambda m: decode(full)), ("init_and_25_steps_of_one", lambda m: one_by_one()), ("decode_5_then_decode_10", lambda m: again()),
                    ("init_step_5_then_step_5", lambda m: resume()), ("eager_init_step_5", lambda m: pair()), ("captured_init_step_5", lambda m: graphs[m].replay())]
            ms = {(mode, name): [] for mode in (0, 1) for name, _ in scen}
            for k in range(WARMUP + TIMED):
                for mode in (0, 1):
                    b.dred_fast = mode
                    for name, fn in scen:
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(s)
                        fn(mode)
                        e.record(s)
                        e.synchronize()
                        if k >= WARMUP:
                            ms[mode, name].append(a.elapsed_time(e))
                        elif k == 0 and name == "init_and_25_steps_of_one" and not torch.equal(d_step.view(torch.int32), d_out.view(torch.int32)):
                            raise SystemExit("mode %d: the stepped features differ from dred_decode's at %d streams" % (mode, n))
                        elif k == 0 and name == "captured_init_step_5":
                            got = d_step[:, :20].clone()
                            decode(five, d_step)
                            s.synchronize()
                            if not torch.equal(got.view(torch.int32), d_step[:, :20].view(torch.int32)):
                                raise SystemExit("mode %d: the captured replay differs from dred_decode's at %d streams" % (mode, n))
        for mode in (0, 1):
            cols = {}
            for name, _ in scen:
                v = np.array(ms[mode, name])
                cols[name] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
            spread = max(c["p90_ms"] - c["p10_ms"] for c in cols.values())
            med = {k: c["median_ms"] for k, c in cols.items()}
            row["modes"].append(dict(mode="fast" if mode else "parity", set_fast=mode, scenarios=cols, spread_ms=spread,
                                     steps_of_one_over_decode_25=med["init_and_25_steps_of_one"] / med["decode_25"],
                                     resume_gain_over_decoding_again_ms=med["decode_5_then_decode_10"] - med["init_step_5_then_step_5"],
                                     capture_gain_over_eager_ms=med["eager_init_step_5"] - med["captured_init_step_5"]))
        b.dred_fast = 0
        b.close()
        print(json.dumps(row), flush=True)
        result["streams"].append(row)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        raise SystemExit(__doc__)
    if "--resume" in sys.argv[1:]:
        measure_resume(args[0], int(args[1]) if len(args) > 1 else 25)
    elif "--fast" in sys.argv[1:]:
        measure_fast(args[0], int(args[1]) if len(args) > 1 else 25)
    else:
        measure(args[0], int(args[1]) if len(args) > 1 else 25, int8="--int8" in sys.argv[1:])
