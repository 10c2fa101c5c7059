#!/usr/bin/env python3
"""Device time of one packet-loss concealment step (lpcnet_batch_plc_step_device) of a large batch under several loss patterns.

    python tools/plc_rate.py [--int8] OUT.json [streams]       (profiles/plc_rate_<streams>.json, plc_rate_int8_<streams>.json when run for the record)

For 8192 streams (default) in LPCNET_PLC_CAUSAL mode: the step time (HIP events around the enqueue-only device-pointer call, on a
caller's stream) in a steady state of 0 %, 5 % and 20 % independent random loss per stream and frame, and through a burst outage
(every stream loses the same 10 frames, then receives again: the step times of the outage and of the 6 frames after it, where the PCM queue
drains, are listed one by one).  Each random-loss figure is the median, minimum and maximum over the steps after a warm-up of 30 steps, with the
share of steps that had no lost stream at all.  Beside them: one frame of analyze_device on the same batch, the cost the loss-free step is
compared with.  --int8 builds the int8 test model (int8 sample kernels and the int8 PLC network) instead of the float one.  One process; the tool stops at the first failure.  Run it under a time limit:
    timeout -k 10 900 python tools/plc_rate.py profiles/plc_rate.json

    python tools/plc_rate.py --fec K [--fec-loop] OUT.json [streams]       (profiles/plc_rate_fec.json holds the runs made for the record)

With --fec K every stream is given K redundancy vectors before each step, in LPCNET_PLC_CODEC mode with 5 % random loss: one
lpcnet_batch_plc_fec_feed_device on the caller's stream, then the step, timed together and apart with HIP events.  Every stream's ring fills at
the same step (100 / K steps after the reset) and from then on every feed compacts every ring, so the steps are reported in two windows: while
the rings fill, and with full rings.  Beside them: the step without any FEC traffic, and the host-pointer feed (lpcnet_batch_plc_fec_feed,
which uploads and synchronises) by the host's clock.  --fec-loop feeds through the per-stream lpcnet_batch_plc_fec_add instead, one call per
vector, and times loop + step by the host's clock: what the batched feed replaces.

    python tools/plc_rate.py [--int8] [--schedule FORM,LANES]... --ab OUT.json [streams]       (profiles/plc_rate_schedule.json, plc_rate_schedule_int8.json)

The group schedule (lpcnet_batch_set_group_schedule).  --schedule FORM,LANES alone sets it for any of the runs above.  --ab compares: ONE batch in one
process, the schedule switched between blocks of steps -- off, then each --schedule given (default 1,1 0,2 0,4 1,4), round after round -- so that
every variant sees the same clocks, the same state history and the same loss flags' statistics.  Per loss pattern (0 %, 5 %, 20 % random loss, the
outage and its recovery) it prints every variant's median over all its blocks, the medians of its single blocks, and the ratio to the off median;
the spread between the off blocks' medians is the noise a ratio has to beat.  The steps are timed like the runs above.

    python tools/plc_rate.py [--widths D1,G1,G2]... [--pred-form S]... [--loss P]... --forms OUT.json [streams[,streams...]]       (profiles/plc_pred_forms.json)

The PLC network's kernels at 1, 2, 4, 8 streams per workgroup (LPCNetBatch.plc_pred_form).  --widths D1,G1,G2 gives the blob a PLC network of those
widths (tests/tools/plc_model.blob_widths) and --pred-form S pins the form, for the first run above too.  --forms compares: for the float and the
int8 model, each --widths and each number of streams, one batch whose form is switched between blocks of steps -- the table's choice, 1, 2, 4, 8,
or the --pred-form values given -- at each --loss P (default 0: the step of a call without loss).  Run on a build without the forms it measures
that build alone, as "parent".
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def step_ms(torch, b, d, lost, s):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    b.plc_step_device(d.data_ptr(), lost, s.cuda_stream)
    e.record(s)
    e.synchronize()
    return a.elapsed_time(e)


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), steps=len(ms))


def measure_ab(out_path, n, schedules, int8=False, rounds=4, block=12):
    import torch
    import plc_synth
    from lpcnet_amd import api, synth
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(n, synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8" if int8 else "float")))
    b.plc_enable(api.PLC_CAUSAL)
    b.tune()
    T = 100
    base = np.stack([synth.make_pcm(700 + k, T).reshape(T, 160) for k in range(64)])
    frames = [torch.from_numpy(np.ascontiguousarray(np.tile(base[:, t], (n // 64 + 1, 1))[:n])).to(dev) for t in range(T)]
    d = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    rng = np.random.default_rng(7)
    variants = [(0, 1)] + [v for v in schedules if v != (0, 1)]
    name = lambda v: "off" if v == (0, 1) else "form %d, lanes %d" % v
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), streams=n, options="LPCNET_PLC_CAUSAL", flavour="int8" if int8 else "float",
                  streams_per_workgroup=b.streams_per_workgroup, rounds=rounds, steps_per_block=block, group_form_of={},
                  note="one batch, one process; the schedule alternates between blocks of steps; ratio = median / the off median of the same pattern", patterns=[])
    b.group_schedule = (1, 1)
    result["group_form_of"] = {str(c): b.group_form(c) for c in (n // 20, n // 5, n) if c >= 1}
    b.group_schedule = (0, 1)

    def report(pattern, blocks):
        off = float(np.median(np.concatenate(blocks[(0, 1)])))
        row = dict(pattern=pattern, variants=[])
        for v in variants:
            med = float(np.median(np.concatenate(blocks[v])))
            row["variants"].append(dict(schedule=name(v), form=v[0], lanes=v[1], median_ms=med, block_medians_ms=[float(np.median(x)) for x in blocks[v]], ratio_to_off=med / off))
        bm = row["variants"][0]["block_medians_ms"]
        row["off_block_spread"] = (max(bm) - min(bm)) / off
        print(json.dumps(row), flush=True)
        result["patterns"].append(row)

    with torch.cuda.stream(s):
        t = 0
        for p in (0.0, 0.05, 0.20):
            b.group_schedule = (0, 1)
            b.plc_reset()
            blocks = {v: [] for v in variants}
            for _ in range(30):
                d.copy_(frames[t % T]); step_ms(torch, b, d, (rng.uniform(size=n) < p).astype(np.uint8), s); t += 1
            for _ in range(rounds):
                for v in variants:
                    b.group_schedule = v
                    ms = []
                    for _ in range(block):
                        d.copy_(frames[t % T]); ms.append(step_ms(torch, b, d, (rng.uniform(size=n) < p).astype(np.uint8), s)); t += 1
                    blocks[v].append(ms)
            report("random loss %g %%" % (100 * p), blocks)
        # the outage: every stream loses the same 10 frames, then receives again; the 10 steps of the outage and the 6 after it, where the PCM queue drains
        out_b, rec_b = {v: [] for v in variants}, {v: [] for v in variants}
        for _ in range(rounds):
            for v in variants:
                b.group_schedule = (0, 1)
                b.plc_reset()
                for k in range(12):
                    d.copy_(frames[k]); step_ms(torch, b, d, np.zeros(n, np.uint8), s)
                b.group_schedule = v
                seq = []
                for k in range(12, 12 + 10 + 6):
                    d.copy_(frames[k % T]); seq.append(step_ms(torch, b, d, np.full(n, 1 if k < 22 else 0, np.uint8), s))
                out_b[v].append(seq[:10]); rec_b[v].append(seq[10:])
        report("outage: every stream lost, 10 frames", out_b)
        report("recovery: the 6 frames after the outage", rec_b)
    b.group_schedule = (0, 1)
    b.sync()
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def plc_blob(int8, widths=None):
    """the test model with the 128 / 16 / 16 PLC network, or (--widths) with one of the given widths (tests/tools/plc_model.blob_widths)"""
    import plc_model
    import plc_synth
    from lpcnet_amd import synth
    if widths:
        return plc_model.blob_widths(*widths, "int8" if int8 else "float")
    return synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8" if int8 else "float"))


def measure_forms(out_path, streams, widths_list, losses, pinned=None, rounds=3, block=8):
    """The prediction kernels' forms side by side: per (flavour, widths, streams, loss) ONE batch, the form switched between blocks of steps -- the
    table's choice, then 1, 2, 4, 8 pinned (or the --pred-form values alone), round after round -- so that every form sees the same clocks and the
    same history.  A library without the forms (the parent build) runs as the single variant "parent".  Per variant: the median over all its
    steps, its blocks' medians and the form a launch over all streams runs with; spread = (largest - smallest block median) / median of the
    first variant, the noise a difference between variants has to beat."""
    import torch
    from lpcnet_amd import api, synth
    dev = torch.device("cuda:0")
    has_forms = hasattr(api.LPCNetBatch, "plc_pred_form")
    variants = ["parent"] if not has_forms else list(pinned) if pinned else [0, 1, 2, 4, 8]
    T = 100
    base = np.stack([synth.make_pcm(700 + k, T).reshape(T, 160) for k in range(64)])
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), options="LPCNET_PLC_CAUSAL", rounds=rounds, steps_per_block=block,
                  note="one batch per row, one process; the form alternates between blocks of steps; variant 0 = the table's choice", rows=[])
    s = torch.cuda.Stream()
    for int8 in (False, True):
        for widths in widths_list:
            blob = plc_blob(int8, widths)
            for n in streams:
                b = api.LPCNetBatch(n, blob)
                b.plc_enable(api.PLC_CAUSAL)
                frames = [torch.from_numpy(np.ascontiguousarray(np.tile(base[:, t], (n // 64 + 1, 1))[:n])).to(dev) for t in range(T)]
                d = torch.zeros((n, 160), dtype=torch.int16, device=dev)
                with torch.cuda.stream(s):
                    for p in losses:
                        rng = np.random.default_rng(7)
                        b.plc_reset()
                        t = 0
                        for _ in range(20):
                            d.copy_(frames[t % T]); step_ms(torch, b, d, (rng.uniform(size=n) < p).astype(np.uint8), s); t += 1
                        blocks = {v: [] for v in variants}
                        forms = {}
                        for _ in range(rounds):
                            for v in variants:
                                if has_forms:
                                    forms[v] = b.plc_pred_form(v)
                                ms = []
                                for _ in range(block):
                                    d.copy_(frames[t % T]); ms.append(step_ms(torch, b, d, (rng.uniform(size=n) < p).astype(np.uint8), s)); t += 1
                                blocks[v].append(ms)
                        first = float(np.median(np.concatenate(blocks[variants[0]])))
                        bm0 = [float(np.median(x)) for x in blocks[variants[0]]]
                        row = dict(flavour="int8" if int8 else "float", widths=list(widths or (128, 16, 16)), streams=n, loss=p, spread=(max(bm0) - min(bm0)) / first, variants=[])
                        for v in variants:
                            row["variants"].append(dict(pinned=v, form=forms.get(v), median_ms=float(np.median(np.concatenate(blocks[v]))),
                                                        block_medians_ms=[float(np.median(x)) for x in blocks[v]]))
                        print(json.dumps(row), flush=True)
                        result["rows"].append(row)
                if has_forms:
                    b.plc_pred_form(0)
                b.sync()
                b.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def measure(out_path, n, int8=False, schedule=None, widths=None, pred_form=None):
    import torch
    from lpcnet_amd import api, synth
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(n, plc_blob(int8, widths))
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_flavour() == int(int8)
    b.tune()
    if schedule:
        b.group_schedule = schedule
    if pred_form is not None:
        b.plc_pred_form(pred_form)
    T = 100
    base = np.stack([synth.make_pcm(700 + k, T).reshape(T, 160) for k in range(64)])
    frames = [torch.from_numpy(np.ascontiguousarray(np.tile(base[:, t], (n // 64 + 1, 1))[:n])).to(dev) for t in range(T)]
    d = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    feat = torch.zeros((n, 1, 36), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    rng = np.random.default_rng(7)
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), streams=n, options="LPCNET_PLC_CAUSAL", flavour="int8" if int8 else "float",
                  streams_per_workgroup=b.L.lpcnet_batch_get_streams_per_workgroup(b.p), group_schedule=list(b.group_schedule),
                  plc_widths=list(widths or (128, 16, 16)), pred_form=b.plc_pred_form(), random_loss=[], burst=None)
    with torch.cuda.stream(s):
        for p in (0.0, 0.05, 0.20):
            b.plc_reset()
            ms, lost_streams = [], []
            for t in range(30 + 120):
                lost = (rng.uniform(size=n) < p).astype(np.uint8)
                d.copy_(frames[t % T])
                m = step_ms(torch, b, d, lost, s)
                if t >= 30:
                    ms.append(m); lost_streams.append(int(lost.sum()))
            row = dict(loss=p, mean_lost_streams_per_step=float(np.mean(lost_streams)), **stats(ms))
            print(json.dumps(row), flush=True)
            result["random_loss"].append(row)
        b.plc_reset()
        for t in range(30):
            d.copy_(frames[t]); step_ms(torch, b, d, np.zeros(n, np.uint8), s)
        seq = []
        for t in range(30, 30 + 10 + 6):
            lost = np.full(n, 1 if t < 40 else 0, np.uint8)
            d.copy_(frames[t % T])
            seq.append(dict(frame=t - 30, lost=bool(t < 40), ms=float(step_ms(torch, b, d, lost, s))))
        result["burst"] = seq
        print(json.dumps(seq), flush=True)
        an = []
        for t in range(40):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s); b.analyze_device(frames[t].data_ptr(), False, feat.data_ptr(), 36, 1, s.cuda_stream); e.record(s)
            e.synchronize()
            if t >= 5:
                an.append(a.elapsed_time(e))
        result["analyze_device_one_frame"] = stats(an)
        print(json.dumps(result["analyze_device_one_frame"]), flush=True)
    b.sync()
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def fec_windows(K, steps, warm):
    """step ranges while every ring still fills and after every ring is full (each stream gets K vectors per step from a reset)"""
    return dict(rings_filling=(warm, min(steps, 95 // K)), rings_full=(min(steps, -(-100 // K) + 10), steps))


def measure_fec(out_path, n, K, loop=False, int8=False, schedule=None):
    import time
    import torch
    import plc_synth
    from lpcnet_amd import api, synth
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(n, synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8" if int8 else "float")))
    b.plc_enable(api.PLC_CODEC)
    b.tune()
    if schedule:
        b.group_schedule = schedule
    T = 100
    base = np.stack([synth.make_pcm(700 + k, T).reshape(T, 160) for k in range(64)])
    frames = [torch.from_numpy(np.ascontiguousarray(np.tile(base[:, t], (n // 64 + 1, 1))[:n])).to(dev) for t in range(T)]
    d = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    rng = np.random.default_rng(7)
    vec_h = (rng.standard_normal((n * K, 20)) * 0.5).astype(np.float32)
    vec_h[:, 0] -= 3.0
    vec = torch.from_numpy(vec_h).to(dev)
    count = np.full(n, K, np.int32)
    s = torch.cuda.Stream()
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), streams=n, options="LPCNET_PLC_CODEC", flavour="int8" if int8 else "float",
                  vectors_per_stream_and_step=K, loss=0.05, feed="per-stream lpcnet_batch_plc_fec_add loop" if loop else "lpcnet_batch_plc_fec_feed_device")
    steps, warm = (-(-100 // K) + 40, 10) if loop else (-(-100 // K) + 130, 30)
    with torch.cuda.stream(s):
        if not loop:
            ms = []
            for t in range(30 + 60):
                d.copy_(frames[t % T])
                m = step_ms(torch, b, d, (rng.uniform(size=n) < 0.05).astype(np.uint8), s)
                if t >= 30:
                    ms.append(m)
            result["step_without_fec"] = stats(ms)
            print(json.dumps(result["step_without_fec"]), flush=True)
            b.plc_reset()
        rows = []
        for t in range(steps):
            lost = (rng.uniform(size=n) < 0.05).astype(np.uint8)
            d.copy_(frames[t % T])
            if loop:
                s.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    for k in range(K):
                        b.plc_fec_add(i, vec_h[i * K + k])
                t1 = time.perf_counter()
                b.plc_step_device(d.data_ptr(), lost, s.cuda_stream)
                s.synchronize()
                rows.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, 0))
            else:
                a, m, e = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                a.record(s)
                dropped = b.plc_fec_feed_device(vec.data_ptr(), count, hip_stream=s.cuda_stream)
                m.record(s)
                b.plc_step_device(d.data_ptr(), lost, s.cuda_stream)
                e.record(s)
                e.synchronize()
                rows.append((a.elapsed_time(m), a.elapsed_time(e), int(dropped.sum())))
        for name, (lo, hi) in fec_windows(K, steps, warm).items():
            if hi - lo >= 10:
                w = rows[lo:hi]
                result[name] = dict(first_step=lo, feed=stats([r[0] for r in w]), feed_and_step=stats([r[1] for r in w]), dropped_vectors_per_step=float(np.mean([r[2] for r in w])))
                print(name, json.dumps(result[name]), flush=True)
        if not loop:          # the host-pointer form with full rings: upload, enqueue, synchronise
            hs = []
            for t in range(25):
                s.synchronize()
                t0 = time.perf_counter()
                b.plc_fec_feed(vec_h, count)
                hs.append((time.perf_counter() - t0) * 1e3)
            result["host_pointer_feed_rings_full_host_clock"] = stats(hs[5:])
            print(json.dumps(result["host_pointer_feed_rings_full_host_clock"]), flush=True)
    b.sync()
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x not in ("--int8", "--fec-loop", "--ab", "--forms")]
    widths_list, pred_forms, losses = [], [], []
    for opt, dest, conv in (("--widths", widths_list, lambda x: tuple(int(v) for v in x.split(","))), ("--pred-form", pred_forms, int), ("--loss", losses, float)):
        while opt in args:
            i = args.index(opt)
            dest.append(conv(args[i + 1]))
            del args[i:i + 2]
    if "--forms" in sys.argv[1:]:
        measure_forms(args[0], [int(x) for x in args[1].split(",")] if len(args) > 1 else [8192], widths_list or [None], losses or [0.0], pinned=pred_forms)
        sys.exit(0)
    schedules = []
    while "--schedule" in args:
        i = args.index("--schedule")
        form, lanes = (int(x) for x in args[i + 1].split(","))
        schedules.append((form, lanes))
        del args[i:i + 2]
    if "--ab" in sys.argv[1:]:
        measure_ab(args[0], int(args[1]) if len(args) > 1 else 8192, schedules or [(1, 1), (0, 2), (0, 4), (1, 4)], int8="--int8" in sys.argv[1:])
        sys.exit(0)
    schedule = schedules[-1] if schedules else None
    if "--fec" in args:
        i = args.index("--fec")
        K = int(args[i + 1])
        del args[i:i + 2]
        measure_fec(args[0], int(args[1]) if len(args) > 1 else 8192, K, loop="--fec-loop" in sys.argv[1:], int8="--int8" in sys.argv[1:], schedule=schedule)
        sys.exit(0)
    measure(args[0], int(args[1]) if len(args) > 1 else 8192, int8="--int8" in sys.argv[1:], schedule=schedule, widths=widths_list[-1] if widths_list else None,
            pred_form=pred_forms[-1] if pred_forms else None)
