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


def measure(out_path, n, int8=False):
    import torch
    import plc_synth
    from lpcnet_amd import api, synth
    dev = torch.device("cuda:0")
    b = api.LPCNetBatch(n, synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8" if int8 else "float")))
    b.plc_enable(api.PLC_CAUSAL)
    assert b.plc_flavour() == int(int8)
    b.tune()
    T = 100
    base = np.stack([synth.make_pcm(700 + k, T).reshape(T, 160) for k in range(64)])
    frames = [torch.from_numpy(np.ascontiguousarray(np.tile(base[:, t], (n // 64 + 1, 1))[:n])).to(dev) for t in range(T)]
    d = torch.zeros((n, 160), dtype=torch.int16, device=dev)
    feat = torch.zeros((n, 1, 36), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    rng = np.random.default_rng(7)
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), streams=n, options="LPCNET_PLC_CAUSAL", flavour="int8" if int8 else "float",
                  streams_per_workgroup=b.L.lpcnet_batch_get_streams_per_workgroup(b.p), random_loss=[], burst=None)
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


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--int8"]
    measure(args[0], int(args[1]) if len(args) > 1 else 8192, int8="--int8" in sys.argv[1:])
