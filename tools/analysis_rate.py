#!/usr/bin/env python3
"""Device time of the feature analysis beside the synthesis step, on the same batch in the same process.

    python tools/analysis_rate.py OUT.json            (profiles/analysis_rate_<date>.json when run for the record)

For each shape -- 2048 streams x 25 frames and 8192 streams x 1 frame -- the median and minimum device time (HIP events around the
enqueue-only device-pointer calls, warmed up, at least 0.5 s of work per figure) of analyze_device and of synthesize_device.  One
process; the two shapes run one after the other and the tool stops at the first failure.  Run it under a time limit:
    timeout -k 10 600 python tools/analysis_rate.py profiles/analysis_rate.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, stream, min_seconds=0.5, min_reps=5):
    for _ in range(2):
        fn()
    stream.synchronize()
    ms, total = [], 0.0
    while total < min_seconds * 1e3 or len(ms) < min_reps:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b)); total += ms[-1]
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), reps=len(ms))


def main(out_path):
    import torch
    from lpcnet_amd import api, synth
    blob = synth.blob_bytes(synth.make_model())
    dev = torch.device("cuda:0")
    base = np.stack([synth.make_pcm(500 + s, 25) for s in range(64)])
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), shapes=[])
    for n, T in ((2048, 25), (8192, 1)):
        b = api.LPCNetBatch(n, blob)
        b.tune()
        pcm = np.ascontiguousarray(np.tile(base, (n // 64, 1))[:, :T * 160])
        d_pcm = torch.from_numpy(pcm).to(dev)
        d_feat = torch.zeros((n, T, 36), dtype=torch.float32, device=dev)
        d_out = torch.zeros((n, T * 160), dtype=torch.int16, device=dev)
        s = torch.cuda.Stream()
        b.analysis_enable(T)
        with torch.cuda.stream(s):
            an = timed(torch, lambda: b.analyze_device(d_pcm.data_ptr(), False, d_feat.data_ptr(), 36, T, s.cuda_stream), s)
            sy = timed(torch, lambda: b.synthesize_device(d_feat.data_ptr(), 36, d_out.data_ptr(), T, s.cuda_stream), s)
        b.sync()
        row = dict(streams=n, frames=T, analyze_device=an, synthesize_device=sy, analysis_share_of_synthesis=an["median_ms"] / sy["median_ms"],
                   streams_per_workgroup=b.streams_per_workgroup)
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
