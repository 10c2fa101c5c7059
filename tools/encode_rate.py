#!/usr/bin/env python3
"""Device time of the encoder beside the decoder's unpacking + synthesis, on the same batch in the same process.

    python tools/encode_rate.py OUT.json                       (profiles/encode_rate_<shapes>.json when run for the record)
    python tools/encode_rate.py --trace 8192x1                 (a few warm encode_device calls of one shape: the program to put under
                                                                `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/encode_rate.py --trace 8192x1`)
    python tools/encode_rate.py --kernels DIR OUT.json         (per-kernel average times of the encoder's five kernels from the
                                                                *kernel_trace.csv rocprofv3 wrote under DIR, the warm launches only)

For each shape -- 8192 streams x 1 packet (one 40-ms real-time step) and 2048 streams x 25 packets -- the median, minimum and maximum
device time (HIP events around the enqueue-only device-pointer calls, warmed up, at least 0.5 s of work per figure) of encode_device,
compute_features_device, analyze_device on the same 4 * packets frames, and decode_device.  One process; the shapes run one after the
other and the tool stops at the first failure.  Run it under a time limit:
    timeout -k 10 900 python tools/encode_rate.py profiles/encode_rate.json
"""
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((8192, 1), (2048, 25))
ENCODER_KERNELS = ("analysis_spectrum_kernel", "analysis_xcorr_kernel", "encode_pitch_kernel", "encode_vq_end_kernel", "encode_vq_mid_kernel")


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
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def setup(torch, n, P):
    from lpcnet_amd import api, synth
    api.set_codebooks(*synth.make_codebooks(5))
    b = api.LPCNetBatch(n, synth.blob_bytes(synth.make_model()))
    base = np.stack([synth.make_pcm(700 + s, 100) for s in range(64)])
    pcm = np.ascontiguousarray(np.tile(base, (n // 64, 1))[:, :P * 640])
    dev = torch.device("cuda:0")
    buf = dict(pcm=torch.from_numpy(pcm).to(dev), pk=torch.zeros((n, P, 8), dtype=torch.uint8, device=dev),
               feat=torch.zeros((n, 4 * P, 36), dtype=torch.float32, device=dev), out=torch.zeros((n, P * 640), dtype=torch.int16, device=dev))
    b.encoder_enable(P)
    return b, buf


def measure(out_path):
    import torch
    from lpcnet_amd import api
    result = dict(build=api.build_info(), device=torch.cuda.get_device_name(0), shapes=[])
    for n, P in SHAPES:
        b, d = setup(torch, n, P)
        b.tune()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            enc = timed(torch, lambda: b.encode_device(d["pcm"].data_ptr(), d["pk"].data_ptr(), P, s.cuda_stream), s)
            cf = timed(torch, lambda: b.compute_features_device(d["pcm"].data_ptr(), d["feat"].data_ptr(), 36, P, s.cuda_stream), s)
            an = timed(torch, lambda: b.analyze_device(d["pcm"].data_ptr(), False, d["feat"].data_ptr(), 36, 4 * P, s.cuda_stream), s)
            de = timed(torch, lambda: b.decode_device(d["pk"].data_ptr(), d["out"].data_ptr(), P, s.cuda_stream), s)
        b.sync()
        row = dict(streams=n, packets=P, encode_device=enc, compute_features_device=cf, analyze_device_4P_frames=an, decode_device=de,
                   vq_share_of_encode_by_difference=(enc["median_ms"] - cf["median_ms"]) / enc["median_ms"],
                   encode_share_of_decode=enc["median_ms"] / de["median_ms"], packets_per_second=n * P / (enc["median_ms"] * 1e-3))
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def trace(shape, calls=20):
    import torch
    n, P = (int(x) for x in shape.split("x"))
    b, d = setup(torch, n, P)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(calls):
            b.encode_device(d["pcm"].data_ptr(), d["pk"].data_ptr(), P, s.cuda_stream)
    b.sync()
    b.close()
    print("traced %d encode_device calls of %d streams x %d packets" % (calls, n, P))


def kernels(directory, out_path):
    """per kernel of the encoder: launches, average / min / max microseconds over the launches after the first two (warm-up)"""
    rows = {}
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        per = {}
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            key = next((k for k in ENCODER_KERNELS if k in name), None)
            if key:
                if key == "encode_pitch_kernel":
                    key += "<quant>" if "true" in name or "ILb1" in name else ("<features>" if "false" in name or "ILb0" in name else "")
                per.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        out = {}
        for k, v in per.items():
            dur = [d for _, d in sorted(v)][2:]
            if dur:
                out[k] = dict(launches=len(dur), avg_us=float(np.mean(dur)) / 1e3, min_us=min(dur) / 1e3, max_us=max(dur) / 1e3)
        if out:
            out["sum_of_averages_us"] = sum(v["avg_us"] for v in out.values())
            rows[os.path.relpath(f, directory)] = out
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(json.dumps(rows, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "--trace":
        trace(sys.argv[2])
    elif sys.argv[1] == "--kernels":
        kernels(sys.argv[2], sys.argv[3])
    else:
        measure(sys.argv[1])
