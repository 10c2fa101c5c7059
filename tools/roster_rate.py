#!/usr/bin/env python3
"""What an active prefix costs against a batch of exactly that size, and what a device-side stream copy costs.

    python tools/roster_rate.py OUT.json [capacity]       (profiles/roster_rate.json when run for the record)

A batch with a capacity of 8 192 float streams (default), PARITY arithmetic, advances ONE frame per step on the device-pointer API, enqueued and
waited for, as `bench.py --rt` does.  For active = 1/4, 1/2, 3/4 and all of the capacity (2 048 / 4 096 / 6 144 / 8 192) the step of the prefix
(lpcnet_batch_set_active) is timed against the yardstick: a batch created with exactly that many streams, in the same process, in alternating
blocks of steps -- yardstick, prefix, yardstick, ... -- so that both see the same clocks.  Per count: the median device time (HIP events on the
caller's stream) and host wall time of each side over all its blocks, the medians of the single blocks, the streams per workgroup each side
ran with, the ratio prefix / yardstick, and the spread between the yardstick's own block medians -- the margin a ratio has to beat.  The
yardstick is measured (lpcnet_batch_tune), as a server would run it; the prefix below the capacity takes the cost table's form and never the
twelve-wave form (include/lpcnet_batch.h), so a ratio above the margin names that difference.

Then lpcnet_batch_copy_streams on a batch of the same capacity with the packet-loss concealment enabled (every per-stream array exists: 17
rows of the copy table): 1, 64 and 1 024 pairs inside the one shard, HIP events around the enqueue-only call, median of 20 calls, with the
bytes a pair moves.  One process; the tool stops at the first failure.  Run it under a time limit:
    timeout -k 10 600 python tools/roster_rate.py profiles/roster_rate.json

    python tools/roster_rate.py --snapshot OUT.json [capacity] [--parent-lib PATH]       (profiles/snapshot_rate.json)

Stream snapshots (lpcnet_batch_snapshot_device / _restore_device) and the copy across shards, for m = 1, 64, 1 024 and the capacity, on batches with
the packet-loss concealment and the encoder enabled.  Every figure is host wall time from the call to the end of the work (the call, then a wait for
the stream or the batch), the median of a few repetitions after two that do not count:
  a  snapshot_device + restore_device of m streams of one batch on a caller's stream, with the HIP-event time between the two records beside it
     (gb_per_s: the records' bytes, once gathered and once scattered, over that time);
  b  lpcnet_batch_copy_streams of m pairs that all cross the two shards of a batch of 2 x capacity streams on one device, then lpcnet_batch_sync;
  c  the same call on the library of the parent commit (--parent-lib: built beside this one from a checkout of that commit), the two
     alternating call by call so that both see the same clocks.  Without --parent-lib the series is left out and the file says so.
The file also holds the record's bytes and the spread (max - min) / median of each series' repetitions, the margin a comparison has to beat.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

ROUNDS, BLOCK, WARM = 4, 12, 6


def steps(torch, b, d_feat, d_pcm, s, t0, count):
    """`count` one-frame steps from frame t0 -> (device ms, wall ms) per step"""
    dev, wall = [], []
    for t in range(t0, t0 + count):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        a.record(s)
        b.synthesize_device(d_feat[t % d_feat.shape[0]].data_ptr(), 36, d_pcm.data_ptr(), 1, s.cuda_stream)
        e.record(s)
        e.synchronize()
        wall.append((time.perf_counter() - w0) * 1e3)
        dev.append(a.elapsed_time(e))
    return dev, wall


def side(blocks):
    dev = [x for blk in blocks for x in blk[0]]
    wall = [x for blk in blocks for x in blk[1]]
    return dict(device_ms_median=float(np.median(dev)), wall_ms_median=float(np.median(wall)), device_ms_min=float(np.min(dev)), device_ms_max=float(np.max(dev)),
                block_device_ms_medians=[float(np.median(blk[0])) for blk in blocks], steps=len(dev))


class ParentLib:
    """the few calls series c needs, on another build of the library (ctypes, beside the one lpcnet_amd.api has loaded)"""

    def __init__(self, path, n, devices, blob, options):
        import ctypes as C
        self.C, self.L = C, C.CDLL(path)
        vp = C.c_void_p
        self.L.lpcnet_batch_create_sharded.restype = vp
        self.L.lpcnet_batch_create_sharded.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
        self.L.lpcnet_batch_load_model.argtypes = [vp, C.c_char_p, C.c_int]
        self.L.lpcnet_batch_plc_enable.argtypes = [vp, C.c_int]
        self.L.lpcnet_batch_encoder_enable.argtypes = [vp, C.c_int]
        self.L.lpcnet_batch_copy_streams.argtypes = [vp, vp, vp, C.c_int, vp]
        self.L.lpcnet_batch_sync.argtypes = [vp]
        self.L.lpcnet_batch_destroy.argtypes = [vp]
        self.L.lpcnet_batch_last_error.restype = C.c_char_p
        self.p = self.L.lpcnet_batch_create_sharded(n, (C.c_int * len(devices))(*devices), len(devices))
        self.chk(0 if self.p else -1)
        self.chk(self.L.lpcnet_batch_load_model(self.p, blob, len(blob)))
        self.chk(self.L.lpcnet_batch_plc_enable(self.p, options))
        self.chk(self.L.lpcnet_batch_encoder_enable(self.p, 1))

    def chk(self, rc):
        if rc:
            raise RuntimeError("parent library: %d %s" % (rc, self.L.lpcnet_batch_last_error().decode()))

    def copy_streams(self, src, dst):
        self.chk(self.L.lpcnet_batch_copy_streams(self.p, src.ctypes.data, dst.ctypes.data, int(src.size), None))

    def sync(self):
        self.chk(self.L.lpcnet_batch_sync(self.p))

    def close(self):
        self.L.lpcnet_batch_destroy(self.p)


def series(ms):
    return dict(wall_ms_median=float(np.median(ms)), wall_ms_min=float(np.min(ms)), wall_ms_max=float(np.max(ms)), calls=len(ms),
                spread=float((np.max(ms) - np.min(ms)) / np.median(ms)))


def snapshot_main(argv):
    import torch
    import plc_synth
    from lpcnet_amd import api, synth
    parent = None
    if "--parent-lib" in argv:
        i = argv.index("--parent-lib")
        parent = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    out_path = argv[0]
    cap = int(argv[1]) if len(argv) > 1 else 8192
    s = torch.cuda.Stream()
    blob = synth.blob_bytes(plc_synth.make_model_with_plc())
    opt = api.PLC_CODEC | api.PLC_DC_FILTER
    one = api.LPCNetBatch(cap, blob)
    one.plc_enable(opt)
    one.encoder_enable(1)
    lay = one.snapshot_layout()
    rb = lay["record_bytes"]
    two = api.LPCNetBatch(2 * cap, blob, devices=[0, 0])
    two.plc_enable(opt)
    two.encoder_enable(1)
    old = ParentLib(parent, 2 * cap, [0, 0], blob, opt) if parent else None
    rec = torch.zeros(cap * rb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    result = dict(capacity=cap, build=api.build_info(), device=torch.cuda.get_device_name(0), record_bytes=rb, sections=len(lay["sections"]),
                  parent_library=bool(parent), a_snapshot_restore=[], b_copy_across_shards=[], c_copy_across_shards_parent=[])
    if not parent:
        result["c_note"] = "no --parent-lib given: series c was not measured"

    def timed(call, wait):
        w0 = time.perf_counter()
        call()
        wait()
        return (time.perf_counter() - w0) * 1e3

    for m in sorted({1, min(64, cap), min(1024, cap), cap}):
        streams = np.arange(m, dtype=np.int32)
        src, dst = np.arange(m, dtype=np.int32), np.arange(cap, cap + m, dtype=np.int32)      # shard 0 -> shard 1
        reps = 9 if m <= 1024 else 5
        wa, da, wb, wc = [], [], [], []
        for r in range(reps + 2):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def both():
                a.record(s)
                meta = one.snapshot_device(streams, rec.data_ptr(), s.cuda_stream)
                one.restore_device(streams, rec.data_ptr(), meta, lay["sections"], s.cuda_stream)
                e.record(s)
            wa.append(timed(both, e.synchronize))
            da.append(a.elapsed_time(e))
            wb.append(timed(lambda: two.copy_streams(src, dst), two.sync))
            if old:
                wc.append(timed(lambda: old.copy_streams(src, dst), old.sync))
        ra = dict(series(wa[2:]), m=m, device_ms_median=float(np.median(da[2:])), gb_per_s=2e-6 * rb * m / float(np.median(da[2:])))
        rbb = dict(series(wb[2:]), m=m)
        print(json.dumps(dict(a=ra, b=rbb)), flush=True)
        result["a_snapshot_restore"].append(ra)
        result["b_copy_across_shards"].append(rbb)
        if old:
            rc = dict(series(wc[2:]), m=m, ratio_b_over_c=rbb["wall_ms_median"] / float(np.median(wc[2:])))
            print(json.dumps(dict(c=rc)), flush=True)
            result["c_copy_across_shards_parent"].append(rc)
    one.close(); two.close()
    if old:
        old.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    if "--snapshot" in sys.argv:
        return snapshot_main([x for x in sys.argv[1:] if x != "--snapshot"])
    import torch
    import plc_synth
    from lpcnet_amd import api, synth
    out_path = sys.argv[1]
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    blob = synth.blob_bytes(synth.make_model(flavour="float"))
    pool = np.stack([synth.make_features(5000 + i, 64) for i in range(64)])
    d_feat = torch.from_numpy(pool).to(dev)[torch.arange(cap, device=dev) % 64].permute(1, 0, 2).contiguous()      # [64 frames][cap][36]
    d_pcm = torch.zeros((cap, 160), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    big = api.LPCNetBatch(cap, blob)
    big.tune()
    result = dict(capacity=cap, build=api.build_info(), device=torch.cuda.get_device_name(0), rounds=ROUNDS, block=BLOCK, warmup=WARM,
                  capacity_streams_per_workgroup=big.streams_per_workgroup, capacity_twelve_waves=big.twelve_waves, prefix=[], copy=[])
    for active in (cap // 4, cap // 2, 3 * cap // 4, cap):
        yard = api.LPCNetBatch(active, blob)
        yard.tune()
        big.active = active
        form = dict(yardstick=(yard.streams_per_workgroup, yard.twelve_waves), prefix=(big.streams_per_workgroup, big.twelve_waves))
        steps(torch, yard, d_feat, d_pcm, s, 0, WARM)
        steps(torch, big, d_feat, d_pcm, s, 0, WARM)
        yb, pb = [], []
        for r in range(ROUNDS):
            yb.append(steps(torch, yard, d_feat, d_pcm, s, WARM + r * BLOCK, BLOCK))
            pb.append(steps(torch, big, d_feat, d_pcm, s, WARM + r * BLOCK, BLOCK))
        y, p = side(yb), side(pb)
        spread = (max(y["block_device_ms_medians"]) - min(y["block_device_ms_medians"])) / y["device_ms_median"]
        rec = dict(active=active, yardstick=y, prefix=p, ratio_device=p["device_ms_median"] / y["device_ms_median"], yardstick_block_spread=spread,
                   streams_per_workgroup_and_twelve_waves=form)
        print(json.dumps(rec), flush=True)
        result["prefix"].append(rec)
        yard.close()
    big.close()
    # the copy: every per-stream array of a batch with the PLC enabled
    pb = api.LPCNetBatch(cap, synth.blob_bytes(plc_synth.make_model_with_plc()))
    pb.plc_enable(api.PLC_CODEC | api.PLC_DC_FILTER)
    pb.encoder_enable(1)
    info = api.plc_model_info(synth.blob_bytes(plc_synth.make_model_with_plc()))
    pair_bytes = (3592 + 72 + 3924 + 72 + 4 * (1152 + 48 + 16) + 2 * 560 + 80 + 16 * (info["g1"] + info["g2"]) + 16 + 4 + 8000 + 320 + 320 + 144 + 144)
    for m in (1, 64, 1024):
        if 2 * m > cap:
            continue
        src, dst = np.arange(m), np.arange(cap - m, cap)
        ms = []
        for _ in range(22):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            pb.copy_streams(src, dst, s.cuda_stream)
            e.record(s)
            e.synchronize()
            ms.append(a.elapsed_time(e))
        ms = ms[2:]
        rec = dict(pairs=m, device_ms_median=float(np.median(ms)), device_ms_min=float(np.min(ms)), device_ms_max=float(np.max(ms)), calls=len(ms),
                   bytes_per_pair=pair_bytes, gb_per_s=2e-6 * pair_bytes * m / float(np.median(ms)))
        print(json.dumps(rec), flush=True)
        result["copy"].append(rec)
    pb.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
