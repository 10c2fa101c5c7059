#!/usr/bin/env python3
"""Bring-up check and A/B of the twelve-wave form of the two-group sample kernel on a GPU box: PCM against the CPU oracle for 8 / 16 / 13 / 5 streams
plus a continued second call, then the sample-kernel rate of both forms, alternating.   python tests/tools/x3_check.py [frames] [timing streams] [rounds]"""
import sys, os, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lpcnet_amd import synth, api
from oracle import orc


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    nt = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    blob = synth.blob_bytes(synth.make_model())
    om = orc.OracleModel(blob)
    bad = 0
    for n in (() if os.environ.get('X3_SKIP_PARITY') else (8, 16, 13, 5)):
        feats = np.stack([synth.make_features(1000 + s, T) for s in range(n)])
        feats2 = np.stack([synth.make_features(2000 + s, 3) for s in range(n)])
        ref, ref2 = [], []
        for s in range(n):
            st = om.new_state(); ref.append(st.synthesize(feats[s])); ref2.append(st.synthesize(feats2[s]))
        b = api.LPCNetBatch(n, blob)
        b.streams_per_workgroup = 8
        b.twelve_waves = 1
        t0 = time.time()
        pcm = b.synthesize(feats)
        d = np.nonzero(pcm != np.stack(ref))
        print("n=%d twelve_waves=%d: mismatching samples %d of %d, first %s (%.2fs)" % (n, b.twelve_waves, d[0].size, pcm.size,
              (d[0][:4].tolist(), d[1][:4].tolist()) if d[0].size else None, time.time() - t0), flush=True)
        d2 = int((b.synthesize(feats2) != np.stack(ref2)).sum())
        print("      continued over a second call: mismatches %d" % d2, flush=True)
        bad += d[0].size + d2
        b.close()
    if bad:
        print("X3 PARITY FAILED")
        return 1
    Tt = 10
    feats = np.stack([synth.make_features(1000 + (s % 64), Tt) for s in range(nt)])
    bs = []
    for tw in (0, 1):
        b = api.LPCNetBatch(nt, blob)
        b.streams_per_workgroup = 8
        b.twelve_waves = tw
        b.enable_timing(True)
        b.synthesize(feats)
        bs.append(b)
    out = [bs[0].synthesize(feats), bs[1].synthesize(feats)]
    print("both forms identical on %d streams: %s" % (nt, bool(np.array_equal(out[0], out[1]))), flush=True)
    for r in range(rounds):
        for tw in (0, 1):
            bs[tw].synthesize(feats)
            ms = bs[tw].last_timing()[0]
            print("timing n=%d twelve_waves=%d round %d: sample kernel %.2f ms -> %.1f M samples/s" % (nt, tw, r, ms, nt * Tt * 160 / ms / 1e3), flush=True)
    return 0 if np.array_equal(out[0], out[1]) else 1


if __name__ == "__main__":
    sys.exit(main())
