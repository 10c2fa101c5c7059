"""The shapes of tests/test_gpu_encode_large.py and the launches they must reach, as api.encode_plan (the engine's own rule, no device) reports
them.  tests/test_encode_plan_host.py asserts the table without a GPU; the GPU tests assert it again before they run."""
import functools
import zlib

import numpy as np

import make_golden_encode as mge
from lpcnet_amd import api, synth

N = 2048                         # capacity of the big batch: chunks of 65536 / 2048 = 32 frames = 8 packets
SMALL = 256                      # the reference batches: one chunk, one item per wavefront -- the form the fixtures pin

# name -> (active streams, packets, the launches of one encode call)
ENCODE = {
    "chunked": (2048, 9, [dict(packets=8, items=16384, ipw_end=4, ipw_mid=2, wg_end=512, last_end=32, wg_mid=1024, last_mid=16),
                          dict(packets=1, items=2048, ipw_end=1, ipw_mid=1, wg_end=256, last_end=8, wg_mid=256, last_mid=8)]),
    "ragged3": (2047, 8, [dict(packets=8, items=16376, ipw_end=3, ipw_mid=2, wg_end=683, last_end=8, wg_mid=1024, last_mid=8)]),
    "ragged2": (1031, 8, [dict(packets=8, items=8248, ipw_end=2, ipw_mid=2, wg_end=516, last_end=8, wg_mid=516, last_mid=8)]),
}
FEATURES = (2048, 9, [8, 1])     # compute_features: active, packets, packets per chunk
ANALYZE = (2048, 33, [32, 1])    # analyze: active, frames, frames per chunk


def check_plans():
    for name, (active, P, want) in ENCODE.items():
        assert api.encode_plan(N, active, P) == want, (name, api.encode_plan(N, active, P))
    active, P, chunks = FEATURES
    assert [r["packets"] for r in api.encode_plan(N, active, P)] == chunks
    active, T, chunks = ANALYZE
    assert api.encode_plan(N, active, T, analysis=True) == [dict(frames=c, items=active * c) for c in chunks]
    # the reference batches run the pinned form
    for P in (1, 8, 9, 10):
        assert all(r["ipw_end"] == 1 and r["ipw_mid"] == 1 for r in api.encode_plan(SMALL, SMALL, P)) and len(api.encode_plan(SMALL, SMALL, P)) == 1
    assert len(api.encode_plan(SMALL, SMALL, 33, analysis=True)) == 1


# where the six streams of tests/golden/golden_encode_v1.npz sit in the big batch: stream 0, the last active stream of every case (1030, 2046,
# 2047: in the ragged cases it alone fills the last workgroup of both VQ kernels), 2046 inside the last workgroup of the full case, two in between
GOLD_AT = (0, 517, 1030, 1500, 2046, 2047)
BASE_SEED, BASES, SHIFT = 41000, 256, 53


PACKETS = 10                     # the longest run of a case: a call of 9 packets and one of 1


@functools.lru_cache(maxsize=None)
def big_pcm():
    """(N, PACKETS * 640) int16, read-only, every row distinct: stream s is make_pcm stream s % 256 rotated by 53 (s // 256) samples, the
    fixture's streams unshifted at GOLD_AT.  Built once per process (make_pcm is the expensive part on the host)"""
    ns = PACKETS * 640
    g = np.load(mge.PATH)
    gold = np.stack([synth.make_pcm(int(s), 4 * g["packets"].shape[1]) for s in g["seeds"]])
    assert [zlib.crc32(p.tobytes()) for p in gold] == g["pcm_crc32"].tolist()
    base = np.stack([synth.make_pcm(BASE_SEED + k, 4 * PACKETS) for k in range(BASES)])
    pcm = np.concatenate([np.roll(base, SHIFT * c, axis=1) for c in range(N // BASES)])
    for k, s in enumerate(GOLD_AT):
        pcm[s] = gold[k, :ns]
    assert pcm.shape == (N, ns) and len({row.tobytes() for row in pcm}) == N      # a mis-indexed item reads another stream's data
    pcm = np.ascontiguousarray(pcm)
    pcm.setflags(write=False)
    return pcm
