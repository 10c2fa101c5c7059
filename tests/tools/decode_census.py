"""A constructive census of the codec's 8-byte packets (7+6+3+2+10+10+10+13+3 bits, MSB first), shared by tests/tools/make_golden_decode.py
and the decode tests: 8 chains of 64 packets, the VQ memory carrying along each chain from zero.  Built, not drawn, so that every branch of
decode_packet (src/lpcnet_dec.c:81-155) and of the double interpolation (src/common.c:37-65) is fed:

  * every (main_pitch, modulation) pair, 64 x 8, exactly once -- so every entry of the pitch table meets every modulation, the unvoiced
    remap of raw modulation 0 included;
  * every (vq_mid & 3, sign of vq_mid, interp_id) triple, 4 x 2 x 8, eight times each;
  * every c0_id four times; every corr_id among the voiced and among the unvoiced packets;
  * vq_mid 0, 4095, 4096 and 8191, and each of the three vq_end indices at 0 and at 1023.

The upper ten bits of vq_mid and the vq_end indices are otherwise random, from a fixed seed: the fixture stores results only, and the CRC-32
of the packets ties it to this generator."""
import zlib

import numpy as np

CHAINS, P = 8, 64
SEED = 20260
FIELDS = (("c0", 7), ("pitch", 6), ("mod", 3), ("corr", 2), ("e0", 10), ("e1", 10), ("e2", 10), ("mid", 13), ("interp", 3))


def pack(f):
    """dict of the nine fields (equal shapes) -> packets (..., 8) uint8"""
    w = np.zeros(np.shape(f["c0"]), np.uint64)
    for name, nb in FIELDS:
        v = np.asarray(f[name], np.uint64)
        assert (v < np.uint64(1 << nb)).all(), name
        w = (w << np.uint64(nb)) | v
    return np.stack([((w >> np.uint64(56 - 8 * k)) & np.uint64(255)).astype(np.uint8) for k in range(8)], axis=-1)


def fields(packets):
    """packets (..., 8) uint8 -> dict of the nine fields as they stand in the packet (modulation raw, 0..7)"""
    w = np.zeros(packets.shape[:-1], np.uint64)
    for k in range(8):
        w = (w << np.uint64(8)) | packets[..., k].astype(np.uint64)
    out, pos = {}, 64
    for name, nb in FIELDS:
        pos -= nb
        out[name] = ((w >> np.uint64(pos)) & np.uint64((1 << nb) - 1)).astype(np.int64)
    return out


def describe(packet):
    """one packet's fields, for a failure message"""
    return {k: int(v) for k, v in fields(np.asarray(packet, np.uint8).reshape(8)).items()}


def packets():
    """the census: (CHAINS, P, 8) uint8"""
    n = CHAINS * P
    r = np.random.default_rng(SEED)
    pair = r.permutation(n)                          # (main_pitch, modulation): each of the 512 pairs once
    triple = r.permutation(n) % 64                   # (vq_mid & 3, sign, interp_id): each of the 64 triples eight times
    f = dict(pitch=pair // 8, mod=pair % 8, c0=r.permutation(n) % 128, interp=triple % 8,
             e0=r.integers(0, 1024, n), e1=r.integers(0, 1024, n), e2=r.integers(0, 1024, n))
    low, sign = triple // 16, (triple // 8) % 2
    high = r.integers(0, 1024, n)
    for lo, sg, hi in ((0, 0, 0), (3, 0, 1023), (0, 1, 0), (3, 1, 1023)):        # vq_mid 0, 4095, 4096, 8191: the first packet of that kind
        high[np.flatnonzero((low == lo) & (sign == sg))[0]] = hi
    f["mid"] = sign * 4096 + high * 4 + low
    corr = np.zeros(n, np.int64)                     # the k-th unvoiced (voiced) packet takes corr_id k % 4
    for voiced in (False, True):
        at = np.flatnonzero((f["mod"] != 0) == voiced)
        corr[at] = np.arange(at.size) % 4
    f["corr"] = corr
    for k, name in enumerate(("e0", "e1", "e2")):    # both corners of every vq_end index, in packets of different chains
        f[name][P * k + 5] = 0
        f[name][P * (k + 3) + 9] = 1023
    return pack({k: v.reshape(CHAINS, P) for k, v in f.items()})


def differences(got, want, pk):
    """got, want (streams, packets, 4, columns) float32 compared on their bit patterns (tolerance 0); pk (streams, packets, 8).  Empty when they
    are equal; else the number of differing floats, which columns and sub-frames differ, and the first difference with stream, packet, sub-frame,
    column, both bit patterns and the packet's parsed fields -- enough to name the branch without running anything again"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and got.ndim == 4, (got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if not bad.any():
        return ""
    s, p, sub, col = (int(x) for x in np.argwhere(bad)[0])
    return ("%d floats differ; columns %s, sub-frames %s, streams %s; first: stream %d packet %d sub-frame %d column %d got %r (0x%08x) want %r (0x%08x) "
            "fields %s" % (int(bad.sum()), np.flatnonzero(bad.any(axis=(0, 1, 2))).tolist(), np.flatnonzero(bad.any(axis=(0, 1, 3))).tolist(),
                           np.flatnonzero(bad.any(axis=(1, 2, 3))).tolist(), s, p, sub, col, float(got[s, p, sub, col]),
                           int(got.view(np.uint32)[s, p, sub, col]), float(want[s, p, sub, col]), int(want.view(np.uint32)[s, p, sub, col]),
                           describe(pk[s, p])))


def crc32(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


PITCH_LOW, PITCH_HIGH = np.float32(.02) * (np.float32(33) - np.float32(100)), np.float32(.02) * (np.float32(255) - np.float32(100))


def coverage(pk, features=None):
    """what the packets reach; with the reference's features (..., 4, >= 19) also how the pitch feature meets its clamps at 33 and 255"""
    f = {k: v.reshape(-1) for k, v in fields(pk).items()}
    unv = f["mod"] == 0
    cov = dict(pitch_mod_pairs=len(set(zip(f["pitch"].tolist(), f["mod"].tolist()))),
               mid_triples=len(set(zip((f["mid"] & 3).tolist(), (f["mid"] >= 4096).tolist(), f["interp"].tolist()))),
               c0_ids=len(set(f["c0"].tolist())), corr_voiced=sorted(set(f["corr"][~unv].tolist())), corr_unvoiced=sorted(set(f["corr"][unv].tolist())),
               mid_corners=sorted(set(f["mid"].tolist()) & {0, 4095, 4096, 8191}),
               e_corners=[sorted(set(f[k].tolist()) & {0, 1023}) for k in ("e0", "e1", "e2")], c0_min=int(f["c0"].min()), c0_max=int(f["c0"].max()))
    if features is not None:
        pitch = np.asarray(features, np.float32)[..., 18].reshape(-1)
        cov.update(clamp_low=int((pitch == PITCH_LOW).sum()), clamp_high=int((pitch == PITCH_HIGH).sum()),
                   inside=int(((pitch > PITCH_LOW) & (pitch < PITCH_HIGH)).sum()))
    return cov


def is_complete(cov):
    """the coverage predicate of the fixture (cov from coverage() with the reference's features)"""
    return (cov["pitch_mod_pairs"] == 64 * 8 and cov["mid_triples"] == 64 and cov["c0_ids"] == 128
            and cov["corr_voiced"] == [0, 1, 2, 3] and cov["corr_unvoiced"] == [0, 1, 2, 3] and cov["mid_corners"] == [0, 4095, 4096, 8191]
            and cov["e_corners"] == [[0, 1023]] * 3 and cov["clamp_low"] > 0 and cov["clamp_high"] > 0 and cov["inside"] > 0)
