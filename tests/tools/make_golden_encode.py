#!/usr/bin/env python3
"""Generate the fixture of the encoder tests from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so: the generic-C float
build, `make -C oracle ref`), with the codebooks of synth.make_codebooks(5):

  tests/golden/golden_encode_v1.npz   seeds and the CRC of each synth.make_pcm stream; lpcnet_encode packets [streams][P][8];
                                      lpcnet_compute_features output [streams][4P][36] for the same PCM from fresh states

    python tests/tools/make_golden_encode.py

The generator prints what tests/test_gpu_encode.py asserts of the fixture: it is not degenerate (voiced and unvoiced packets, both
signs of vq_mid, most interp_id values, every corr_id, a non-zero modulation)."""
import ctypes as C
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lpcnet_amd import synth  # noqa: E402

SEEDS = (31, 32, 33, 34, 35, 36)
P = 64
CODEBOOK_SEED = 5
PATH = os.path.join(ROOT, "tests", "golden", "golden_encode_v1.npz")


def load_ref(path=os.path.join(ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so"), codebooks=None):
    L = C.CDLL(path)
    L.lpcnet_encoder_create.restype = C.c_void_p
    L.lpcnet_encoder_destroy.argtypes = [C.c_void_p]
    L.lpcnet_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lpcnet_compute_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lpcnet_compute_single_frame_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_set_codebooks.argtypes = [C.c_void_p] * 4
    cbs = [np.ascontiguousarray(c, np.float32) for c in (codebooks or synth.make_codebooks(CODEBOOK_SEED))]
    L.ref_set_codebooks(*[c.ctypes.data for c in cbs])
    return L


class RefEncoder:
    """one LPCNetEncState of the compiled reference, driven through its three entry points"""

    def __init__(self, L):
        self.L, self.st = L, L.lpcnet_encoder_create()

    def encode(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        out = np.zeros((pcm.size // 640, 8), np.uint8)
        for p in range(out.shape[0]):
            self.L.lpcnet_encode(self.st, pcm[p * 640:].ctypes.data, out[p].ctypes.data)
        return out

    def compute_features(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        out = np.zeros((pcm.size // 640, 4, 36), np.float32)
        for p in range(out.shape[0]):
            self.L.lpcnet_compute_features(self.st, pcm[p * 640:].ctypes.data, out[p].ctypes.data)
        return out.reshape(-1, 36)

    def analyze(self, pcm):
        """single-frame analysis: the STATE advances as in the engine; the returned features are stale after a four-frame call"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        out = np.zeros((pcm.size // 160, 36), np.float32)
        for t in range(out.shape[0]):
            self.L.lpcnet_compute_single_frame_features(self.st, pcm[t * 160:].ctypes.data, out[t].ctypes.data)
        return out

    def close(self):
        self.L.lpcnet_encoder_destroy(self.st)


def packet_fields(packets):
    """packets (..., 8) uint8 -> dict of the nine bit fields (7+6+3+2+10+10+10+13+3, MSB first)"""
    w = np.zeros(packets.shape[:-1], np.uint64)
    for k in range(8):
        w = (w << np.uint64(8)) | packets[..., k].astype(np.uint64)
    out, pos = {}, 64
    for name, nb in (("c0", 7), ("pitch", 6), ("mod", 3), ("corr", 2), ("e0", 10), ("e1", 10), ("e2", 10), ("mid", 13), ("interp", 3)):
        pos -= nb
        out[name] = ((w >> np.uint64(pos)) & np.uint64((1 << nb) - 1)).astype(np.int64)
    return out


def coverage(packets):
    f = packet_fields(packets)
    return dict(voiced=int((f["mod"] != 0).sum()), unvoiced=int((f["mod"] == 0).sum()), mid_pos=int((f["mid"] < 4096).sum()),
                mid_neg=int((f["mid"] >= 4096).sum()), interp_ids=sorted(set(f["interp"].reshape(-1).tolist())),
                corr_ids=sorted(set(f["corr"].reshape(-1).tolist())), modulated=int(((f["mod"] != 0) & (f["mod"] != 4)).sum()),
                pitch_ids=len(set(f["pitch"].reshape(-1).tolist())))


def is_rich(cov):
    return (cov["voiced"] > 0 and cov["unvoiced"] > 0 and cov["mid_pos"] > 0 and cov["mid_neg"] > 0 and len(cov["interp_ids"]) >= 6
            and cov["corr_ids"] == [0, 1, 2, 3] and cov["modulated"] > 0)


def generate():
    L = load_ref()
    packets, feats, crcs = [], [], []
    for seed in SEEDS:
        pcm = synth.make_pcm(seed, 4 * P)
        crcs.append(zlib.crc32(pcm.tobytes()))
        e = RefEncoder(L); packets.append(e.encode(pcm)); e.close()
        e = RefEncoder(L); feats.append(e.compute_features(pcm)); e.close()
    return dict(seeds=np.array(SEEDS, np.int32), pcm_crc32=np.array(crcs, np.uint32), codebook_seed=np.int32(CODEBOOK_SEED),
                packets=np.stack(packets), features=np.stack(feats))


def main():
    g = generate()
    np.savez_compressed(PATH, **g)
    cov = coverage(g["packets"])
    print("packets", g["packets"].shape, "features", g["features"].shape, cov, "rich" if is_rich(cov) else "DEGENERATE")


if __name__ == "__main__":
    main()
