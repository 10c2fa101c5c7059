#!/usr/bin/env python3
"""Generate the fixture of the encoder's tie rules from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so: the generic-C float build,
`make -C oracle ref`), under the codebooks of tests/tools/encode_ties.py, whose entries tie on purpose:

  tests/golden/golden_encode_ties_v1.npz   seeds and the CRC of each synth.make_pcm stream, the codebook seed; lpcnet_encode packets
                                           [streams][P][8] and the VQ memory [streams][18] after the last packet; two recorded counts:
                                           packets won by a zero row of ceps_codebook_diff4, and packets in which double_interp_search
                                           passed over the forbidden id 7 although it was the nearest

    python tests/tools/make_golden_encode_ties.py

It prints the census of encode_ties.census and refuses to write unless every condition of encode_ties.conditions holds: the reference decides
every tie by the lower index, and every kind of pair separates a winner from a twin at least ten times."""
import ctypes as C
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import encode_ties  # noqa: E402
import make_golden_encode as mge  # noqa: E402
from lpcnet_amd import synth  # noqa: E402

SEEDS = (41, 42, 43, 44, 45, 46)
P = 64
PATH = os.path.join(ROOT, "tests", "golden", "golden_encode_ties_v1.npz")


def ref_encode(L, pcm):
    """one fresh LPCNetEncState of the compiled reference over pcm -> (packets [P][8], the VQ memory [18] after the last one).  The memory is what the
    reference's decode_packet leaves after that packet: the quantised frame 3, by the expression the encoder keeps it with (src/lpcnet_enc.c:230,
    :719; src/lpcnet_dec.c:133, :154) -- the harness reaches the decoder's copy without a struct offset"""
    L.ref_decode_packet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    e = mge.RefEncoder(L)
    packets = e.encode(pcm)
    e.close()
    mem, feats = np.zeros(18, np.float32), np.zeros((4, 36), np.float32)
    L.ref_decode_packet(feats.ctypes.data, mem.ctypes.data, packets[-1].ctypes.data)
    return packets, mem


def generate():
    ties = encode_ties.make(encode_ties.SEED)
    L = mge.load_ref(codebooks=ties["cbs"])
    try:
        packets, mems, crcs, id7 = [], [], [], 0
        for seed in SEEDS:
            pcm = synth.make_pcm(seed, 4 * P)
            crcs.append(zlib.crc32(pcm.tobytes()))
            pk, mem = ref_encode(L, pcm)
            packets.append(pk); mems.append(mem)
            e = mge.RefEncoder(L); feats = e.compute_features(pcm); e.close()
            interp, n7 = encode_ties.interp_census(pk, feats, ties["cbs"])
            assert np.array_equal(interp, mge.packet_fields(pk)["interp"]), seed      # (the recomputation is the reference's search)
            id7 += n7
    finally:
        mge.load_ref()                           # (the library is shared within a process: back to the codebooks of make_codebooks(5))
    return dict(seeds=np.array(SEEDS, np.int32), pcm_crc32=np.array(crcs, np.uint32), codebook_seed=np.int32(encode_ties.SEED),
                packets=np.stack(packets), vq_mem=np.stack(mems), forbidden_id7=np.int32(id7),
                zero_row_winners=np.int32(encode_ties.census(np.stack(packets), ties)["mid_zero_row"]))


def main():
    g = generate()
    c = encode_ties.census(g["packets"], encode_ties.make(int(g["codebook_seed"])))
    print(c)
    print("recorded, not required: zero-row winners", int(g["zero_row_winners"]), "forbidden id 7 passed over", int(g["forbidden_id7"]))
    bad = encode_ties.conditions(c)
    if bad:
        sys.exit("NOT WRITTEN: " + "; ".join(bad))
    np.savez_compressed(PATH, **g)
    print("wrote", PATH, "packets", g["packets"].shape, "vq_mem", g["vq_mem"].shape)


if __name__ == "__main__":
    main()
