#!/usr/bin/env python3
"""Generate the fixture of the decode tests from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so: the generic-C float build,
`make -C oracle ref`), with the codebooks of synth.make_codebooks(5) and the float test model:

  tests/golden/golden_decode_v1.npz
      packets_crc32      CRC-32 of the census of tests/tools/decode_census.py (8 chains x 64 packets; the packets themselves are regenerated)
      features           decode_packet's output per packet, columns 0..19 (the reference leaves 20..35 zero), [8][64][4][20]
      vq_mem             the VQ memory at the end of each chain, [8][18]
      pcm_crc32          CRC-32 of lpcnet_decode's 640 samples per packet, [8][64]
      pcm_chain, pcm     the full PCM of one chain, [PCM_PACKETS * 640]
      enc_features_crc32 decode_packet over the packets of golden_encode_v1.npz (a real encoder's, 6 x 64): CRC-32 of each stream's rows [256][20]
      enc_stream, enc_features   the full rows of one of those streams

    python tests/tools/make_golden_decode.py

Nothing is written unless the census passes its coverage predicate (decode_census.is_complete) and no PCM sample sits at +-32767 / -32768.
The archive is written with fixed time stamps: the same reference build gives the same bytes."""
import ctypes as C
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_census as dc  # noqa: E402
from lpcnet_amd import synth  # noqa: E402

CODEBOOK_SEED = 5
PCM_CHAIN = 3
PCM_PACKETS = dc.P           # packets of PCM_CHAIN whose samples are stored in full (shorten this, never the features, to stay under MAX_BYTES)
ENC_STREAM = 2
MAX_BYTES = 256 * 1024
PATH = os.path.join(ROOT, "tests", "golden", "golden_decode_v1.npz")
ENC_PATH = os.path.join(ROOT, "tests", "golden", "golden_encode_v1.npz")


def ref_features(lib, chain):
    """ref_decode_packet along one chain from a zero VQ memory: packets (P, 8) -> (features (P, 4, 36), final VQ memory (18,))"""
    feats, vq = np.zeros((chain.shape[0], 4, 36), np.float32), np.zeros(18, np.float32)
    for p in range(chain.shape[0]):
        lib.ref_decode_packet(feats[p].reshape(-1), vq, np.ascontiguousarray(chain[p]))
    return feats, vq


def ref_pcm(lib, blob, chain):
    """lpcnet_decode along one chain on a fresh decoder: (P, 640) int16"""
    dec = lib.lpcnet_decoder_create()
    buf = C.create_string_buffer(blob, len(blob))
    if lib.lpcnet_load_model(dec, buf, len(blob)) != 0:
        raise RuntimeError("reference lpcnet_load_model failed")
    pcm = np.zeros((chain.shape[0], 640), np.int16)
    for p in range(chain.shape[0]):
        lib.lpcnet_decode(dec, np.ascontiguousarray(chain[p]), pcm[p])
    lib.lpcnet_decoder_destroy(dec)
    return pcm


def generate():
    from oracle import ref
    lib = ref.RefLib("gf").lib
    lib.ref_set_codebooks(*[np.ascontiguousarray(c, np.float32) for c in synth.make_codebooks(CODEBOOK_SEED)])
    blob = synth.blob_bytes(synth.make_model(flavour="float"))
    pk = dc.packets()
    feats, mems, pcm = [], [], []
    for s in range(dc.CHAINS):
        f, m = ref_features(lib, pk[s])
        assert not f[:, :, 20:].any()
        feats.append(f[:, :, :20]); mems.append(m); pcm.append(ref_pcm(lib, blob, pk[s]))
    feats, pcm = np.stack(feats), np.stack(pcm)
    enc = np.load(ENC_PATH)["packets"]
    enc_rows = [np.ascontiguousarray(ref_features(lib, enc[s])[0][:, :, :20]).reshape(-1, 20) for s in range(enc.shape[0])]
    fixture = dict(packets_crc32=np.uint32(dc.crc32(pk)), codebook_seed=np.int32(CODEBOOK_SEED), features=feats, vq_mem=np.stack(mems),
                   pcm_crc32=np.array([[dc.crc32(pcm[s, p]) for p in range(dc.P)] for s in range(dc.CHAINS)], np.uint32),
                   pcm_chain=np.int32(PCM_CHAIN), pcm=np.ascontiguousarray(pcm[PCM_CHAIN, :PCM_PACKETS]).reshape(-1),
                   enc_features_crc32=np.array([dc.crc32(r) for r in enc_rows], np.uint32), enc_stream=np.int32(ENC_STREAM),
                   enc_features=enc_rows[ENC_STREAM])
    facts = dict(coverage=dc.coverage(pk, feats), c0_range=(float(feats[..., 3, 0].min()), float(feats[..., 3, 0].max())),
                 rail_share=float(((pcm == 32767) | (pcm <= -32767)).mean()), max_abs_sample=int(np.abs(pcm.astype(np.int32)).max()),
                 nonzero_share=float((pcm != 0).mean()), enc_coverage=dc.coverage(enc))
    return fixture, facts


def archive(fixture):
    """the bytes of an .npz with fixed member time stamps (np.savez_compressed stamps the members with the time of day)"""
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(fixture):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(fixture[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue(), compresslevel=9)
    return out.getvalue()


def main():
    fixture, facts = generate()
    for k, v in facts.items():
        print(k, v)
    if not dc.is_complete(facts["coverage"]):
        sys.exit("the census misses its coverage predicate: nothing written")
    if facts["rail_share"] != 0:
        sys.exit("PCM samples at the rails: nothing written")
    data = archive(fixture)
    if len(data) >= MAX_BYTES:
        sys.exit("%d bytes, the limit is %d: shorten PCM_PACKETS" % (len(data), MAX_BYTES))
    with open(PATH, "wb") as f:
        f.write(data)
    print("wrote", PATH, len(data), "bytes")


if __name__ == "__main__":
    main()
