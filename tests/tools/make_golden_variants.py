#!/usr/bin/env python3
"""Generate tests/golden/golden_variants_v1.npz from the reference's variant builds (oracle/_ref/liblpcnet_ref_{gg,ge,gx}.so: the generic-C float
build with LPC_GAMMA 0.9, with END2END, and with END2END and LPC_GAMMA 0.95; `make -C oracle ref`), driven through ctypes.  Inputs are seeded, so
the fixture holds results only:

  pcm_<fl>_<seed>, gru_a_<fl>_<seed>, gru_b_<fl>_<seed>   lpcnet_synthesize over the first T frames of synth.make_features(seed, 60), fl in gg / ge / gx:
               the PCM and the final GRU states.  No sample of any of these streams is at +-32767: the tool refuses to write a fixture otherwise
               (END2END with LPC_GAMMA 1 is an unstable filter on the synthetic model; SEEDS are those that stay inside the range for T frames)
  rail_share   [3 flavours][3 seeds] share of the live samples at +-32767 (all zero, see above), max_abs the largest |sample|
  plc_crc_<fl> [2 option sets][5][4], fl in gg / gx: lpcnet_plc_update / lpcnet_plc_conceal over PLC_T frames of plc_model.stream_pcm(s) with the
               losses of plc_lost(), LPCNET_PLC_CAUSAL and LPCNET_PLC_CODEC: CRC-32 over the per-frame CRC-32 values of each block of PLC_BLOCK frames
  plc_full_<fl> [2][PLC_T][160] the output of stream PLC_FULL_STREAM
  packet_pcm_gg [12][640] lpcnet_decode of golden_v1.npz's packets with the codebooks of synth.make_codebooks(5)
  blob_crc, plc_blob_crc, feat_crc [3], plc_in_crc, plc_lost_crc, packets_crc: CRC-32 of the two model blobs and of every input

    python tests/tools/make_golden_variants.py [OUT.npz]
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import synth  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "golden_variants_v1.npz")
FLAVOURS = ("gg", "ge", "gx")
SEEDS = (8200, 8202, 8203)         # END2END with LPC_GAMMA 1 stays below full scale for T frames on these (checked with the oracle, asserted below)
T = 12
PLC_FLAVOURS = ("gg", "gx")
PLC_OPTIONS = (0, 2)               # LPCNET_PLC_CAUSAL, LPCNET_PLC_CODEC
PLC_STREAMS, PLC_T, PLC_BLOCK, PLC_FULL_STREAM = 5, 24, 6, 2
CODEBOOK_SEED = 5


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def features(seed):
    return np.ascontiguousarray(synth.make_features(seed, 60)[:T])


def plc_pcm():
    return np.stack([pm.stream_pcm(s, PLC_T) for s in range(PLC_STREAMS)])


def plc_lost():
    """[5][24] uint8: per stream one burst of five lost frames and two isolated losses, at different frames for every stream"""
    L = np.zeros((PLC_STREAMS, PLC_T), np.uint8)
    for s in range(PLC_STREAMS):
        L[s, 1 + s] = 1
        L[s, 8 + s:13 + s] = 1
        L[s, 19 + s % 4] = 1
    return L


def block_crc(out):
    """out [n][PLC_T][160] int16 -> [n][PLC_T / PLC_BLOCK] uint32, as plc_model.block_crc with blocks of PLC_BLOCK frames"""
    n, t = out.shape[0], out.shape[1]
    assert t % PLC_BLOCK == 0
    fr = np.array([[zlib.crc32(np.ascontiguousarray(f).tobytes()) for f in s] for s in out], "<u4").reshape(n, t // PLC_BLOCK, PLC_BLOCK)
    return np.array([[zlib.crc32(np.ascontiguousarray(b).tobytes()) for b in s] for s in fr], np.uint32)


def rail_share(pcm):
    live = pcm[320:]
    return float((np.abs(live.astype(np.int32)) >= 32767).mean())


def generate():
    from make_golden_plc import load_ref, run_stream
    from oracle import ref
    out = {}
    blob = synth.blob_bytes(synth.make_model(flavour="float"))
    blob_plc = synth.blob_bytes(plc_synth.make_model_with_plc())
    out["blob_crc"], out["plc_blob_crc"] = crc(np.frombuffer(blob, np.uint8)), crc(np.frombuffer(blob_plc, np.uint8))
    out["seeds"], out["n_frames"] = np.array(SEEDS), np.array(T)
    out["feat_crc"] = np.array([crc(features(s)) for s in SEEDS], np.uint32)
    share, peak = np.zeros((len(FLAVOURS), len(SEEDS))), np.zeros((len(FLAVOURS), len(SEEDS)), np.int32)
    for i, fl in enumerate(FLAVOURS):
        lib = ref.RefLib(fl)
        for j, seed in enumerate(SEEDS):
            st = lib.new_state(blob)
            pcm = st.synthesize(features(seed))
            share[i, j], peak[i, j] = rail_share(pcm), np.abs(pcm.astype(np.int32)).max()
            assert peak[i, j] < 32767, "flavour %s seed %d: %.1f %% of the live samples are on the rails" % (fl, seed, 100 * share[i, j])
            assert np.any(pcm[320:] != 0) and not np.any(pcm[:320])
            out[f"pcm_{fl}_{seed}"] = pcm
            _, _, out[f"gru_a_{fl}_{seed}"], out[f"gru_b_{fl}_{seed}"] = st.nnet_state()
    out["rail_share"], out["max_abs"] = share, peak
    # PLC
    pcm_in, lost = plc_pcm(), plc_lost()
    out["plc_in_crc"], out["plc_lost_crc"] = crc(pcm_in), crc(lost)
    for fl in PLC_FLAVOURS:
        L = load_ref(os.path.join(ref.REF_DIR, f"liblpcnet_ref_{fl}.so"))
        res = [np.stack([run_stream(L, blob_plc, opt, pcm_in[s], lost[s])[0] for s in range(PLC_STREAMS)]) for opt in PLC_OPTIONS]
        for r in res:              # (the input has full-scale passages, which received frames pass on: the concealed frames are what must stay inside)
            assert np.abs(r[lost != 0].astype(np.int32)).max() < 32767 and (r[lost != 0] != 0).mean() > 0.5
        out[f"plc_crc_{fl}"] = np.stack([block_crc(r) for r in res])
        out[f"plc_full_{fl}"] = np.stack([r[PLC_FULL_STREAM] for r in res])
    # codec
    packets = np.load(os.path.join(ROOT, "tests", "golden", "golden_v1.npz"))["packets"]
    out["packets_crc"] = crc(packets)
    gg = ref.RefLib("gg").lib
    gg.ref_set_codebooks(*synth.make_codebooks(CODEBOOK_SEED))
    dec = gg.lpcnet_decoder_create()
    buf = C.create_string_buffer(blob, len(blob))
    assert gg.lpcnet_load_model(dec, buf, len(blob)) == 0
    pcm = np.zeros((len(packets), 640), np.int16)
    for i, pk in enumerate(packets):
        gg.lpcnet_decode(dec, np.ascontiguousarray(pk), pcm[i])
    gg.lpcnet_decoder_destroy(dec)
    assert np.abs(pcm.astype(np.int32)).max() < 32767
    out["packet_pcm_gg"] = pcm
    return out


def main():
    out = generate()
    again = generate()
    assert out.keys() == again.keys() and all(np.array_equal(out[k], again[k]) for k in out), "the reference's output is not reproducible"
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for i, fl in enumerate(FLAVOURS):
        print(fl, "rail share", out["rail_share"][i].tolist(), "largest |sample|", out["max_abs"][i].tolist())


if __name__ == "__main__":
    main()
