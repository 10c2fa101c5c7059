#!/usr/bin/env python3
"""Generate tests/golden/golden_plc_i8_v1.npz from the compiled reference's generic-C int8 build (oracle/_ref/liblpcnet_ref_gi.so, DOT_PROD,
`make -C oracle ref`), driven through ctypes exactly as make_golden_plc.py drives the float build.  The model is
plc_synth.make_model_with_plc(flavour="int8"); the inputs are the seeded ones of tests/tools/plc_model.py, so the fixture holds results only:

  pcm_crc      [4 option sets][64][30], pcm_full [4][40][160], fec_crc [64][30], fec_full [30][160]: as in golden_plc_v1.npz
  pred         [40][20] compute_plc_pred on plc_model.pred_inputs(), chained from the reference's exported layer functions at 128 / 16 / 16
  blob_crc, in_crc: CRC-32 of the model blob and of the input PCM

The NumPy restatement (plc_i8_model.PlcNetNumpyI8) must equal `pred` bit for bit: it is what the tests use at 128 / 256 / 256, where the
reference's stack arrays (sized by the stand-in nnet_data.h) are too small.  The number of non-zero concealed samples is printed per option set:
a set that conceals to silence would prove nothing.

    python tests/tools/make_golden_plc_i8.py [OUT.npz]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plc_model as pm  # noqa: E402
import plc_i8_model as pq  # noqa: E402
import plc_synth  # noqa: E402
from make_golden_plc import load_ref, ref_pred_trace, run_stream  # noqa: E402
from lpcnet_amd import synth  # noqa: E402


def main():
    L = load_ref(os.path.join(pm.ROOT, "oracle", "_ref", "liblpcnet_ref_gi.so"))
    blob = synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))
    pcm = np.stack([pm.stream_pcm(s) for s in range(pm.N_STREAMS)])
    lost = pm.loss_patterns()
    pcm_crc, pcm_full = [], []
    for opt in pm.OPTION_SETS:
        out = np.stack([run_stream(L, blob, opt, pcm[s], lost[s])[0] for s in range(pm.N_STREAMS)])
        pcm_crc.append(pm.block_crc(out)); pcm_full.append(out[pm.FULL_STREAM, pm.FULL_FRAMES[0]:pm.FULL_FRAMES[1]])
        nz = int((out[lost.astype(bool)] != 0).sum())
        print("options", opt, "lost frames", int(lost.sum()), "nonzero concealed samples", nz, "of", int(lost.sum()) * 160, flush=True)
        assert nz > 0.5 * int(lost.sum()) * 160, "the concealment is (nearly) silence: pick another seed"
    ops, vec = pm.fec_schedule()
    flost = pm.fec_loss_patterns()
    res = [run_stream(L, blob, 0, pcm[s], flost[s], ops[:, s], vec[:, s]) for s in range(pm.N_STREAMS)]
    fout = np.stack([r[0] for r in res])
    print("FEC vectors used", int(np.stack([r[1] for r in res])[..., 4].sum()))
    xs = pm.pred_inputs()
    pred = ref_pred_trace(L, blob, xs)
    net = pq.PlcNetNumpyI8(blob)
    mine = np.stack([net.pred(x) for x in xs])
    same = np.array_equal(mine.view(np.uint32), pred.view(np.uint32))
    print("NumPy restatement equals the reference:", same)
    assert same
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_plc_i8_v1.npz")
    np.savez_compressed(out_path, pcm_crc=np.stack(pcm_crc), pcm_full=np.stack(pcm_full), fec_crc=pm.block_crc(fout),
                        fec_full=fout[pm.FEC_FULL_STREAM, pm.FEC_FULL_FRAMES[0]:pm.FEC_FULL_FRAMES[1]], pred=pred,
                        blob_crc=np.uint32(zlib.crc32(blob)), in_crc=np.uint32(zlib.crc32(pcm.tobytes())), options=np.array(pm.OPTION_SETS, np.int32))


if __name__ == "__main__":
    main()
