#!/usr/bin/env python3
"""Generate tests/golden/golden_plc_fec_v1.npz from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so, the generic-C float build, and
liblpcnet_ref_gi.so, the generic-C int8 build; `make -C oracle ref`): the script of tests/tools/plc_fec_script.py driven through
lpcnet_plc_fec_clear / lpcnet_plc_fec_add / lpcnet_plc_update / lpcnet_plc_conceal, one LPCNetPLCState per stream.  The fixture holds the
script as it was run (inputs, flags, FEC vectors) and the output PCM:

  pcm_in [5][60][160], lost / count / skip / clear [60][5], vec [sum(count)][20]
  pcm_out [3][5][60][160] for cases = (options, int8): (LPCNET_PLC_CODEC, 0), (LPCNET_PLC_CAUSAL | LPCNET_PLC_DC_FILTER, 0), (LPCNET_PLC_CODEC, 1)
  blob_crc [2]: CRC-32 of the float and of the int8 model blob

    python tests/tools/make_golden_plc_fec.py [OUT.npz]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plc_model as pm  # noqa: E402
import plc_fec_script as fs  # noqa: E402
import plc_synth  # noqa: E402
from make_golden_plc import load_ref  # noqa: E402
from lpcnet_amd import synth  # noqa: E402

CASES = ((2, 0), (4, 0), (2, 1))


def run_stream(L, blob, options, sc, s):
    st = L.lpcnet_plc_create(options)
    assert L.lpcnet_plc_load_model(st, blob, len(blob)) == 0
    out = np.zeros((fs.T, 160), np.int16)
    fed = 0
    for t in range(fs.T):
        row = fs.step_rows(sc, t)[0] + int(sc["count"][t, :s].sum())
        if sc["clear"][t, s]:
            L.lpcnet_plc_fec_clear(st)
        for _ in range(int(sc["skip"][t, s])):
            L.lpcnet_plc_fec_add(st, None)
        for k in range(int(sc["count"][t, s])):
            v = np.ascontiguousarray(sc["vec"][row + k])
            L.lpcnet_plc_fec_add(st, v.ctypes.data)
            fed += 1
        frame = np.ascontiguousarray(sc["pcm"][s, t]).copy()
        if sc["lost"][t, s]:
            frame[:] = 0
            L.lpcnet_plc_conceal(st, frame.ctypes.data)
        else:
            L.lpcnet_plc_update(st, frame.ctypes.data)
        out[t] = frame
    L.lpcnet_plc_destroy(st)
    return out, fed


def main():
    sc = fs.script()
    libs = [load_ref(os.path.join(pm.ROOT, "oracle", "_ref", "liblpcnet_ref_g%s.so" % f)) for f in "fi"]
    blobs = [synth.blob_bytes(plc_synth.make_model_with_plc()), synth.blob_bytes(plc_synth.make_model_with_plc(flavour="int8"))]
    outs = []
    for options, i8 in CASES:
        res = [run_stream(libs[i8], blobs[i8], options, sc, s) for s in range(fs.N)]
        out = np.stack([r[0] for r in res])
        lost = sc["lost"].T.astype(bool)
        print("options", options, "int8" if i8 else "float", "vectors fed", sum(r[1] for r in res), "lost frames", int(lost.sum()),
              "nonzero concealed samples", int((out[lost] != 0).sum()), "of", int(lost.sum()) * 160, flush=True)
        outs.append(out)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_plc_fec_v1.npz")
    np.savez_compressed(out_path, pcm_in=sc["pcm"], lost=sc["lost"], count=sc["count"], skip=sc["skip"], clear=sc["clear"], vec=sc["vec"],
                        pcm_out=np.stack(outs), cases=np.array(CASES, np.int32), blob_crc=np.array([zlib.crc32(b) for b in blobs], np.uint32))


if __name__ == "__main__":
    main()
