#!/usr/bin/env python3
"""Generate tests/golden/golden_plc_v1.npz from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so, the generic-C float build,
`make -C oracle ref`), driven through ctypes.  Inputs are seeded (tests/tools/plc_model.py); the fixture holds results:

  pcm_crc      [4 option sets][64][30] per block of 10 output frames of lpcnet_plc_update / lpcnet_plc_conceal, stream by stream: CRC-32 over
               the block's ten per-frame CRC-32 values (plc_model.block_crc)
  pcm_full     [4][40][160] the output samples of stream plc_model.FULL_STREAM, frames FULL_FRAMES (what a failing comparison is looked at with)
  fec_crc      [64][30] the same for the run with FEC schedules (LPCNET_PLC_CAUSAL), fec_full [30][160] of FEC_FULL_STREAM, frames FEC_FULL_FRAMES
  summary      [2][300][64][10] int16 for LPCNET_PLC_CAUSAL and LPCNET_PLC_CODEC (the DC filter does not change the control flow: checked here),
               fec_summary [300][64][10]: the control flow per stream and frame (PlcControl of plc_model.py)
  burg         [8][36] burg_cepstral_analysis of plc_model.burg_frames()
  pred         [40][20] compute_plc_pred on plc_model.pred_inputs(), chained from the reference's exported layer functions
               (_lpcnet_compute_dense, compute_gruB) on ctypes mirrors of the layer structs of src/nnet.h, at 128 / 16 / 16
  blob_crc, in_crc: CRC-32 of the model blob and of the input PCM

    python tests/tools/make_golden_plc.py [OUT.npz]
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import synth  # noqa: E402

f32 = np.float32


class DenseLayer(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("input_weights", C.c_void_p), ("nb_inputs", C.c_int), ("nb_neurons", C.c_int), ("activation", C.c_int)]


class GRULayer(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("subias", C.c_void_p), ("input_weights", C.c_void_p), ("input_weights_idx", C.c_void_p),
                ("recurrent_weights", C.c_void_p), ("nb_inputs", C.c_int), ("nb_neurons", C.c_int), ("activation", C.c_int), ("reset_after", C.c_int)]


ACTIVATION_LINEAR, ACTIVATION_TANH = 0, 2          # src/nnet.h


def load_ref(path=os.path.join(pm.ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")):
    L = C.CDLL(path)
    L.lpcnet_plc_create.restype = C.c_void_p
    L.lpcnet_plc_create.argtypes = [C.c_int]
    L.lpcnet_plc_destroy.argtypes = [C.c_void_p]
    L.lpcnet_plc_load_model.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lpcnet_plc_update.argtypes = [C.c_void_p, C.c_void_p]
    L.lpcnet_plc_conceal.argtypes = [C.c_void_p, C.c_void_p]
    L.lpcnet_plc_fec_add.argtypes = [C.c_void_p, C.c_void_p]
    L.lpcnet_plc_fec_clear.argtypes = [C.c_void_p]
    L.burg_cepstral_analysis.argtypes = [C.c_void_p, C.c_void_p]
    L._lpcnet_compute_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.compute_gruB.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def run_stream(L, blob, options, pcm, lost, ops=None, vec=None):
    """(T, 160) int16 in -> (T, 160) out, and the control summaries"""
    st = L.lpcnet_plc_create(options)
    assert L.lpcnet_plc_load_model(st, blob, len(blob)) == 0
    ctl = pm.PlcControl(options)
    out = np.zeros_like(pcm)
    sm = np.zeros((pcm.shape[0], 10), np.int32)
    for t in range(pcm.shape[0]):
        if ops is not None:
            op = int(ops[t])
            pm.apply_fec_op(ctl, op)
            if op == 1 or op == 4:
                for k in range(2 if op == 4 else 1):
                    v = np.ascontiguousarray(vec[t, k])
                    L.lpcnet_plc_fec_add(st, v.ctypes.data)
            elif op == 2:
                L.lpcnet_plc_fec_add(st, None)
            elif op == 3:
                L.lpcnet_plc_fec_clear(st)
        frame = np.ascontiguousarray(pcm[t]).copy()
        if lost[t]:
            frame[:] = 0
            L.lpcnet_plc_conceal(st, frame.ctypes.data)
        else:
            L.lpcnet_plc_update(st, frame.ctypes.data)
        out[t] = frame
        sm[t] = ctl.step(int(lost[t]))
    L.lpcnet_plc_destroy(st)
    return out, sm


def ref_pred_trace(L, blob, xs):
    a = pm.blob_arrays(blob)
    keep = {k: np.frombuffer(v, np.uint8).copy() for k, v in a.items() if k.startswith("plc_")}
    ptr = lambda k: keep[k].ctypes.data
    d1 = DenseLayer(ptr("plc_dense1_bias"), ptr("plc_dense1_weights"), 57, 128, ACTIVATION_TANH)
    g1 = GRULayer(ptr("plc_gru1_bias"), ptr("plc_gru1_subias"), ptr("plc_gru1_weights"), ptr("plc_gru1_weights_idx"), ptr("plc_gru1_recurrent_weights"), 128, 16, ACTIVATION_TANH, 1)
    g2 = GRULayer(ptr("plc_gru2_bias"), ptr("plc_gru2_subias"), ptr("plc_gru2_weights"), ptr("plc_gru2_weights_idx"), ptr("plc_gru2_recurrent_weights"), 16, 16, ACTIVATION_TANH, 1)
    do = DenseLayer(ptr("plc_out_bias"), ptr("plc_out_weights"), 16, 20, ACTIVATION_LINEAR)
    zeros = np.zeros(3 * 16, f32)
    s1, s2 = np.zeros(16, f32), np.zeros(16, f32)
    outs = np.zeros((xs.shape[0], 20), f32)
    for t, x in enumerate(xs):
        x = np.ascontiguousarray(x, f32)
        dense_out = np.zeros(128, f32)
        L._lpcnet_compute_dense(C.byref(d1), dense_out.ctypes.data, x.ctypes.data)
        L.compute_gruB(C.byref(g1), zeros.ctypes.data, s1.ctypes.data, dense_out.ctypes.data)
        L.compute_gruB(C.byref(g2), zeros.ctypes.data, s2.ctypes.data, s1.ctypes.data)
        o = np.zeros(20, f32)
        L._lpcnet_compute_dense(C.byref(do), o.ctypes.data, s2.ctypes.data)
        v = f32(o[19] + f32(0.1))
        o[19] = f32(0.5) if f32(0.5) < v else v          # out[19] = MIN16(.5f, out[19]+.1f)
        outs[t] = o
    return outs


def main():
    L = load_ref()
    blob = synth.blob_bytes(plc_synth.make_model_with_plc())
    pcm = np.stack([pm.stream_pcm(s) for s in range(pm.N_STREAMS)])
    lost = pm.loss_patterns()
    pcm_crc, pcm_full, summ = [], [], []
    for opt in pm.OPTION_SETS:
        res = [run_stream(L, blob, opt, pcm[s], lost[s]) for s in range(pm.N_STREAMS)]
        out = np.stack([r[0] for r in res])
        pcm_crc.append(pm.block_crc(out)); pcm_full.append(out[pm.FULL_STREAM, pm.FULL_FRAMES[0]:pm.FULL_FRAMES[1]]); summ.append(np.stack([r[1] for r in res], axis=1))
        print("options", opt, "lost frames", int(lost.sum()), "nonzero concealed samples", int((out[lost.astype(bool)] != 0).sum()))
    ops, vec = pm.fec_schedule()
    flost = pm.fec_loss_patterns()
    res = [run_stream(L, blob, 0, pcm[s], flost[s], ops[:, s], vec[:, s]) for s in range(pm.N_STREAMS)]
    fout = np.stack([r[0] for r in res])
    fsum = np.stack([r[1] for r in res], axis=1)
    print("FEC vectors used", int(fsum[..., 4].sum()))
    frames = pm.burg_frames()
    burg = np.zeros((frames.shape[0], 36), f32)
    for k, fr in enumerate(frames):
        x = np.ascontiguousarray(fr, f32)
        L.burg_cepstral_analysis(burg[k].ctypes.data, x.ctypes.data)
    xs = pm.pred_inputs()
    pred = ref_pred_trace(L, blob, xs)
    net = pm.PlcNetNumpy(blob)
    mine = np.stack([net.pred(x) for x in xs])
    print("NumPy restatement equals the reference:", np.array_equal(mine.view(np.uint32), pred.view(np.uint32)))
    assert np.array_equal(summ[0], summ[2]) and np.array_equal(summ[1], summ[3])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_plc_v1.npz")
    np.savez_compressed(out_path, pcm_crc=np.stack(pcm_crc), pcm_full=np.stack(pcm_full),
                        summary=np.stack(summ[:2]).astype(np.int16), fec_crc=pm.block_crc(fout),
                        fec_full=fout[pm.FEC_FULL_STREAM, pm.FEC_FULL_FRAMES[0]:pm.FEC_FULL_FRAMES[1]], fec_summary=fsum.astype(np.int16), burg=burg, pred=pred,
                        blob_crc=np.uint32(zlib.crc32(blob)), in_crc=np.uint32(zlib.crc32(pcm.tobytes())), options=np.array(pm.OPTION_SETS, np.int32))


if __name__ == "__main__":
    main()
