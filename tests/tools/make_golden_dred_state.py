#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_state_v1.npz: the DRED decoder's per-stream state (RDOVAEDecState, src/dred_rdovae_dec.h:35-39: dense2_state,
dense4_state, dense6_state) as the compiled reference leaves it after dred_rdovae_dec_init_states and after every dred_rdovae_decode_qframe
(src/dred_rdovae_dec.c:37-98) -- what lpcnet_batch_dred_init / _dred_step keep per stream and get_dred_dec_state returns.

The chain is make_golden_dred.RefDecoder's: the reference's exported layer functions (_lpcnet_compute_dense, compute_gruB) of
oracle/_ref/liblpcnet_ref_gf.so (generic-C float) and liblpcnet_ref_gi.so (generic-C int8, on dred_i8_model's blobs), in the decoder's sequence, with
the three GRU states recorded between the calls.  Width sets, inputs and counts are dred_model's.  The fixture holds results:

  state_<flavour>_<set>   [9][8][W] float32: stream s's three states end to end (W = the sum of the GRU widths) after init_states (row 0) and after
                          latent l (row l + 1) for l < count[s]; rows past count[s] + 1 are zero.  f_small, i_small, f_mixed
  zero_state_<flavour>_small, zero_feat_<flavour>_small   [9][3][W], [9][8][20]: two latents decoded from all-zero states (DRED_rdovae_init_decoder)
                          for every stream: the states (row 0 zero) and the features
  blob_crc_*, in_crc_*    CRC-32 of the model blobs and of the inputs

Before it writes, the generator asserts that the features its chain produces equal the existing fixtures' (golden_dred_v1.npz, golden_dred_i8_v1.npz).

    python tests/tools/make_golden_dred_state.py [OUT.npz]
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dred_i8_model as di  # noqa: E402
import dred_model as dm  # noqa: E402
import plc_model as pm  # noqa: E402
from make_golden_dred import RefDecoder, load_ref  # noqa: E402
from make_golden_dred_i8 import REF_I8  # noqa: E402

f32 = np.float32
ZERO_LATENTS = 2
CASES = (("f", "small"), ("i", "small"), ("f", "mixed"))


def chain(dec, h, latents, count):
    """RefDecoder.decode's loop from the GRU states `h` (modified in place): -> features [4 count][20], the states after every latent [count][W]"""
    L, W = dec.L, dec.widths
    zeros = np.zeros(1024, f32)
    off = np.concatenate([[0], np.cumsum(W)]).astype(int)
    out, states = np.zeros((4 * count, 20), f32), np.zeros((count, sum(x.size for x in h)), f32)
    for l in range(count):
        buf = np.zeros(off[8], f32)
        x = np.ascontiguousarray(latents[l], f32)
        src = x.ctypes.data
        for k in range(8):
            dst = buf[off[k]:off[k + 1]]
            if k in dm.DENSE_AT:
                L._lpcnet_compute_dense(C.byref(dec.layers[k]), dst.ctypes.data, src)
            else:
                g = dm.GRU_AT.index(k)
                L.compute_gruB(C.byref(dec.layers[k]), zeros.ctypes.data, h[g].ctypes.data, src)
                dst[:] = h[g]
            src = dst.ctypes.data
        q = np.zeros(dm.NB_OUT, f32)
        L._lpcnet_compute_dense(C.byref(dec.final), q.ctypes.data, buf.ctypes.data)
        out[4 * l:4 * l + 4] = q.reshape(4, 20)
        states[l] = np.concatenate(h)
    return out, states


def init_states(dec, state):
    state = np.ascontiguousarray(state, f32)
    h = [np.zeros(dec.widths[k], f32) for k in dm.GRU_AT]
    for k in range(3):
        dec.L._lpcnet_compute_dense(C.byref(dec.state[k]), h[k].ctypes.data, state.ctypes.data)
    return h


def main():
    gold = {"f": np.load(os.path.join(pm.ROOT, "tests", "golden", "golden_dred_v1.npz")), "i": np.load(os.path.join(pm.ROOT, "tests", "golden", "golden_dred_i8_v1.npz"))}
    lib = {"f": load_ref(), "i": load_ref(REF_I8)}
    res = {}
    for fl, name in CASES:
        blob = dm.set_blob(name) if fl == "f" else di.blob_dec(name)
        state, latents = dm.set_inputs(name)
        assert np.uint32(zlib.crc32(blob)) == gold[fl]["blob_crc_" + name] and np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == gold[fl]["in_crc_" + name]
        dec = RefDecoder(lib[fl], blob)
        W = sum(dec.widths[k] for k in dm.GRU_AT)
        st = np.zeros((dm.N_STREAMS, dm.N_LATENTS + 1, W), f32)
        feat = np.zeros((dm.N_STREAMS, 4 * dm.N_LATENTS, 20), f32)
        for s in range(dm.N_STREAMS):
            c = int(dm.COUNT[s])
            h = init_states(dec, state[s])
            st[s, 0] = np.concatenate(h)
            feat[s, :4 * c], st[s, 1:c + 1] = chain(dec, h, latents[s], c)
        same = np.array_equal(feat.view(np.uint32), gold[fl]["feat_" + name].view(np.uint32))
        print(fl, name, "the chain's features equal the existing fixture's:", same, "| states finite:", bool(np.isfinite(st).all()), "| max abs", float(np.abs(st).max()))
        assert same and np.isfinite(st).all()
        # the states move: no latent leaves a stream's record as it found it
        for s in range(dm.N_STREAMS):
            for l in range(int(dm.COUNT[s])):
                assert not np.array_equal(st[s, l], st[s, l + 1]), (fl, name, s, l)
        res["state_%s_%s" % (fl, name)] = st
        res["blob_crc_%s_%s" % (fl, name)] = np.uint32(zlib.crc32(blob))
        res["in_crc_%s_%s" % (fl, name)] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
        if name == "small":
            zs = np.zeros((dm.N_STREAMS, ZERO_LATENTS + 1, W), f32)
            zf = np.zeros((dm.N_STREAMS, 4 * ZERO_LATENTS, 20), f32)
            for s in range(dm.N_STREAMS):
                h = [np.zeros(dec.widths[k], f32) for k in dm.GRU_AT]      # DRED_rdovae_init_decoder
                zf[s], zs[s, 1:] = chain(dec, h, latents[s], ZERO_LATENTS)
            assert np.isfinite(zf).all() and not np.array_equal(zf, feat[:, :4 * ZERO_LATENTS])
            res["zero_state_%s_small" % fl], res["zero_feat_%s_small" % fl] = zs, zf
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_state_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 150 * 1024


if __name__ == "__main__":
    main()
