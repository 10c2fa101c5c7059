#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_v1.npz from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so, the generic-C float build,
`make -C oracle ref`), driven through ctypes.  The reference's exported layer functions (_lpcnet_compute_dense, compute_gruB) are chained on
ctypes mirrors of the layer structs of src/nnet.h in the sequence of the DRED decoder:

  dred_rdovae_dec_init_states   src/dred_rdovae_dec.c:37-47    the three GRU states = dense(state1..3) of the initial state, tanh
  dred_rdovae_decode_qframe     src/dred_rdovae_dec.c:50-98    dec_dense1, GRU dec_dense2 (:66-69: the state is copied into the buffer), dec_dense3, GRU
                                                               dec_dense4 (:75-78), dec_dense5, GRU dec_dense6 (:84-87), dec_dense7, dec_dense8,
                                                               dec_final over the whole buffer (:97)
  DRED_rdovae_decode_all        src/dred_rdovae.c:38-52        latent l -> features[4 l .. 4 l + 3]

Inputs are seeded (tests/tools/dred_model.py); the fixture holds results:

  feat_<set>   [9][28][20] float32 for the width sets w256, mixed and small (7 latents, count = dred_model.COUNT; rows past 4 count[s] are zero)
  long_crc     [16] CRC-32 of every stream's decoded rows of the long run at width 256 (26 latents, count = dred_model.LONG_COUNT),
  long_full    [104][20] stream 3 of it in full
  blob_crc_<set>, in_crc_<set>, long_in_crc: CRC-32 of the model blobs and of the inputs

    python tests/tools/make_golden_dred.py [OUT.npz]
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dred_model as dm  # noqa: E402
import plc_model as pm  # noqa: E402
from make_golden_plc import ACTIVATION_LINEAR, ACTIVATION_TANH, DenseLayer, GRULayer  # noqa: E402

f32 = np.float32


def load_ref(path=os.path.join(pm.ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")):
    L = C.CDLL(path)
    L._lpcnet_compute_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.compute_gruB.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


class RefDecoder:
    """the decoder's layer structs over one blob's arrays"""

    def __init__(self, L, blob):
        self.L = L
        a = pm.blob_arrays(blob)
        self.keep = {k: np.frombuffer(v, np.uint8).copy() for k, v in a.items() if k.startswith(("dec_", "state"))}
        ptr = lambda k: self.keep[k].ctypes.data
        size = lambda k: self.keep[k].size // 4
        self.widths = [size("dec_dense%d_bias" % (k + 1)) // (6 if k in dm.GRU_AT else 1) for k in range(8)]
        self.latent_dim = size("dec_dense1_weights") // self.widths[0]
        self.state_dim = size("state1_weights") // self.widths[1]

        def dense(name, n_in, n_out, act):
            return DenseLayer(ptr(name + "_bias"), ptr(name + "_weights"), n_in, n_out, act)

        self.state = [dense("state%d" % (k + 1), self.state_dim, self.widths[dm.GRU_AT[k]], ACTIVATION_TANH) for k in range(3)]
        self.layers, prev = [], self.latent_dim
        for k in range(8):
            name = "dec_dense%d" % (k + 1)
            if k in dm.DENSE_AT:
                self.layers.append(dense(name, prev, self.widths[k], ACTIVATION_TANH))
            else:
                self.layers.append(GRULayer(ptr(name + "_bias"), ptr(name + "_subias"), ptr(name + "_weights"), ptr(name + "_weights_idx"),
                                            ptr(name + "_recurrent_weights"), prev, self.widths[k], ACTIVATION_TANH, 1))
            prev = self.widths[k]
        self.final = dense("dec_final", sum(self.widths), dm.NB_OUT, ACTIVATION_LINEAR)

    def decode(self, state, latents, count):
        L, W = self.L, self.widths
        state = np.ascontiguousarray(state, f32)
        h = [np.zeros(W[k], f32) for k in dm.GRU_AT]
        for k in range(3):                                       # dred_rdovae_dec_init_states, src/dred_rdovae_dec.c:44-46
            L._lpcnet_compute_dense(C.byref(self.state[k]), h[k].ctypes.data, state.ctypes.data)
        zeros = np.zeros(1024, f32)                              # zero_vector, :60
        off = np.concatenate([[0], np.cumsum(W)]).astype(int)
        out = np.zeros((4 * count, 20), f32)
        for l in range(count):                                   # DRED_rdovae_decode_all, src/dred_rdovae.c:44-51
            buf = np.zeros(off[8], f32)
            x = np.ascontiguousarray(latents[l], f32)
            src = x.ctypes.data
            for k in range(8):                                   # dred_rdovae_decode_qframe, src/dred_rdovae_dec.c:63-95
                dst = buf[off[k]:off[k + 1]]
                if k in dm.DENSE_AT:
                    L._lpcnet_compute_dense(C.byref(self.layers[k]), dst.ctypes.data, src)
                else:
                    g = dm.GRU_AT.index(k)
                    L.compute_gruB(C.byref(self.layers[k]), zeros.ctypes.data, h[g].ctypes.data, src)
                    dst[:] = h[g]                                # RNN_COPY(&buffer[output_index], dec_state->dense2_state, ...)
                src = dst.ctypes.data
            q = np.zeros(dm.NB_OUT, f32)
            L._lpcnet_compute_dense(C.byref(self.final), q.ctypes.data, buf.ctypes.data)      # :97
            out[4 * l:4 * l + 4] = q.reshape(4, 20)
        return out

    def decode_all(self, state, latents, count):
        out = np.zeros((latents.shape[0], 4 * latents.shape[1], 20), f32)
        for s in range(latents.shape[0]):
            out[s, :4 * int(count[s])] = self.decode(state[s], latents[s], int(count[s]))
        return out


def main():
    L = load_ref()
    res = {}
    for name in dm.SETS:
        blob = dm.set_blob(name)
        state, latents = dm.set_inputs(name)
        ref = RefDecoder(L, blob).decode_all(state, latents, dm.COUNT)
        mine = dm.DredDecNumpy(blob).decode_all(state, latents, dm.COUNT)
        same = np.array_equal(mine.view(np.uint32), ref.view(np.uint32))
        print(name, "NumPy restatement equals the reference:", same, "| finite:", bool(np.isfinite(ref).all()), "| max abs", float(np.abs(ref).max()))
        assert same and np.isfinite(ref).all()
        # the fixture senses the order of the recurrent sum: taken from the last unit down, more than half of stream 0's outputs change
        desc = dm.DredDecNumpy(blob, descending_recurrent=True).decode(state[0], latents[0], int(dm.COUNT[0]))
        changed = int((desc.view(np.uint32) != ref[0, :4 * int(dm.COUNT[0])].view(np.uint32)).sum())
        print(name, "outputs of stream 0 that a descending recurrent sum changes:", changed, "of", desc.size)
        assert dm.COUNT[0] == dm.N_LATENTS and changed > desc.size // 2
        # the scaled latent of stream 0 drives dec_dense1 past the tanh table's last knot (index 200: |x| > 8), the zero latent leaves its bias
        net = dm.DredDecNumpy(blob)
        pre = pm.PlcNetNumpy._dense(net.layers[0][0], net.layers[0][1], latents[0, 0])
        print(name, "dec_dense1 pre-activations beyond the table's last knot, stream 0 latent 0:", int((np.abs(pre) > 8).sum()), "of", pre.size)
        assert (np.abs(pre) > 8).any() and not latents[0, 3].any()
        # the packed form of a blob with the PLC network decodes the same values: the decoder's arrays do not depend on what precedes them
        assert pm.blob_arrays(dm.set_blob(name, with_plc=True))["dec_final_weights"] == pm.blob_arrays(blob)["dec_final_weights"]
        res["feat_" + name] = ref
        res["blob_crc_" + name] = np.uint32(zlib.crc32(blob))
        res["in_crc_" + name] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
    blob = dm.set_blob("w256")
    state, latents = dm.long_inputs()
    ref = RefDecoder(L, blob).decode_all(state, latents, dm.LONG_COUNT)
    assert np.isfinite(ref).all()
    res["long_crc"] = dm.stream_crc(ref, dm.LONG_COUNT)
    res["long_full"] = ref[dm.LONG_FULL_STREAM]
    res["long_in_crc"] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 150 * 1024


if __name__ == "__main__":
    main()
