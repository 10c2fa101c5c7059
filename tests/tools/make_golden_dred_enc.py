#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_enc_v1.npz from the compiled reference (oracle/_ref/liblpcnet_ref_gf.so, the generic-C float build,
`make -C oracle ref`), driven through ctypes.  The reference's exported layer functions are chained on ctypes mirrors of the layer structs of
src/nnet.h in the sequence of dred_rdovae_encode_dframe (src/dred_rdovae_enc.c:38-95):

  enc_dense1, GRU enc_dense2 (:56-57: the state is copied into the buffer), enc_dense3, GRU enc_dense4, enc_dense5, GRU enc_dense6, enc_dense7,
  enc_dense8 (:52-84); bits_dense over [bits_dense_state | buffer] (:87); gdense1 over the buffer, gdense2 (:91-93)

bits_dense is a compute_conv1d (src/nnet.c:452-470): it copies its memory and the input into a stack buffer, runs bias + sgemv_accum(output, weights,
N, K M, N, tmp) + the linear activation, and shifts the memory.  The oracle's build gives that buffer 384 floats, and the window of the training
defaults has 5 632.  The sum itself is what _lpcnet_compute_dense (src/nnet.c:122-135) does for a DenseLayer with nb_inputs = K M -- the same static
sgemv_accum with the same arguments in the same object file, and no stack buffer -- so this tool assembles the window itself (data movement) and takes
the sum from the reference's compiled dense function at every width set.  At the set `narrow` (K M = 366) it ALSO runs compute_conv1d itself with its
memory and asserts that every latent of every double frame and the shifted memory agree in all bits; compute_conv1d is never called with K M > 384.

Inputs are seeded (tests/tools/dred_enc_model.py); the fixture holds results:

  lat_<set>, init_<set>    [9][7][latent] / [9][7][state] float32 for the width sets tf, w256 and narrow (count = dred_enc_model.COUNT; rows past
                           count[s] are zero)
  gru_<set>                [9][gru floats]: every stream's final GRU states (dense2_state, dense4_state, dense6_state)
  mem_crc_<set>, mem_full_<set>: CRC-32 of every stream's final conv memory, and stream 0's in full
  long_crc                 [16] CRC-32 over every stream's latent and initial-state rows of the long run at `tf` (26 double frames, LONG_COUNT)
  long_lat, long_init      stream 3 of it in full;  long_gru_crc, long_mem_crc: CRC-32 of every stream's final GRU states / conv memory
  rt_feat                  [2][28][20]: the compiled reference's DECODE (make_golden_dred.RefDecoder) of the reference's own encoder output for
                           streams 0 and 4 of the blob set_blob("tf", with_dec=True): state = initial_state[6], latents 6, 5, .. 0 (dred_enc_model.py)
  blob_crc_<set>, blob_crc_rt, in_crc, long_in_crc: CRC-32 of the model blobs and of the inputs

    python tests/tools/make_golden_dred_enc.py [OUT.npz]
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dred_enc_model as em  # noqa: E402
import plc_model as pm  # noqa: E402
from make_golden_dred import RefDecoder  # noqa: E402
from make_golden_plc import ACTIVATION_LINEAR, ACTIVATION_TANH, DenseLayer, GRULayer  # noqa: E402

f32 = np.float32


class Conv1DLayer(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("input_weights", C.c_void_p), ("nb_inputs", C.c_int), ("kernel_size", C.c_int), ("nb_neurons", C.c_int),
                ("activation", C.c_int)]


def load_ref(path=os.path.join(pm.ROOT, "oracle", "_ref", "liblpcnet_ref_gf.so")):
    L = C.CDLL(path)
    L._lpcnet_compute_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.compute_gruB.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.compute_conv1d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


class RefEncoder:
    """the encoder's layer structs over one blob's arrays"""

    def __init__(self, L, blob):
        self.L = L
        a = pm.blob_arrays(blob)
        self.keep = {k: np.frombuffer(v, np.uint8).copy() for k, v in a.items() if k.startswith(("enc_dense", "bits_dense", "gdense"))}
        ptr = lambda k: self.keep[k].ctypes.data
        size = lambda k: self.keep[k].size // 4
        W = self.widths = [size("enc_dense%d_bias" % (k + 1)) // (6 if k in em.GRU_AT else 1) for k in range(8)]
        self.total = sum(W)
        self.latent_dim = size("bits_dense_bias")
        self.taps = size("bits_dense_weights") // (self.total * self.latent_dim)
        self.gdense1, self.state_dim = size("gdense1_bias"), size("gdense2_bias")

        def dense(name, n_in, n_out, act):
            return DenseLayer(ptr(name + "_bias"), ptr(name + "_weights"), n_in, n_out, act)

        self.layers, prev = [], em.IN_DIM
        for k in range(8):
            name = "enc_dense%d" % (k + 1)
            if k in em.DENSE_AT:
                self.layers.append(dense(name, prev, W[k], ACTIVATION_TANH))
            else:
                self.layers.append(GRULayer(ptr(name + "_bias"), ptr(name + "_subias"), ptr(name + "_weights"), ptr(name + "_weights_idx"),
                                            ptr(name + "_recurrent_weights"), prev, W[k], ACTIVATION_TANH, 1))
            prev = W[k]
        self.bits_as_dense = dense("bits_dense", self.taps * self.total, self.latent_dim, ACTIVATION_LINEAR)
        self.bits_conv = Conv1DLayer(ptr("bits_dense_bias"), ptr("bits_dense_weights"), self.total, self.taps, self.latent_dim, ACTIVATION_LINEAR)
        self.g1 = dense("gdense1", self.total, self.gdense1, ACTIVATION_TANH)
        self.g2 = dense("gdense2", self.gdense1, self.state_dim, ACTIVATION_TANH)
        self.gru_floats = sum(W[k] for k in em.GRU_AT)
        self.state_floats = self.gru_floats + (self.taps - 1) * self.total
        self.conv_checked = 0

    def conv1d_itself(self, mem, buf):
        """compute_conv1d on a copy of `mem`: (latents, the shifted memory).  Refused where the window overruns the reference's stack buffer"""
        if self.taps * self.total > em.MAX_CONV:
            raise ValueError("compute_conv1d: a window of %d floats overruns the reference's %d-float stack buffer" % (self.taps * self.total, em.MAX_CONV))
        mem = mem.copy()
        out = np.zeros(self.latent_dim, f32)
        self.L.compute_conv1d(C.byref(self.bits_conv), out.ctypes.data, mem.ctypes.data, buf.ctypes.data)
        return out, mem

    def encode_dframe(self, st, x40):
        """one double frame: the state vector `st` (the reference's member order) advances in place -> (latents, initial state)"""
        L, W = self.L, self.widths
        o = np.concatenate([[0], np.cumsum([W[k] for k in em.GRU_AT])]).astype(int)
        h = [np.ascontiguousarray(st[o[g]:o[g + 1]]) for g in range(3)]
        mem = st[self.gru_floats:]
        zeros = np.zeros(1024, f32)                              # zero_vector, src/dred_rdovae_enc.c:49
        off = np.concatenate([[0], np.cumsum(W)]).astype(int)
        buf = np.zeros(self.total + self.gdense1, f32)
        x = np.ascontiguousarray(x40, f32)
        src = x.ctypes.data
        for k in range(8):                                       # :52-84
            dst = buf[off[k]:off[k + 1]]
            if k in em.DENSE_AT:
                L._lpcnet_compute_dense(C.byref(self.layers[k]), dst.ctypes.data, src)
            else:
                g = em.GRU_AT.index(k)
                L.compute_gruB(C.byref(self.layers[k]), zeros.ctypes.data, h[g].ctypes.data, src)
                dst[:] = h[g]                                    # RNN_COPY(&buffer[output_index], enc_state->dense2_state, ...)
                st[o[g]:o[g + 1]] = h[g]
            src = dst.ctypes.data
        # :87 by the dense route: the window [mem | buffer] assembled here, the sum by the reference's _lpcnet_compute_dense
        window = np.ascontiguousarray(np.concatenate([mem, buf[:self.total]]))
        lat = np.zeros(self.latent_dim, f32)
        L._lpcnet_compute_dense(C.byref(self.bits_as_dense), lat.ctypes.data, window.ctypes.data)
        shifted = window[self.total:].copy()                     # src/nnet.c:468-469
        if self.taps * self.total <= em.MAX_CONV:                # ... and by compute_conv1d itself where its buffer holds the window
            lat2, mem2 = self.conv1d_itself(np.ascontiguousarray(mem), np.ascontiguousarray(buf[:self.total]))
            assert np.array_equal(lat.view(np.uint32), lat2.view(np.uint32)) and np.array_equal(shifted.view(np.uint32), mem2.view(np.uint32)), \
                "the dense route and compute_conv1d differ"
            self.conv_checked += 1
        mem[:] = shifted
        L._lpcnet_compute_dense(C.byref(self.g1), buf[self.total:].ctypes.data, buf.ctypes.data)          # :91
        init = np.zeros(self.state_dim, f32)
        L._lpcnet_compute_dense(C.byref(self.g2), init.ctypes.data, buf[self.total:].ctypes.data)         # :93
        return lat, init

    def encode_all(self, feat, count):
        n, D = feat.shape[0], feat.shape[1] // 2
        lat, init = np.zeros((n, D, self.latent_dim), f32), np.zeros((n, D, self.state_dim), f32)
        states = np.zeros((n, self.state_floats), f32)           # DRED_rdovae_init_encoder
        for s in range(n):
            for d in range(int(count[s])):
                lat[s, d], init[s, d] = self.encode_dframe(states[s], np.concatenate([feat[s, 2 * d], feat[s, 2 * d + 1]]))
        return lat, init, states


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def main():
    L = load_ref()
    res = {}
    feat = em.inputs()
    res["in_crc"] = np.uint32(zlib.crc32(feat.tobytes()))
    assert em.COUNT.min() == 0 and em.COUNT.max() == em.N_DFRAMES and (em.COUNT[em.COUNT > 0] < 3).any()
    for name in em.SETS:
        blob = em.set_blob(name)
        ref = RefEncoder(L, blob)
        lat, init, states = ref.encode_all(feat, em.COUNT)
        net = em.DredEncNumpy(blob)
        m_lat, m_init, m_states = net.encode_all(feat, em.COUNT)
        ok = same(m_lat, lat) and same(m_init, init) and same(m_states, states)
        finite = bool(np.isfinite(lat).all() and np.isfinite(init).all() and np.isfinite(states).all())
        print(name, "NumPy restatement equals the reference:", ok, "| finite:", finite, "| max abs latent", float(np.abs(lat).max()),
              "| double frames where compute_conv1d itself ran and agreed:", ref.conv_checked)
        assert ok and finite
        assert (ref.conv_checked == int(em.COUNT.sum())) == (name == "narrow")
        if name != "narrow":                                     # (the refusal: never into the reference's stack buffer with a longer window)
            try:
                ref.conv1d_itself(np.zeros((ref.taps - 1) * ref.total, f32), np.zeros(ref.total, f32))
                raise AssertionError("compute_conv1d was called with a window beyond its buffer")
            except ValueError:
                pass
        # the fixture senses the order of the window's sum: taken from the last term down, more than half of stream 0's latents change
        desc = em.DredEncNumpy(blob, descending_conv=True)
        d_lat, _ = desc.encode(desc.fresh(), feat[0], int(em.COUNT[0]))
        changed = int((d_lat.view(np.uint32) != lat[0, :int(em.COUNT[0])].view(np.uint32)).sum())
        print(name, "latents of stream 0 that a descending window sum changes:", changed, "of", d_lat.size)
        assert em.COUNT[0] == em.N_DFRAMES and changed > d_lat.size // 2
        # the scaled double frame of stream 0 drives enc_dense1 past the tanh table's last knot (index 200: |x| > 8); one double frame is all zero
        pre = net.enc1_preact(np.concatenate([feat[0, 0], feat[0, 1]]))
        print(name, "enc_dense1 pre-activations beyond the table's last knot, stream 0 double frame 0:", int((np.abs(pre) > 8).sum()), "of", pre.size)
        assert (np.abs(pre) > 8).any() and not feat[0, 6:8].any()
        res["lat_" + name], res["init_" + name] = lat, init
        res["gru_" + name] = states[:, :ref.gru_floats].copy()
        res["mem_crc_" + name] = em.mem_crc(states, ref.gru_floats)
        res["mem_full_" + name] = states[0, ref.gru_floats:].copy()
        res["blob_crc_" + name] = np.uint32(zlib.crc32(blob))
    # the long run at the training defaults
    blob = em.set_blob("tf")
    feat = em.long_inputs()
    ref = RefEncoder(L, blob)
    lat, init, states = ref.encode_all(feat, em.LONG_COUNT)
    assert np.isfinite(lat).all() and np.isfinite(init).all() and np.isfinite(states).all()
    s = em.LONG_FULL_STREAM
    m_lat, m_init = (lambda net: net.encode(net.fresh(), feat[s], int(em.LONG_COUNT[s])))(em.DredEncNumpy(blob))
    assert same(m_lat, lat[s]) and same(m_init, init[s])
    res["long_crc"] = em.rows_crc(lat, init, em.LONG_COUNT)
    res["long_lat"], res["long_init"] = lat[s], init[s]
    res["long_gru_crc"] = np.array([zlib.crc32(st[:ref.gru_floats].tobytes()) for st in states], np.uint32)
    res["long_mem_crc"] = em.mem_crc(states, ref.gru_floats)
    res["long_in_crc"] = np.uint32(zlib.crc32(feat.tobytes()))
    # encoder -> decoder on a blob with both networks: the reference's decode of the reference's encoder output
    blob = em.set_blob("tf", with_dec=True)
    assert pm.blob_arrays(blob)["bits_dense_weights"] == pm.blob_arrays(em.set_blob("tf"))["bits_dense_weights"]
    feat = em.inputs()
    dec = RefDecoder(L, blob)
    assert (dec.latent_dim, dec.state_dim) == (em.SETS["tf"]["latent_dim"], em.SETS["tf"]["state_dim"])
    rt = []
    for s in em.RT_STREAMS:
        c = int(em.COUNT[s])
        assert c == em.N_DFRAMES
        rt.append(dec.decode(res["init_tf"][s, c - 1], res["lat_tf"][s, :c][::-1], c))
    res["rt_feat"] = np.stack(rt)
    assert np.isfinite(res["rt_feat"]).all()
    res["blob_crc_rt"] = np.uint32(zlib.crc32(blob))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_enc_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 150 * 1024


if __name__ == "__main__":
    main()
