"""TEST TOOLING shared by tests/tools/make_golden_dred_i8.py, tests/tools/make_golden_dred_enc_i8.py, tests/test_dred_i8_host.py,
tests/test_gpu_dred_i8.py, tests/test_gpu_dred_enc_i8.py and the --int8 runs of tools/dred_rate.py / tools/dred_enc_rate.py: both DRED halves of an
int8 (DOT_PROD) blob.
  * blobs: dred_model.add_dred / dred_enc_model.add_dred_enc with gru_flavour="int8" on the int8 LPCNet test model, with or without the int8 PLC
    network of plc_synth; the width sets, inputs and counts are dred_model's and dred_enc_model's own;
  * DredDecNumpyI8 / DredEncNumpyI8: the two chains as the reference's generic-C int8 build runs them -- every dense layer in float
    (plc_model.PlcNetNumpy._dense: the int8 build's _lpcnet_compute_dense and compute_conv1d work on float weights), the three GRUs of each half
    through plc_i8_model.PlcNetNumpyI8._gru (compute_gruB over sparse_sgemv_accum8x4 / sgemv_accum8x4, src/vec.h:274-339).  The fixtures
    (tests/golden/golden_dred_i8_v1.npz, golden_dred_enc_i8_v1.npz) pin both to the reference.
    unscaled=True is the generators' sensitivity check: the accumulator is left unscaled -- each block's integer sum is multiplied by 1/128/127 and
    added to the plain bias -- the same terms with other roundings;
    every quantisation point asserts |x| <= 1: GRU inputs and states are tanh outputs or convex combinations of them, so the reference's
    (signed char) conversion never wraps.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpcnet_amd import synth  # noqa: E402
import dred_enc_model as em  # noqa: E402
import dred_model as dm  # noqa: E402
import plc_i8_model as pq  # noqa: E402
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402

f32 = np.float32


def _base(with_plc):
    return plc_synth.make_model_with_plc(flavour="int8") if with_plc else synth.make_model(flavour="int8")


def blob_dec(name, with_plc=False, with_enc=None):
    """the int8 LPCNet test model (with the int8 PLC network if with_plc), the int8 encoder of dred_enc_model's set `with_enc` if given, and the int8
    decoder of dred_model's set `name`"""
    m = _base(with_plc)
    if with_enc:
        s = em.SETS[with_enc]
        em.add_dred_enc(m, s["widths"], taps=s["taps"], latent_dim=s["latent_dim"], gdense1=s["gdense1"], state_dim=s["state_dim"], gru_flavour="int8")
    return synth.blob_bytes(dm.add_dred(m, dm.SETS[name]["widths"], dm.SETS[name]["latent_dim"], gru_flavour="int8"))


def blob_enc(name, with_dec=False):
    """the int8 LPCNet test model followed by the int8 encoder of dred_enc_model's set `name` (with_dec: and the int8 decoder of dred_model's set
    "mixed" -- latent 80, state 24 -- behind it)"""
    return blob_dec("mixed", with_enc=name) if with_dec else _enc_only(name)


def _enc_only(name):
    s = em.SETS[name]
    m = _base(False)
    em.add_dred_enc(m, s["widths"], taps=s["taps"], latent_dim=s["latent_dim"], gdense1=s["gdense1"], state_dim=s["state_dim"], gru_flavour="int8")
    return synth.blob_bytes(m)


def gru_i8(a, name, n):
    """the record PlcNetNumpyI8._gru takes, from a blob's arrays"""
    g = lambda k, dt=f32: np.frombuffer(a[k], dt)
    return dict(N=n, bias=g(name + "_bias"), w=g(name + "_weights", np.int8).reshape(-1, 8, 4).astype(np.int32), idx=g(name + "_weights_idx", np.int32),
                rec=g(name + "_recurrent_weights", np.int8).reshape(3 * n // 8, n // 4, 8, 4).astype(np.int32))


def gru_unscaled(G, state, x):
    """PlcNetNumpyI8._gru with the accumulator left unscaled: from the plain bias, each block's integer sum times 1/128/127 added"""
    N = G["N"]
    xq, sq = pq.quant_s8(x), pq.quant_s8(state)
    zrh = (G["bias"][:3 * N] + f32(0)).astype(f32)
    idx, p, blk = G["idx"], 0, 0
    for grp in range(3 * N // 8):
        cnt = int(idx[p]); p += 1
        y = zrh[grp * 8:grp * 8 + 8]
        for _ in range(cnt):
            pos = int(idx[p]); p += 1
            y = (y + ((G["w"][blk] @ xq[pos:pos + 4]).astype(f32) * pq.SCALE_1).astype(f32)).astype(f32)
            blk += 1
        zrh[grp * 8:grp * 8 + 8] = y
    recur = G["bias"][3 * N:].copy()
    for j in range(N // 4):
        recur = (recur + ((G["rec"][:, j] @ sq[4 * j:4 * j + 4]).reshape(3 * N).astype(f32) * pq.SCALE_1).astype(f32)).astype(f32)
    zr = pm.sigmoid_approx(zrh[:2 * N] + recur[:2 * N])
    z, r = zr[:N], zr[N:]
    h = pm.tanh_approx(zrh[2 * N:] + recur[2 * N:] * r)
    return (z * state + (f32(1) - z) * h).astype(f32)


class _GruI8:
    """the GRU call both restatements share: the range check at the two quantisation points, then the int8 compute_gruB"""
    unscaled = False

    def _gru(self, G, state, x):
        assert np.abs(x).max() <= 1 and np.abs(state).max() <= 1, "a GRU input or state beyond [-1, 1]: the reference's signed char would wrap"
        return gru_unscaled(G, state, x) if self.unscaled else pq.PlcNetNumpyI8._gru(G, state, x)


class DredDecNumpyI8(_GruI8, dm.DredDecNumpy):
    def __init__(self, blob, unscaled=False):
        a = pm.blob_arrays(blob)
        g = lambda k, dt=f32: np.frombuffer(a[k], dt)
        self.widths = [g(n + "_bias").size if n in dm.DENSE_NAMES else g(n + "_bias").size // 6 for n in ("dec_dense%d" % (k + 1) for k in range(8))]
        self.latent_dim = g("dec_dense1_weights").size // self.widths[0]
        self.state_dim = g("state1_weights").size // self.widths[1]
        dense = lambda name, n_in: (g(name + "_weights").reshape(n_in, -1), g(name + "_bias"))
        self.state = [dense("state%d" % (k + 1), self.state_dim) for k in range(3)]
        self.layers, prev = [], self.latent_dim
        for k in range(8):
            name = "dec_dense%d" % (k + 1)
            self.layers.append(dense(name, prev) if k in dm.DENSE_AT else gru_i8(a, name, self.widths[k]))
            prev = self.widths[k]
        self.final = dense("dec_final", sum(self.widths))
        self.unscaled = unscaled


class DredEncNumpyI8(_GruI8, em.DredEncNumpy):
    def __init__(self, blob, unscaled=False):
        a = pm.blob_arrays(blob)
        g = lambda k, dt=f32: np.frombuffer(a[k], dt)
        self.widths = [g(n + "_bias").size if n in em.DENSE_NAMES else g(n + "_bias").size // 6 for n in ("enc_dense%d" % (k + 1) for k in range(8))]
        self.total = sum(self.widths)
        self.latent_dim = g("bits_dense_bias").size
        self.taps = g("bits_dense_weights").size // (self.total * self.latent_dim)
        self.gdense1 = g("gdense1_bias").size
        self.state_dim = g("gdense2_bias").size
        dense = lambda name, n_in: (g(name + "_weights").reshape(n_in, -1), g(name + "_bias"))
        self.layers, prev = [], em.IN_DIM
        for k in range(8):
            name = "enc_dense%d" % (k + 1)
            self.layers.append(dense(name, prev) if k in em.DENSE_AT else gru_i8(a, name, self.widths[k]))
            prev = self.widths[k]
        self.bits = dense("bits_dense", self.taps * self.total)
        self.g1 = dense("gdense1", self.total)
        self.g2 = dense("gdense2", self.gdense1)
        self.gru_floats = sum(self.widths[k] for k in em.GRU_AT)
        self.state_floats = self.gru_floats + (self.taps - 1) * self.total
        self.unscaled = unscaled

    def encode_dframe(self, st, x40):
        """dred_enc_model.DredEncNumpy.encode_dframe with the int8 GRUs"""
        dn = pm.PlcNetNumpy._dense
        h, mem = self._split(st)
        x, buf = np.asarray(x40, f32), []
        for k in range(8):
            if k in em.DENSE_AT:
                x = pm.tanh_approx(dn(self.layers[k][0], self.layers[k][1], x))
            else:
                g = em.GRU_AT.index(k)
                h[g][:] = self._gru(self.layers[k], h[g].copy(), x)
                x = h[g].copy()
            buf.append(x)
        buf = np.concatenate(buf)
        window = np.concatenate([mem, buf])
        lat = dn(self.bits[0], self.bits[1], window)
        mem[:] = window[self.total:]
        g1 = pm.tanh_approx(dn(self.g1[0], self.g1[1], buf))
        return lat, pm.tanh_approx(dn(self.g2[0], self.g2[1], g1))
