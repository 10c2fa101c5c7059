"""TEST TOOLING shared by tests/tools/make_golden_dred.py, tests/test_dred_host.py, tests/test_gpu_dred.py and tools/dred_rate.py:
  * seeded DRED decoder blobs (state1..3, dec_dense1..8, dec_final in the names and layouts torch/rdovae/export_rdovae_weights.py and
    training_tf2/dump_rdovae.py emit), appended to the LPCNet test model as write_lpcnet_weights.c:72-75 appends the trained ones;
  * the inputs of the fixture (tests/golden/golden_dred_v1.npz): initial states, latents, counts -- seeded, so the fixture stores results only;
  * DredDecNumpy: DRED_rdovae_decode_all (src/dred_rdovae.c:38-52; dred_rdovae_dec_init_states and dred_rdovae_decode_qframe,
    src/dred_rdovae_dec.c:37-98) restated on PlcNetNumpy._dense / ._gru (tests/tools/plc_model.py), which the PLC fixture pins to the
    reference; the DRED fixture pins this chain to the reference at three width sets.
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpcnet_amd import synth  # noqa: E402
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402

f32 = np.float32
STATE_DIM = 24                       # nb_state_dim, training_tf2/rdovae.py:199
NB_OUT = 80                          # four 20-float frames per latent
DENSE_NAMES = ("dec_dense1", "dec_dense3", "dec_dense5", "dec_dense7", "dec_dense8")
GRU_NAMES = ("dec_dense2", "dec_dense4", "dec_dense6")
DENSE_AT, GRU_AT = (0, 2, 4, 6, 7), (1, 3, 5)

# the width sets of the fixture: the dump's default, the defaults of training_tf2/rdovae.py:236-251, and a small one where no width equals another
SETS = {
    "w256": dict(widths=(256,) * 8, latent_dim=80),
    "mixed": dict(widths=(256, 128, 256, 128, 256, 128, 128, 128), latent_dim=80),
    "small": dict(widths=(40, 24, 36, 16, 44, 8, 12, 20), latent_dim=36),
}
N_STREAMS, N_LATENTS = 9, 7
COUNT = np.array([7, 1, 0, 2, 7, 3, 7, 5, 4], np.int32)
LONG_STREAMS, LONG_LATENTS, LONG_FULL_STREAM = 16, 26, 3
LONG_COUNT = np.array([26, 26, 13, 26, 1, 26, 25, 26, 26, 0, 26, 26, 7, 26, 26, 26], np.int32)


def add_dred(m, widths, latent_dim=80, state_dim=STATE_DIM, gru_flavour="float", final_out=NB_OUT, seed=0xD2ED):
    """append a seeded decoder to the model `m`.  gru_flavour: "float", "int8", or one of them per GRU"""
    rng = np.random.default_rng([seed, latent_dim, state_dim] + list(widths))
    flav = (gru_flavour,) * 3 if isinstance(gru_flavour, str) else tuple(gru_flavour)

    def dense(name, n_in, n_out, scale):
        m.add(name + "_weights", (rng.standard_normal((n_in, n_out)) * scale).astype(f32), synth.WEIGHT_TYPE_FLOAT)
        m.add(name + "_bias", (rng.standard_normal(n_out) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)

    for k in range(3):
        dense("state%d" % (k + 1), state_dim, widths[GRU_AT[k]], 0.3)
    prev = latent_dim
    for k in range(8):
        if k in DENSE_AT:
            dense(DENSE_NAMES[DENSE_AT.index(k)], prev, widths[k], 1.2 / np.sqrt(prev))
        else:
            g = GRU_AT.index(k)
            plc_synth._gru(m, GRU_NAMES[g], rng, prev, widths[k], flav[g], block_density=0.5)      # (0.5: row groups without blocks and with all of them)
        prev = widths[k]
    dense("dec_final", int(sum(widths)), final_out, 0.05)
    return m


def blob_dred(widths, latent_dim=80, with_plc=False, **kw):
    """the LPCNet test model (with the PLC network of plc_synth if with_plc) followed by a seeded DRED decoder of these widths"""
    m = plc_synth.make_model_with_plc() if with_plc else synth.make_model()
    return synth.blob_bytes(add_dred(m, widths, latent_dim, **kw))


def set_blob(name, with_plc=False):
    return blob_dred(SETS[name]["widths"], SETS[name]["latent_dim"], with_plc)


def inputs(latent_dim, n_streams=N_STREAMS, n_latents=N_LATENTS, state_dim=STATE_DIM, seed=0x1A7E):
    """state [n][state_dim] uniform in [-1, 1]; latents [n][n_latents][latent_dim] N(0, 1.5^2) with one latent per stream scaled by 8 (the
    tanh table's clamp at index 200) and one all zero"""
    rng = np.random.default_rng([seed, latent_dim, n_streams, n_latents])
    state = rng.uniform(-1, 1, (n_streams, state_dim)).astype(f32)
    latents = (rng.standard_normal((n_streams, n_latents, latent_dim)) * 1.5).astype(f32)
    for s in range(n_streams):
        latents[s, s % n_latents] *= f32(8)
        latents[s, (s + 3) % n_latents] = 0
    return state, latents


def set_inputs(name):
    return inputs(SETS[name]["latent_dim"])


def long_inputs():
    return inputs(SETS["w256"]["latent_dim"], LONG_STREAMS, LONG_LATENTS)


def stream_crc(feat, count):
    """feat [n][4 L][20], count [n] -> CRC-32 of every stream's decoded rows"""
    return np.array([zlib.crc32(np.ascontiguousarray(feat[s, :4 * int(count[s])]).tobytes()) for s in range(feat.shape[0])], np.uint32)


class DredDecNumpy:
    def __init__(self, blob, descending_recurrent=False):
        a = pm.blob_arrays(blob)
        g = lambda k, dt=f32: np.frombuffer(a[k], dt)
        self.widths = [g(n + "_bias").size if n in DENSE_NAMES else g(n + "_bias").size // 6 for n in ("dec_dense%d" % (k + 1) for k in range(8))]
        self.latent_dim = g("dec_dense1_weights").size // self.widths[0]
        self.state_dim = g("state1_weights").size // self.widths[1]
        dense = lambda name, n_in: (g(name + "_weights").reshape(n_in, -1), g(name + "_bias"))
        self.state = [dense("state%d" % (k + 1), self.state_dim) for k in range(3)]
        self.layers, prev = [], self.latent_dim
        for k in range(8):
            name = "dec_dense%d" % (k + 1)
            if k in DENSE_AT:
                self.layers.append(dense(name, prev))
            else:
                n = self.widths[k]
                rec = g(name + "_recurrent_weights").reshape(n, 3 * n)
                self.layers.append(dict(N=n, bias=g(name + "_bias"), w=g(name + "_weights").reshape(-1, 4, 8), idx=g(name + "_weights_idx", np.int32), rec=rec))
            prev = self.widths[k]
        self.final = dense("dec_final", sum(self.widths))
        self.descending = descending_recurrent      # (the generator's order-sensitivity check: the recurrent sum from the last unit down)

    def _gru(self, G, state, x):
        if not self.descending:
            return pm.PlcNetNumpy._gru(G, state, x)
        return self._gru_descending(G, state, x)

    @staticmethod
    def _gru_descending(G, state, x):
        """PlcNetNumpy._gru with the recurrent sum taken over j = N - 1 .. 0: the same terms in another order"""
        N = G["N"]
        zrh = (G["bias"][:3 * N] + f32(0)).astype(f32)
        idx, p, blk = G["idx"], 0, 0
        for grp in range(3 * N // 8):
            cnt = int(idx[p]); p += 1
            y = zrh[grp * 8:grp * 8 + 8]
            for _ in range(cnt):
                pos = int(idx[p]); p += 1
                for k in range(4):
                    y = (y + G["w"][blk, k] * x[pos + k]).astype(f32)
                blk += 1
            zrh[grp * 8:grp * 8 + 8] = y
        recur = G["bias"][3 * N:].copy()
        for j in range(N - 1, -1, -1):
            recur = (recur + G["rec"][j] * state[j]).astype(f32)
        zr = pm.sigmoid_approx(zrh[:2 * N] + recur[:2 * N])
        z, r = zr[:N], zr[N:]
        h = pm.tanh_approx(zrh[2 * N:] + recur[2 * N:] * r)
        return (z * state + (f32(1) - z) * h).astype(f32)

    def decode(self, state, latents, count):
        """one stream: state [state_dim], latents [>= count][latent_dim] -> features [4 count][20]"""
        dn = pm.PlcNetNumpy._dense
        h = [pm.tanh_approx(dn(w, b, np.asarray(state, f32))) for w, b in self.state]
        out = np.zeros((4 * count, 20), f32)
        for l in range(count):
            x, buf = np.asarray(latents[l], f32), []
            for k in range(8):
                if k in DENSE_AT:
                    x = pm.tanh_approx(dn(self.layers[k][0], self.layers[k][1], x))
                else:
                    g = GRU_AT.index(k)
                    h[g] = self._gru(self.layers[k], h[g], x)
                    x = h[g]
                buf.append(x)
            out[4 * l:4 * l + 4] = dn(self.final[0], self.final[1], np.concatenate(buf)).reshape(4, 20)
        return out

    def decode_all(self, state, latents, count, fill=0.0):
        """every stream: -> [n][4 max_latents][20], rows past 4 count[s] hold `fill`"""
        n, L = latents.shape[0], latents.shape[1]
        out = np.full((n, 4 * L, 20), fill, f32)
        for s in range(n):
            out[s, :4 * int(count[s])] = self.decode(state[s], latents[s], int(count[s]))
        return out


def packed(feat, first, take):
    """the packed form's permutation of decoded features [n][rows][20]: rows first[s] .. first[s] + take[s] - 1 of every stream, last row first"""
    rows = [feat[s, first[s]:first[s] + take[s]][::-1] for s in range(feat.shape[0])]
    return np.concatenate(rows) if rows else np.zeros((0, 20), f32)
