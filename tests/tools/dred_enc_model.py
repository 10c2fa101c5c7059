"""TEST TOOLING shared by tests/tools/make_golden_dred_enc.py, tests/test_dred_enc_host.py, tests/test_gpu_dred_enc.py and tools/dred_enc_rate.py:
  * seeded DRED encoder blobs (enc_dense1..8, bits_dense, gdense1, gdense2 in the names and layouts of the reference's rdovae_enc_arrays),
    appended to the LPCNet test model as write_lpcnet_weights.c:72-75 appends the trained ones;
  * the inputs of the fixture (tests/golden/golden_dred_enc_v1.npz): feature frames and counts -- seeded, so the fixture stores results only;
  * DredEncNumpy: dred_rdovae_encode_dframe (src/dred_rdovae_enc.c:38-95) restated on PlcNetNumpy._dense / ._gru (tests/tools/plc_model.py), which
    the PLC fixture pins to the reference; the encoder's fixture pins this chain to the reference at three width sets.

The decoder's view of an encoder's output (what `rt_feat` of the fixture holds, and what a redundancy packet carries): for a stream that has encoded
c double frames, the decoder's initial state is initial_state[c - 1] -- the newest double frame's -- and its latents are latents[c - 1], latents[c - 2],
.. latents[0]: the newest first, each decoding to four feature frames, the newest first."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpcnet_amd import synth  # noqa: E402
import dred_model as dm  # noqa: E402
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402

f32 = np.float32
IN_DIM = 40                          # two 20-float feature frames
MAX_CONV = 384                       # MAX_CONV_INPUTS of the oracle's build of the reference (oracle/refgen.py): compute_conv1d's stack buffer
DENSE_NAMES = ("enc_dense1", "enc_dense3", "enc_dense5", "enc_dense7", "enc_dense8")
GRU_NAMES = ("enc_dense2", "enc_dense4", "enc_dense6")
DENSE_AT, GRU_AT = dm.DENSE_AT, dm.GRU_AT

# the width sets of the fixture: the training defaults (training_tf2/rdovae.py:201-231), width 256 throughout, and a narrow one whose window fits
# compute_conv1d's buffer (3 x 122 = 366 <= 384) and where no width equals another
SETS = {
    "tf": dict(widths=(256, 128, 256, 128, 256, 128, 128, 128), taps=4, latent_dim=80, gdense1=128, state_dim=24),
    "w256": dict(widths=(256,) * 8, taps=4, latent_dim=80, gdense1=128, state_dim=24),
    "narrow": dict(widths=(20, 16, 28, 8, 12, 24, 4, 10), taps=3, latent_dim=18, gdense1=14, state_dim=6),
}
N_STREAMS, N_DFRAMES = 9, 7
COUNT = np.array([7, 1, 0, 2, 7, 3, 7, 5, 4], np.int32)          # (1 and 2: fewer than taps - 1, so zeros remain in the window)
LONG_STREAMS, LONG_DFRAMES, LONG_FULL_STREAM = 16, 26, 3
LONG_COUNT = np.array([26, 26, 13, 26, 1, 26, 25, 26, 26, 0, 26, 26, 7, 26, 26, 26], np.int32)
RT_STREAMS = (0, 4)                  # the two streams of `rt_feat` (count 7) on the blob set_blob("tf", with_dec=True)


def add_dred_enc(m, widths, taps=4, latent_dim=80, gdense1=128, state_dim=24, gru_flavour="float", in_dim=IN_DIM, bits_rows=None, seed=0xE2C0):
    """append a seeded encoder to the model `m`.  gru_flavour: "float", "int8", or one of them per GRU; bits_rows: the rows of bits_dense_weights
    when they are not taps x sum(widths)"""
    rng = np.random.default_rng([seed, taps, latent_dim, gdense1, state_dim] + list(widths))
    flav = (gru_flavour,) * 3 if isinstance(gru_flavour, str) else tuple(gru_flavour)
    total = int(sum(widths))

    def dense(name, n_in, n_out, scale):
        m.add(name + "_weights", (rng.standard_normal((n_in, n_out)) * scale).astype(f32), synth.WEIGHT_TYPE_FLOAT)
        m.add(name + "_bias", (rng.standard_normal(n_out) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)

    prev = in_dim
    for k in range(8):
        if k in DENSE_AT:
            dense(DENSE_NAMES[DENSE_AT.index(k)], prev, widths[k], 1.2 / np.sqrt(prev))
        else:
            g = GRU_AT.index(k)
            plc_synth._gru(m, GRU_NAMES[g], rng, prev, widths[k], flav[g], block_density=0.5)      # (0.5: row groups without blocks and with all of them)
        prev = widths[k]
    rows = taps * total if bits_rows is None else bits_rows
    dense("bits_dense", rows, latent_dim, 1.5 / np.sqrt(rows))
    dense("gdense1", total, gdense1, 1.2 / np.sqrt(total))
    dense("gdense2", gdense1, state_dim, 1.2 / np.sqrt(gdense1))
    return m


def blob_enc(widths, with_dec=False, first=False, **kw):
    """the LPCNet test model followed by a seeded encoder of these widths (first: the encoder's arrays BEFORE the LPCNet arrays; with_dec: the
    decoder of dred_model's set "mixed" -- latent 80, state 24 -- between them, where the reference's blobs have it after the encoder)"""
    m = synth.make_model()
    before = list(m.arrays)
    add_dred_enc(m, widths, **kw)
    if first:                            # (dict order is blob order)
        m.arrays = {k: m.arrays[k] for k in [k for k in m.arrays if k not in before] + before}
    if with_dec:
        dm.add_dred(m, dm.SETS["mixed"]["widths"], dm.SETS["mixed"]["latent_dim"])
    return synth.blob_bytes(m)


def set_blob(name, with_dec=False, first=False):
    s = SETS[name]
    return blob_enc(s["widths"], with_dec, first, taps=s["taps"], latent_dim=s["latent_dim"], gdense1=s["gdense1"], state_dim=s["state_dim"])


def inputs(n_streams=N_STREAMS, n_dframes=N_DFRAMES, seed=0xFEA7):
    """features [n][2 n_dframes][20] N(0, 1) with one double frame per stream scaled by 8 (enc_dense1's pre-activations pass the tanh table's last knot)
    and one all zero"""
    rng = np.random.default_rng([seed, n_streams, n_dframes])
    feat = rng.standard_normal((n_streams, 2 * n_dframes, 20)).astype(f32)
    for s in range(n_streams):
        d = s % n_dframes
        feat[s, 2 * d:2 * d + 2] *= f32(8)
        d = (s + 3) % n_dframes
        feat[s, 2 * d:2 * d + 2] = 0
    return feat


def long_inputs():
    return inputs(LONG_STREAMS, LONG_DFRAMES)


def strided(feat, stride, fill=777.0):
    """[n][rows][20] -> [n][rows][stride] with `fill` behind the 20 floats"""
    out = np.full(feat.shape[:2] + (stride,), fill, f32)
    out[:, :, :20] = feat
    return out


def rows_crc(lat, init, count):
    """CRC-32 per stream over its encoded rows: the latents' then the initial states'"""
    return np.array([zlib.crc32(np.ascontiguousarray(lat[s, :int(count[s])]).tobytes() + np.ascontiguousarray(init[s, :int(count[s])]).tobytes())
                     for s in range(lat.shape[0])], np.uint32)


def mem_crc(states, gru_floats):
    """CRC-32 per stream over the conv memory of its state vector (the part behind the GRU states)"""
    return np.array([zlib.crc32(np.ascontiguousarray(st[gru_floats:]).tobytes()) for st in states], np.uint32)


class DredEncNumpy:
    def __init__(self, blob, descending_conv=False):
        a = pm.blob_arrays(blob)
        g = lambda k, dt=f32: np.frombuffer(a[k], dt)
        self.widths = [g(n + "_bias").size if n in DENSE_NAMES else g(n + "_bias").size // 6 for n in ("enc_dense%d" % (k + 1) for k in range(8))]
        self.total = sum(self.widths)
        self.latent_dim = g("bits_dense_bias").size
        self.taps = g("bits_dense_weights").size // (self.total * self.latent_dim)
        self.gdense1 = g("gdense1_bias").size
        self.state_dim = g("gdense2_bias").size
        dense = lambda name, n_in: (g(name + "_weights").reshape(n_in, -1), g(name + "_bias"))
        self.layers, prev = [], IN_DIM
        for k in range(8):
            name = "enc_dense%d" % (k + 1)
            if k in DENSE_AT:
                self.layers.append(dense(name, prev))
            else:
                n = self.widths[k]
                self.layers.append(dict(N=n, bias=g(name + "_bias"), w=g(name + "_weights").reshape(-1, 4, 8), idx=g(name + "_weights_idx", np.int32),
                                        rec=g(name + "_recurrent_weights").reshape(n, 3 * n)))
            prev = self.widths[k]
        self.bits = dense("bits_dense", self.taps * self.total)
        self.g1 = dense("gdense1", self.total)
        self.g2 = dense("gdense2", self.gdense1)
        self.gru_floats = sum(self.widths[k] for k in GRU_AT)
        self.state_floats = self.gru_floats + (self.taps - 1) * self.total
        self.descending = descending_conv      # (the generator's order-sensitivity check: the window's sum from its last term down)

    def fresh(self):
        """DRED_rdovae_init_encoder: the state vector in the reference's member order, zero"""
        return np.zeros(self.state_floats, f32)

    def _split(self, st):
        o = np.concatenate([[0], np.cumsum([self.widths[k] for k in GRU_AT])]).astype(int)
        return [st[o[g]:o[g + 1]] for g in range(3)], st[self.gru_floats:]

    def encode_dframe(self, st, x40):
        """one double frame: the state vector `st` advances in place -> (latents, initial state)"""
        dn = pm.PlcNetNumpy._dense
        h, mem = self._split(st)
        x, buf = np.asarray(x40, f32), []
        for k in range(8):
            if k in DENSE_AT:
                x = pm.tanh_approx(dn(self.layers[k][0], self.layers[k][1], x))
            else:
                g = GRU_AT.index(k)
                h[g][:] = pm.PlcNetNumpy._gru(self.layers[k], h[g].copy(), x)
                x = h[g].copy()
            buf.append(x)
        buf = np.concatenate(buf)
        window = np.concatenate([mem, buf])      # compute_conv1d, src/nnet.c:452-470: [mem | input], oldest tap first
        if self.descending:
            lat = dn(self.bits[0][::-1], self.bits[1], window[::-1])
        else:
            lat = dn(self.bits[0], self.bits[1], window)
        mem[:] = window[self.total:]
        g1 = pm.tanh_approx(dn(self.g1[0], self.g1[1], buf))
        return lat, pm.tanh_approx(dn(self.g2[0], self.g2[1], g1))

    def enc1_preact(self, x40):
        return pm.PlcNetNumpy._dense(self.layers[0][0], self.layers[0][1], np.asarray(x40, f32))

    def encode(self, st, feat, count, first=0):
        """one stream: double frames first .. first + count - 1 of feat [2 n][>= 20] -> (latents [count][L], initial [count][S]); st advances"""
        lat, init = np.zeros((count, self.latent_dim), f32), np.zeros((count, self.state_dim), f32)
        for d in range(count):
            lat[d], init[d] = self.encode_dframe(st, np.concatenate([feat[2 * (first + d), :20], feat[2 * (first + d) + 1, :20]]))
        return lat, init

    def encode_all(self, feat, count, fill=0.0):
        """every stream from a fresh state: -> (latents [n][D][L], initial [n][D][S], final states [n][state_floats]); rows past count[s] hold `fill`"""
        n, D = feat.shape[0], feat.shape[1] // 2
        lat, init = np.full((n, D, self.latent_dim), fill, f32), np.full((n, D, self.state_dim), fill, f32)
        states = np.zeros((n, self.state_floats), f32)
        for s in range(n):
            c = int(count[s])
            lat[s, :c], init[s, :c] = self.encode(states[s], feat[s], c)
        return lat, init, states
