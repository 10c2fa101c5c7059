"""TEST TOOLING shared by tests/tools/make_golden_plc.py, tests/test_plc_host.py and tests/test_gpu_plc.py:
  * the inputs of the PLC fixture (tests/golden/golden_plc_v1.npz): streams, loss patterns, FEC schedules -- seeded, so the fixture
    stores results only;
  * PlcNetNumpy: a NumPy float32 restatement of compute_plc_pred (src/lpcnet_plc.c:135-146; _lpcnet_compute_dense src/nnet.c:122-135,
    compute_gruB :326-372, the float build's sparse_sgemv_accum8x4 src/vec.h:347-403 and sgemv_accum src/nnet.c:73-86) with every product
    and sum rounded to float32 in the reference's order; the fixture pins it to the reference at 128 / 16 / 16;
  * PlcControl: the integer control flow of lpcnet_plc_update_causal / lpcnet_plc_conceal_causal / lpcnet_plc_fec_add (src/lpcnet_plc.c:109-131,
    :188-340) restated from the reference, independent of the engine's planner, reduced to the summary lpcnet_hip_plc_plan reports.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpcnet_amd import synth  # noqa: E402
import plc_synth  # noqa: E402

f32 = np.float32
N_STREAMS, T = 64, 300
OPTION_SETS = (0, 2, 4, 6)          # CAUSAL, CODEC, CAUSAL | DC_FILTER, CODEC | DC_FILTER
FEC_STREAMS = 8                     # streams 0..7 of the FEC run carry schedules
BLOCK = 10                          # the fixture checks output in blocks of 10 frames: CRC-32 over the block's ten per-frame CRC-32 values
FULL_STREAM, FULL_FRAMES = 6, (70, 110)          # ... and holds these frames of this stream in full: the burst of 15 lost frames and the recovery
FEC_FULL_STREAM, FEC_FULL_FRAMES = 2, (145, 175) # ... and these of the FEC run: the full ring read down by a 20-frame loss


def block_crc(out):
    """out [n][T][160] int16, T a multiple of BLOCK -> [n][T / BLOCK] uint32: CRC-32 over the little-endian CRC-32 values of the block's frames"""
    import zlib
    n, t = out.shape[0], out.shape[1]
    assert t % BLOCK == 0
    fr = np.array([[zlib.crc32(np.ascontiguousarray(f).tobytes()) for f in s] for s in out], "<u4").reshape(n, t // BLOCK, BLOCK)
    return np.array([[zlib.crc32(np.ascontiguousarray(b).tobytes()) for b in s] for s in fr], np.uint32)


def stream_pcm(s, n_frames=T):
    return synth.make_pcm(500 + s, n_frames).reshape(n_frames, 160)


def loss_patterns(n=N_STREAMS, n_frames=T):
    """[n][n_frames] uint8: no loss, isolated losses, a loss in frame 0, losses one and two frames apart, bursts of 2, 5 and 15,
    alternating loss, then seeded random patterns of 3 .. 25 % loss with bursts"""
    L = np.zeros((n, n_frames), np.uint8)
    L[1, [20, 77, 140, 260]] = 1
    L[2, [0, 50]] = 1
    L[3, [30, 32, 90, 93, 150, 152, 154]] = 1
    L[4, [40, 41, 100, 101]] = 1
    L[5, 60:65] = 1
    L[6, 80:95] = 1
    L[6, 200:230] = 1
    L[7, 10:120:2] = 1
    L[8, 0:3] = 1
    L[9, [5, 7, 8, 10, 13]] = 1
    for s in range(10, n):
        rng = np.random.default_rng([s, 0x10C])
        p = rng.uniform(0.03, 0.25)
        t = 0
        while t < n_frames:
            if rng.uniform() < p:
                run = int(rng.choice([1, 1, 1, 2, 2, 3, 5, 12]))
                L[s, t:t + run] = 1
                t += run
            t += 1
    return L


def fec_schedule(n=N_STREAMS, n_frames=T):
    """per frame and stream the calls made BEFORE the step: ops [n_frames][n] (0 none, 1 add a vector, 2 add NULL, 3 clear, 4 add two vectors)
    and the vectors [n_frames][n][2][20]"""
    ops = np.zeros((n_frames, n), np.uint8)
    vec = np.zeros((n_frames, n, 2, 20), f32)
    rng = np.random.default_rng(0xFEC)
    for s in range(FEC_STREAMS):
        for t in range(n_frames):
            u = rng.uniform()
            if s == 0:
                ops[t, s] = 1
            elif s == 1:
                ops[t, s] = 1 if u < 0.6 else 2 if u < 0.8 else 0
            elif s == 2:
                ops[t, s] = 4 if t < 120 else 1          # fills the ring (100 vectors), then keeps adding
            elif s == 3:
                ops[t, s] = 3 if t % 50 == 49 else 1
            else:
                ops[t, s] = 1 if u < 0.5 else 2 if u < 0.6 else 4 if u < 0.7 else 3 if u < 0.72 else 0
            v = (rng.standard_normal((2, 20)) * 0.5).astype(f32)
            v[:, 0] -= f32(3.0)
            v[:, 18] = (rng.uniform(-0.6, 0.6, 2)).astype(f32)
            v[:, 19] = (rng.uniform(-0.4, 0.4, 2)).astype(f32)
            vec[t, s] = v
    return ops, vec


def fec_loss_patterns(n=N_STREAMS, n_frames=T):
    L = loss_patterns(n, n_frames)
    L[0] = 0
    L[0, 30:36] = 1
    L[0, 100:130:3] = 1
    L[2] = 0
    L[2, 150:170] = 1          # reads the full ring down
    L[2, 250:255] = 1
    return L


def blob_widths(d1, g1, g2, flavour="float", seed=777, block_density=None):
    """the LPCNet test model of `flavour` with a d1 / g1 / g2 PLC network in the same flavour; block_density as in plc_synth._gru (both GRUs)"""
    m = synth.make_model(flavour=flavour)
    rng = np.random.default_rng(seed)
    m.add("plc_dense1_weights", (rng.standard_normal((57, d1)) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", (rng.standard_normal(d1) * 0.05).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    plc_synth._gru(m, "plc_gru1", rng, d1, g1, flavour, block_density)
    plc_synth._gru(m, "plc_gru2", rng, g1, g2, flavour, block_density)
    m.add("plc_out_weights", (rng.standard_normal((g2, 20)) * 0.08).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_out_bias", (rng.standard_normal(20) * 0.2).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    return synth.blob_bytes(m)


def blob_256(seed=777):
    """the LPCNet test model with a 128 / 256 / 256 PLC network (the trained PLC model's GRU width, training_tf2/lpcnet_plc.py:65)"""
    return blob_widths(128, 256, 256, "float", seed)


def group_counts(idx, groups):
    """block counts per row group of an index stream {count, positions...}"""
    out, p = [], 0
    for _ in range(groups):
        out.append(int(idx[p]))
        p += 1 + out[-1]
    assert p == len(idx)
    return out


def blob_arrays(blob):
    """{name: (type, raw bytes)} of a DNNw blob (src/parse_lpcnet_weights.c:53-77)"""
    out, p = {}, 0
    while p < len(blob):
        size, block = int(np.frombuffer(blob, np.int32, 1, p + 12)[0]), int(np.frombuffer(blob, np.int32, 1, p + 16)[0])
        name = blob[p + 20:p + 64].split(b"\0")[0].decode()
        out[name] = blob[p + 64:p + 64 + size]
        p += 64 + block
    return out


_TANSIG = None


def _tansig():
    global _TANSIG
    if _TANSIG is None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_tables
        _TANSIG = gen_tables.tansig()
    return _TANSIG


def tanh_approx(x):
    """src/vec.h:82-99 on a float32 vector"""
    x = np.asarray(x, f32)
    tab = _tansig()
    sign = np.where(x < 0, f32(-1), f32(1)).astype(f32)
    ax = np.abs(x)
    i = np.minimum(200, np.floor(0.5 + 25.0 * ax.astype(np.float64)).astype(np.int64))          # (25*x is formed in float, then .5 + in double)
    i = np.minimum(200, np.floor(0.5 + (f32(25) * ax).astype(np.float64)).astype(np.int64))
    dx = ax - f32(0.04) * i.astype(f32)
    y = tab[i]
    dy = f32(1) - y * y
    y = y + dx * dy * (f32(1) - y * dx)
    return (sign * y).astype(f32)


def sigmoid_approx(x):
    return (f32(0.5) + f32(0.5) * tanh_approx(f32(0.5) * np.asarray(x, f32))).astype(f32)


class PlcNetNumpy:
    def __init__(self, blob):
        a = blob_arrays(blob)
        g = lambda k, dt=f32: np.frombuffer(a[k], dt)
        self.d1 = g("plc_dense1_bias").size
        self.g1 = g("plc_gru1_bias").size // 6
        self.g2 = g("plc_gru2_bias").size // 6
        self.dense1 = (g("plc_dense1_weights").reshape(57, self.d1), g("plc_dense1_bias"))
        self.out = (g("plc_out_weights").reshape(self.g2, 20), g("plc_out_bias"))
        self.gru = []
        for name, n_in, n in (("plc_gru1", self.d1, self.g1), ("plc_gru2", self.g1, self.g2)):
            self.gru.append(dict(N=n, bias=g(name + "_bias"), w=g(name + "_weights").reshape(-1, 4, 8), idx=g(name + "_weights_idx", np.int32),
                                 rec=g(name + "_recurrent_weights").reshape(n, 3 * n)))
        self.h1 = np.zeros(self.g1, f32)
        self.h2 = np.zeros(self.g2, f32)

    @staticmethod
    def _dense(w, b, x):
        acc = b.copy()
        for j in range(w.shape[0]):
            acc = (acc + w[j] * x[j]).astype(f32)
        return acc

    @staticmethod
    def _gru(G, state, x):
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
        for j in range(N):
            recur = (recur + G["rec"][j] * state[j]).astype(f32)
        zr = sigmoid_approx(zrh[:2 * N] + recur[:2 * N])
        z, r = zr[:N], zr[N:]
        h = tanh_approx(zrh[2 * N:] + recur[2 * N:] * r)
        return (z * state + (f32(1) - z) * h).astype(f32)

    def pred(self, x57):
        x = np.asarray(x57, f32)
        d = tanh_approx(self._dense(self.dense1[0], self.dense1[1], x))
        self.h1 = self._gru(self.gru[0], self.h1, d)
        self.h2 = self._gru(self.gru[1], self.h2, self.h1)
        out = self._dense(self.out[0], self.out[1], self.h2)
        v = f32(out[19] + f32(0.1))
        out[19] = f32(0.5) if f32(0.5) < v else v
        return out


class PlcControl:
    """the ints of one LPCNetPLCState (plus feature_buffer_fill of its LPCNetState) in causal mode"""

    def __init__(self, options):
        self.blending = (options & 3) == 0
        self.pcm_fill, self.skip_analysis, self.blend, self.loss_count = 400, 0, 0, 0
        self.fec_fill = self.fec_keep = self.fec_read = self.fec_skip = 0
        self.fbuf = 0

    def fec_add(self, is_null):
        if is_null:
            self.fec_skip += 1
            return
        if self.fec_fill == 100:
            if self.fec_keep == 0:
                return
            self.fec_fill -= self.fec_keep
            self.fec_read -= self.fec_keep
            self.fec_keep = 0
        self.fec_fill += 1

    def fec_clear(self):
        self.fec_fill = self.fec_keep = self.fec_read = self.fec_skip = 0

    def _deferred(self):
        if self.fbuf < 4:
            self.fbuf += 1

    def _fec_or_pred(self):
        if self.fec_read != self.fec_fill and self.fec_skip == 0:
            self.fec_read += 1
            self.fec_keep = max(0, max(self.fec_keep, self.fec_read - 3))
            return 1
        if self.fec_skip > 0:
            self.fec_skip -= 1
        return 0

    def step(self, lost):
        """-> the 10-int summary of lpcnet_hip_plc_plan"""
        sm = [0] * 10
        if lost:
            sm[0], sm[1] = 1, self.fbuf
            self.fbuf = 0
            while self.pcm_fill > 0:
                n = min(self.pcm_fill, 160)
                sm[4] += self._fec_or_pred()
                self.pcm_fill -= n
                self.skip_analysis += 1
                sm[2] += 1
                sm[3] += n
            if self._fec_or_pred():
                self.loss_count = 0
                sm[4] += 1
            else:
                self.loss_count += 1
            self.blend = 1
            sm[9] = self.loss_count
            return sm
        if self.skip_analysis:
            if self.blend:
                if self.blending:
                    self._deferred(); self._deferred()
                    sm[5], sm[8] = 1, 2
                else:
                    self.fec_read = max(self.fec_read - 2, self.fec_keep)
                    sm[5] = 2
                self.pcm_fill = 80
                sm[6] = 1
            else:
                self.pcm_fill += 160
                sm[6] = 2
        if not self.blend:
            if self.fec_skip:
                self.fec_skip -= 1
            elif self.fec_read < self.fec_fill:
                self.fec_read += 1
            self.fec_keep = max(0, max(self.fec_keep, self.fec_read - 3))
            sm[7] = 1
        if self.skip_analysis:
            if self.blending:
                self._deferred()
                sm[8] += 1
            self.skip_analysis -= 1
        else:
            self._deferred()
            sm[8] += 1
            sm[6] = 3
        self.loss_count = 0
        self.blend = 0
        return sm


def apply_fec_op(ctl, op):
    if op == 1:
        ctl.fec_add(False)
    elif op == 2:
        ctl.fec_add(True)
    elif op == 3:
        ctl.fec_clear()
    elif op == 4:
        ctl.fec_add(False); ctl.fec_add(False)


def burg_frames():
    """[8][160] int16-valued float32 frames: speech-like, silent, full-scale alternation, DC offset, a single pulse, low-level noise"""
    rng = np.random.default_rng(0xB0)
    sp = stream_pcm(3, 40)
    fr = [sp[5], sp[17], np.zeros(160), np.where(np.arange(160) % 2 == 0, 32767, -32768), np.full(160, 12000.0),
          np.where(np.arange(160) == 37, 30000.0, 0.0), rng.integers(-3, 4, 160), sp[33] // 4 + 9000]
    return np.stack([np.asarray(x, f32) for x in fr])


def pred_inputs(n_steps=40, seed=0x9ED):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_steps, 57)) * 1.5).astype(f32)
    x[::5] = 0
    x[:, 56] = rng.choice([-1.0, 0.0, 1.0], n_steps).astype(f32)
    return x
