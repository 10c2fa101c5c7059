"""TEST TOOLING shared by tests/tools/make_golden_plc_i8.py, tests/test_plc_i8_host.py and tests/test_gpu_plc_i8.py: the int8 (DOT_PROD) PLC network.
  * PlcNetNumpyI8: a NumPy restatement of compute_plc_pred (src/lpcnet_plc.c:135-146) as the reference's generic-C int8 build runs it: the dense
    layers in float (plc_model.PlcNetNumpy._dense), the GRUs through sparse_sgemv_accum8x4 / sgemv_accum8x4 of src/vec.h:274-339 with USE_SU_BIAS
    undefined -- start from `bias`; out *= 128*127; the inputs of a product quantised once, (signed char)(int)floor(.5 + 127 x) with the product in
    float and the sum in double; per 8x4 block, in list order, the exact integer sum of the four products added with one rounded float32 add;
    out *= 1/128/127 -- float32 at every rounding point.  The fixture (tests/golden/golden_plc_i8_v1.npz) pins it to the reference at 128 / 16 / 16;
  * blob_256_i8: the int8 counterpart of plc_model.blob_256 (widths 128 / 256 / 256); blob_wide_i8: widths 128 / 512 / 264, beyond the 256 lanes of
    the kernel's workgroup; model_with_plc: an LPCNet model of one flavour with a small PLC network of another (or the same);
  * blob_sparse_i8: a 128 / 16 / 16 int8 blob whose GRU 1 input matrix misses whole 8x4 blocks (a row group without any, one with a single block);
  * pred_traces: several streams' input traces through either restatement, one process per stream (the widest networks take ~0.6 s per step).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plc_model as pm  # noqa: E402
import plc_synth  # noqa: E402
from lpcnet_amd import synth  # noqa: E402

f32 = np.float32
SCALE = f32(128) * f32(127)
SCALE_1 = f32(1) / f32(128) / f32(127)


def quant_s8(x):
    """src/vec.h:280, :311 on a float32 vector -> int32 values of the signed chars"""
    t = (f32(127) * np.asarray(x, f32)).astype(f32)
    q = np.floor(0.5 + t.astype(np.float64)).astype(np.int64)
    return (((q + 128) & 0xFF) - 128).astype(np.int32)


def add_gru_i8(m, name, rng, n_in, n, block_mask=None):
    """plc_synth._gru's int8 arrays; block_mask [n_in / 4][3 n / 8] (optional): input-weight blocks to keep -- the others leave the index lists"""
    W, Q = synth._quantize_matrix((rng.standard_normal((n_in, 3 * n)) * 0.08).astype(f32))
    if block_mask is not None:
        keep = np.repeat(np.repeat(np.asarray(block_mask, bool), 4, axis=0), 8, axis=1)
        W, Q = W * keep, Q * keep
    _, Wq, idx = synth._sparse_blocks(W, Q)
    m.add(name + "_weights", Wq, synth.WEIGHT_TYPE_QWEIGHT)
    m.add(name + "_weights_idx", idx, synth.WEIGHT_TYPE_INT)
    _, Qr = synth._quantize_matrix((rng.standard_normal((n, 3 * n)) * 0.2).astype(f32))
    m.add(name + "_recurrent_weights", Qr.reshape(n // 4, 4, 3 * n // 8, 8).transpose(2, 0, 3, 1).astype(np.int8), synth.WEIGHT_TYPE_QWEIGHT)
    bias = (rng.standard_normal((2, 3 * n)) * 0.1).astype(f32)
    sub = bias.copy()
    sub[0] -= (Q * (1.0 / 128.0)).sum(axis=0).astype(f32)
    sub[1] -= (Qr * (1.0 / 128.0)).sum(axis=0).astype(f32)
    m.add(name + "_bias", bias, synth.WEIGHT_TYPE_FLOAT)
    m.add(name + "_subias", sub.astype(f32), synth.WEIGHT_TYPE_FLOAT)


def _add_out(m, rng, g2):
    m.add("plc_out_weights", (rng.standard_normal((g2, 20)) * 0.08).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_out_bias", (rng.standard_normal(20) * 0.2).astype(f32), synth.WEIGHT_TYPE_FLOAT)


def blob_256_i8(seed=777):
    """the int8 LPCNet test model with a 128 / 256 / 256 int8 PLC network (plc_model.blob_256's widths)"""
    m = synth.make_model(flavour="int8")
    rng = np.random.default_rng(seed)
    m.add("plc_dense1_weights", (rng.standard_normal((57, 128)) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", (rng.standard_normal(128) * 0.05).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    add_gru_i8(m, "plc_gru1", rng, 128, 256)
    add_gru_i8(m, "plc_gru2", rng, 256, 256)
    _add_out(m, rng, 256)
    return synth.blob_bytes(m)


def blob_wide_i8(seed=778):
    """128 / 512 / 264: GRU 1 at the loader's limit (two units per lane of the kernel's 256, 128 packed dwords into GRU 2), GRU 2 with eight units
    in the second pass, and g1 != g2"""
    m = synth.make_model(flavour="int8")
    rng = np.random.default_rng(seed)
    m.add("plc_dense1_weights", (rng.standard_normal((57, 128)) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", (rng.standard_normal(128) * 0.05).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    add_gru_i8(m, "plc_gru1", rng, 128, 512)
    add_gru_i8(m, "plc_gru2", rng, 512, 264)
    _add_out(m, rng, 264)
    return synth.blob_bytes(m)


def model_with_plc(flavour, plc_flavour, block_mask=None):
    """an LPCNet test model of `flavour` with a 128 / 16 / 16 PLC network whose GRU arrays are `plc_flavour` ("float" / "int8"); block_mask as in
    add_gru_i8 (int8 only), for GRU 1"""
    m = synth.make_model(flavour=flavour)
    rng = np.random.default_rng(1)
    m.add("plc_dense1_weights", (rng.standard_normal((57, 128)) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", np.zeros(128, f32), synth.WEIGHT_TYPE_FLOAT)
    if plc_flavour == "int8":
        add_gru_i8(m, "plc_gru1", rng, 128, 16, block_mask)
        add_gru_i8(m, "plc_gru2", rng, 16, 16)
    else:
        plc_synth._gru(m, "plc_gru1", rng, 128, 16, "float")
        plc_synth._gru(m, "plc_gru2", rng, 16, 16, "float")
    m.add("plc_out_weights", np.zeros((16, 20), f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_out_bias", np.zeros(20, f32), synth.WEIGHT_TYPE_FLOAT)
    return m


def sparse_mask(seed=99):
    """[32][6] blocks of a 128 -> 3 x 16 input matrix: row group 0 keeps none, row group 1 one, the others an irregular 20 .. 80 %"""
    rng = np.random.default_rng(seed)
    mask = np.zeros((32, 6), bool)
    mask[17, 1] = True
    for g, p in zip(range(2, 6), (0.2, 0.5, 0.8, 0.35)):
        mask[:, g] = rng.uniform(size=32) < p
    return mask


def blob_sparse_i8(seed=555):
    m = synth.make_model(flavour="int8")
    rng = np.random.default_rng(seed)
    m.add("plc_dense1_weights", (rng.standard_normal((57, 128)) * 0.1).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    m.add("plc_dense1_bias", (rng.standard_normal(128) * 0.05).astype(f32), synth.WEIGHT_TYPE_FLOAT)
    add_gru_i8(m, "plc_gru1", rng, 128, 16, sparse_mask())
    add_gru_i8(m, "plc_gru2", rng, 16, 16)
    _add_out(m, rng, 16)
    return synth.blob_bytes(m)


group_counts = pm.group_counts


class PlcNetNumpyI8:
    def __init__(self, blob):
        a = pm.blob_arrays(blob)
        g = lambda k, dt=f32: np.frombuffer(a[k], dt)
        self.d1 = g("plc_dense1_bias").size
        self.g1 = g("plc_gru1_bias").size // 6
        self.g2 = g("plc_gru2_bias").size // 6
        self.dense1 = (g("plc_dense1_weights").reshape(57, self.d1), g("plc_dense1_bias"))
        self.out = (g("plc_out_weights").reshape(self.g2, 20), g("plc_out_bias"))
        self.gru = []
        for name, n_in, n in (("plc_gru1", self.d1, self.g1), ("plc_gru2", self.g1, self.g2)):
            self.gru.append(dict(N=n, bias=g(name + "_bias"), w=g(name + "_weights", np.int8).reshape(-1, 8, 4).astype(np.int32),
                                 idx=g(name + "_weights_idx", np.int32),
                                 rec=g(name + "_recurrent_weights", np.int8).reshape(3 * n // 8, n // 4, 8, 4).astype(np.int32)))
        self.h1 = np.zeros(self.g1, f32)
        self.h2 = np.zeros(self.g2, f32)

    @staticmethod
    def _gru(G, state, x):
        N = G["N"]
        xq, sq = quant_s8(x), quant_s8(state)
        zrh = ((G["bias"][:3 * N] + f32(0)).astype(f32) * SCALE).astype(f32)
        idx, p, blk = G["idx"], 0, 0
        for grp in range(3 * N // 8):
            cnt = int(idx[p]); p += 1
            y = zrh[grp * 8:grp * 8 + 8]
            for _ in range(cnt):
                pos = int(idx[p]); p += 1
                y = (y + (G["w"][blk] @ xq[pos:pos + 4]).astype(f32)).astype(f32)          # [8][4] . [4]: exact, then one float add per row
                blk += 1
            zrh[grp * 8:grp * 8 + 8] = y
        zrh = (zrh * SCALE_1).astype(f32)
        recur = (G["bias"][3 * N:] * SCALE).astype(f32)
        for j in range(N // 4):
            recur = (recur + (G["rec"][:, j] @ sq[4 * j:4 * j + 4]).reshape(3 * N).astype(f32)).astype(f32)
        recur = (recur * SCALE_1).astype(f32)
        zr = pm.sigmoid_approx(zrh[:2 * N] + recur[:2 * N])
        z, r = zr[:N], zr[N:]
        h = pm.tanh_approx(zrh[2 * N:] + recur[2 * N:] * r)
        return (z * state + (f32(1) - z) * h).astype(f32)

    def pred(self, x57):
        x = np.asarray(x57, f32)
        d = pm.tanh_approx(pm.PlcNetNumpy._dense(self.dense1[0], self.dense1[1], x))
        self.h1 = self._gru(self.gru[0], self.h1, d)
        self.h2 = self._gru(self.gru[1], self.h2, self.h1)
        out = pm.PlcNetNumpy._dense(self.out[0], self.out[1], self.h2)
        v = f32(out[19] + f32(0.1))
        out[19] = f32(0.5) if f32(0.5) < v else v
        return out


def _trace_worker(args):
    blob, int8, xs = args
    net = (PlcNetNumpyI8 if int8 else pm.PlcNetNumpy)(blob)
    return np.stack([net.pred(x) for x in xs])


def pred_traces(blob, int8, xs):
    """xs [n][steps][57]: every stream's own input trace through a fresh restatement of the blob's PLC network (float or int8) -> [n][steps][20].
    The streams run in a pool of processes (spawned, so a parent that already initialised HIP is not forked), one each"""
    import multiprocessing as mp
    jobs = [(blob, int8, np.ascontiguousarray(x)) for x in xs]
    if len(jobs) == 1:
        return np.stack([_trace_worker(jobs[0])])
    with mp.get_context("spawn").Pool(min(len(jobs), 8)) as pool:
        return np.stack(pool.map(_trace_worker, jobs))
