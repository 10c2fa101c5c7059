#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_enc_fast_v1.npz: the yardstick of the DRED encoder's FAST flavour (lpcnet_batch_dred_enc_set_fast), by the protocol
of the decoder's (make_golden_dred_fast.py) -- FAST may deviate from the reference's generic-C float build (gf) no more than the reference's own
AVX2+FMA float build (af) does on the same inputs.  Both builds come from `make -C oracle ref` (oracle/_ref/liblpcnet_ref_gf.so, liblpcnet_ref_af.so)
and are driven by make_golden_dred_enc.RefEncoder: the same chain of layer functions on the seeded blobs and inputs of dred_enc_model.py, bits_dense
by the dense route that make_golden_dred_enc.py describes (compute_conv1d is never called with a window beyond 384 floats).

An envelope is taken per double-frame index d.  For the outputs it is the maximum of |af - gf| over the streams that encode double frame d; for the
final state of a stream -- which is the state behind its LAST double frame -- over the streams whose count is d + 1 (0 where there is none):

  env_lat_<set>, env_init_<set>, env_gru_<set>, env_mem_<set>   [7] for the width sets tf, w256 and narrow (dred_enc_model.inputs(), COUNT): latents,
                   initial states, final GRU states, final conv memory.  The gf values are golden_dred_enc_v1.npz's (lat_, init_, gru_, mem_full_:
                   the conv memory of stream 0); mem_gf_narrow [9][244] adds every stream's conv memory at the narrow set
  tile_lat, tile_init, tile_gru, tile_env_lat, tile_env_init, tile_env_gru: the tiling case on `narrow` -- 69 streams (64 + 5), 7 double frames,
                   the counts of make_golden_dred_fast.tile_counts() (0, 1 and 7 in every group of 16)
  long_env_lat, long_env_init [26], long_env_gru, long_env_mem [26]: the long run at `tf` (16 x 26, LONG_COUNT), the envelope over all 16 streams;
                   long_lat, long_init [4][26][..], long_gru [4][384]: gf in full for LONG_GF_STREAMS (golden_dred_enc_v1.npz holds stream 3 alone)
  restated_worst_<case>: the worst ratio |restatement - gf| / envelope of FastEncNumpy below on that case (asserted <= 0.25 here)
  blob_crc_<set>, in_crc, tile_in_crc, long_in_crc: CRC-32 of the blobs and inputs

FastEncNumpy is the FAST definition restated in NumPy: every sum one fma chain from its bias in ascending input order (an fma
through float64), exp / reciprocal activations on libm's exp2.  The generator asserts that it stays within a quarter of the envelope everywhere: a
condition on the inputs (the decoder's kernel measured 0.025), not a knob.

    python tests/tools/make_golden_dred_enc_fast.py [OUT.npz]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dred_enc_model as em  # noqa: E402
import make_golden_dred_fast as mf  # noqa: E402
import plc_model as pm  # noqa: E402

f32, f64 = np.float32, np.float64
TILE_STREAMS, TILE_SET = mf.TILE_STREAMS, "narrow"
LONG_GF_STREAMS = (3, 0, 2, 12)          # counts 26, 26, 13, 7
RESTATED_CAP = 0.25


def tile_inputs():
    return em.inputs(TILE_STREAMS, em.N_DFRAMES, seed=0x7115)


def tile_counts():
    assert em.N_DFRAMES == 7
    return mf.tile_counts()


def fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def fast_sigmoid(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return (f32(1) / (f32(1) + np.exp2(f32(-1.44269504) * np.asarray(x, f32)))).astype(f32)


def fast_tanh(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return (f32(1) - f32(2) * (f32(1) / (f32(1) + np.exp2(f32(2.88539008) * np.asarray(x, f32))))).astype(f32)


def chain(w, acc, x):
    """acc [n][rows] goes on over the inputs x [n][K] of the matrix w [K][rows], ascending"""
    for j in range(w.shape[0]):
        acc = fma(w[j][None, :], x[:, j:j + 1], acc)
    return acc


class FastEncNumpy:
    """the encoder's FAST arithmetic on the arrays dred_enc_model.DredEncNumpy parses; every stream of a call side by side"""

    def __init__(self, blob):
        self.net = em.DredEncNumpy(blob)

    def _gru(self, G, h, x):
        N, n = G["N"], x.shape[0]
        inp = np.repeat(G["bias"][None, :3 * N], n, 0).astype(f32)
        idx, p, blk = G["idx"], 0, 0
        for grp in range(3 * N // 8):
            cnt = int(idx[p]); p += 1
            y = inp[:, grp * 8:grp * 8 + 8]
            for _ in range(cnt):
                pos = int(idx[p]); p += 1
                for k in range(4):
                    y = fma(G["w"][blk, k][None, :], x[:, pos + k:pos + k + 1], y)
                blk += 1
            inp[:, grp * 8:grp * 8 + 8] = y
        rec = chain(G["rec"], np.repeat(G["bias"][None, 3 * N:], n, 0).astype(f32), h)
        z = fast_sigmoid(inp[:, :N] + rec[:, :N])
        r = fast_sigmoid(inp[:, N:2 * N] + rec[:, N:2 * N])
        c = fast_tanh(fma(rec[:, 2 * N:], r, inp[:, 2 * N:]))
        return fma(z, h, (f32(1) - z) * c)

    def encode_dframe(self, st, x40):
        """st [n][state_floats] (the reference's member order) advances in place; x40 [n][40] -> (latents [n][L], initial [n][S])"""
        net, n = self.net, st.shape[0]
        o = np.concatenate([[0], np.cumsum([net.widths[k] for k in em.GRU_AT])]).astype(int)
        rep = lambda b: np.repeat(b[None, :], n, 0).astype(f32)
        x, buf = np.asarray(x40, f32), []
        for k in range(8):
            if k in em.DENSE_AT:
                x = fast_tanh(chain(net.layers[k][0], rep(net.layers[k][1]), x))
            else:
                g = em.GRU_AT.index(k)
                x = self._gru(net.layers[k], st[:, o[g]:o[g + 1]].copy(), x)
                st[:, o[g]:o[g + 1]] = x
            buf.append(x)
        buf = np.concatenate(buf, 1)
        window = np.concatenate([st[:, net.gru_floats:], buf], 1)
        lat = chain(net.bits[0], rep(net.bits[1]), window)
        st[:, net.gru_floats:] = window[:, net.total:]
        g1 = fast_tanh(chain(net.g1[0], rep(net.g1[1]), buf))
        return lat, fast_tanh(chain(net.g2[0], rep(net.g2[1]), g1))

    def encode_all(self, feat, count, states=None, first=0):
        """as DredEncNumpy.encode_all (rows past count[s] zero); `states` given: they go on, from double frame `first` of feat"""
        count = np.asarray(count)
        n, D = feat.shape[0], feat.shape[1] // 2
        lat, init = np.zeros((n, D, self.net.latent_dim), f32), np.zeros((n, D, self.net.state_dim), f32)
        states = np.zeros((n, self.net.state_floats), f32) if states is None else states
        for d in range(int(count.max(initial=0))):
            live = np.nonzero(count > d)[0]
            st = states[live]
            lat[live, d], init[live, d] = self.encode_dframe(st, feat[live, 2 * (first + d):2 * (first + d) + 2, :20].reshape(len(live), 40))
            states[live] = st
        return lat, init, states


def envelopes(af, gf, count, gru_floats):
    """(lat, init, gru, mem) envelopes [D] between two (latents, initial, states) triples"""
    count = np.asarray(count)
    D = af[0].shape[1]
    env = np.zeros((4, D), f64)
    dif = lambda a, b: np.abs(a.astype(f64) - b.astype(f64)).max()
    for d in range(D):
        live, last = count > d, count == d + 1
        if live.any():
            env[0, d], env[1, d] = dif(af[0][live, d], gf[0][live, d]), dif(af[1][live, d], gf[1][live, d])
        if last.any():
            env[2, d], env[3, d] = dif(af[2][last, :gru_floats], gf[2][last, :gru_floats]), dif(af[2][last, gru_floats:], gf[2][last, gru_floats:])
    return env.astype(f32)


def worst_ratio(got, gf, env, count, gru_floats, streams=None, what="", kinds=(0, 1, 2, 3)):
    """max over kinds and double-frame indices of (max |got - gf| over the streams of the index) / envelope; every deviation printed before it is
    judged by the caller.  `streams`: the streams gf holds (rows of gf in that order), all without it.  A deviation where the envelope is 0 counts as inf"""
    count = np.asarray(count)
    streams = np.arange(len(count)) if streams is None else np.asarray(streams)
    worst = 0.0
    names = ("latents", "initial", "gru", "mem")
    for d in range(env.shape[1]):
        for kind in kinds:
            sel = np.nonzero((count[streams] > d) if kind < 2 else (count[streams] == d + 1))[0]
            if not len(sel):
                continue
            if kind < 2:
                a, b = got[kind][streams[sel], d], gf[kind][sel, d]
            elif kind == 2:
                a, b = got[2][streams[sel], :gru_floats], gf[2][sel, :gru_floats]
            else:
                a, b = got[2][streams[sel], gru_floats:], gf[2][sel, gru_floats:]
            dev = float(np.abs(a.astype(f64) - b.astype(f64)).max())
            e = float(env[kind, d])
            print("%s %s double frame %d: deviation %.3g envelope %.3g" % (what, names[kind], d, dev, e))
            ratio = dev / e if e > 0 else (0.0 if dev == 0 else float("inf"))
            worst = max(worst, ratio if np.isfinite(dev) else float("inf"))
    return worst


def main():
    import make_golden_dred_enc as mg
    ref = os.path.join(pm.ROOT, "oracle", "_ref")
    gf_lib, af_lib = mg.load_ref(os.path.join(ref, "liblpcnet_ref_gf.so")), mg.load_ref(os.path.join(ref, "liblpcnet_ref_af.so"))
    old = np.load(os.path.join(pm.ROOT, "tests", "golden", "golden_dred_enc_v1.npz"))
    res = {}

    def both(blob, feat, count):
        gf = mg.RefEncoder(gf_lib, blob).encode_all(feat, count)
        af = mg.RefEncoder(af_lib, blob).encode_all(feat, count)
        assert all(np.isfinite(x).all() for x in gf + af)
        return gf, af

    def check(case, blob, feat, count, gf, env, gruf):
        count = np.asarray(count)
        for d in range(env.shape[1]):            # every envelope entry over live streams is > 0
            assert (env[:2, d] > 0).all() == bool((count > d).any()) and (env[2:, d] > 0).all() == bool((count == d + 1).any()), (case, d, env[:, d])
        worst = worst_ratio(FastEncNumpy(blob).encode_all(feat, count), gf, env, count, gruf, what=case + " restated")
        print(case, "restatement worst deviation / envelope %.4f" % worst)
        assert worst <= RESTATED_CAP, (case, worst)
        res["restated_worst_" + case] = f32(worst)

    feat = em.inputs()
    res["in_crc"] = np.uint32(zlib.crc32(feat.tobytes()))
    for name in em.SETS:
        blob = em.set_blob(name)
        gruf = em.DredEncNumpy(blob).gru_floats
        gf, af = both(blob, feat, em.COUNT)
        assert mg.same(gf[0], old["lat_" + name]) and mg.same(gf[1], old["init_" + name]) and mg.same(gf[2][:, :gruf], old["gru_" + name]) and \
            mg.same(gf[2][0, gruf:], old["mem_full_" + name]), name
        env = envelopes(af, gf, em.COUNT, gruf)
        for k, kind in enumerate(("lat", "init", "gru", "mem")):
            res["env_%s_%s" % (kind, name)] = env[k]
        res["blob_crc_" + name] = np.uint32(zlib.crc32(blob))
        if name == "narrow":
            res["mem_gf_narrow"] = gf[2][:, gruf:].copy()
        print(name, "env", env)
        check(name, blob, feat, em.COUNT, gf, env, gruf)
    # the tiling case
    blob = em.set_blob(TILE_SET)
    gruf = em.DredEncNumpy(blob).gru_floats
    feat, count = tile_inputs(), tile_counts()
    assert {0, 1, em.N_DFRAMES} <= set(count.tolist())
    for T in (16, 32):
        for t0 in range(0, TILE_STREAMS, T):
            assert len(set(count[t0:t0 + T].tolist())) > 1, (T, t0)
    gf, af = both(blob, feat, count)
    env = envelopes(af, gf, count, gruf)
    res["tile_lat"], res["tile_init"], res["tile_gru"] = gf[0], gf[1], gf[2][:, :gruf].copy()
    res["tile_env_lat"], res["tile_env_init"], res["tile_env_gru"] = env[0], env[1], env[2]
    res["tile_in_crc"] = np.uint32(zlib.crc32(feat.tobytes() + count.tobytes()))
    check("tile", blob, feat, count, gf, env, gruf)
    # the long run
    blob = em.set_blob("tf")
    gruf = em.DredEncNumpy(blob).gru_floats
    feat = em.long_inputs()
    gf, af = both(blob, feat, em.LONG_COUNT)
    assert mg.same(gf[0][em.LONG_FULL_STREAM], old["long_lat"]) and mg.same(gf[1][em.LONG_FULL_STREAM], old["long_init"])
    assert np.array_equal(em.rows_crc(gf[0], gf[1], em.LONG_COUNT), old["long_crc"])
    env = envelopes(af, gf, em.LONG_COUNT, gruf)
    for k, kind in enumerate(("lat", "init", "gru", "mem")):
        res["long_env_" + kind] = env[k]
    pick = list(LONG_GF_STREAMS)
    res["long_lat"], res["long_init"], res["long_gru"] = gf[0][pick], gf[1][pick], gf[2][pick, :gruf].copy()
    res["long_in_crc"] = np.uint32(zlib.crc32(feat.tobytes()))
    check("long", blob, feat, em.LONG_COUNT, gf, env, gruf)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_enc_fast_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 333 * 1024


if __name__ == "__main__":
    main()
