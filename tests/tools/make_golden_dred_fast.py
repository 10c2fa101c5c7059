#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_fast_v1.npz: the yardstick of the DRED decoder's FAST flavour (lpcnet_batch_dred_set_fast), by the protocol
tests/golden/simd_envelope_v1.json set for the sample kernel -- FAST may deviate from the reference's generic-C float build (gf) no more than the
reference's own AVX2+FMA float build (af) does on the same inputs.  Both builds come from `make -C oracle ref` (oracle/_ref/liblpcnet_ref_gf.so,
liblpcnet_ref_af.so) and are driven by make_golden_dred.RefDecoder: the same chain of layer functions on the same seeded blobs and inputs.

  env_<set>   [7]  for the width sets w256, mixed and small on the inputs of golden_dred_v1.npz (dred_model.set_inputs, dred_model.COUNT): per latent
                   index the maximum over the streams that decode it and their 80 outputs of |af - gf| (the gf values are feat_<set> of that fixture)
  tile_gf     [69][28][20], tile_env [7]: the tiling case on the `small` set -- 69 streams (64 + 5: whole tiles and a remainder at 16, 32 and 64
                   streams per tile), 7 latents, seeded counts (tile_counts()) that hold 0, 1 and 7 and differ inside every tile
  long_gf     [16][104][20], long_env [26]: the long run (dred_model.long_inputs, dred_model.LONG_COUNT) at width 256
  blob_crc_<set>, in_crc_<set>, tile_in_crc, long_in_crc: CRC-32 of the blobs and inputs

    python tests/tools/make_golden_dred_fast.py [OUT.npz]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dred_model as dm  # noqa: E402
import plc_model as pm  # noqa: E402

f32 = np.float32
TILE_STREAMS, TILE_SET = 69, "small"


def tile_inputs():
    return dm.inputs(dm.SETS[TILE_SET]["latent_dim"], TILE_STREAMS, dm.N_LATENTS, seed=0x7115)


def tile_counts():
    """seeded counts 0 .. 7 for the 69 streams; 0, 1 and 7 stand in every group of 16 streams, so they differ inside every tile of 16, 32 or 64"""
    rng = np.random.default_rng(0xC0C7)
    c = rng.integers(0, dm.N_LATENTS + 1, TILE_STREAMS).astype(np.int32)
    for t0 in range(0, TILE_STREAMS, 16):
        c[t0], c[t0 + 1], c[t0 + 2] = 0, 1, dm.N_LATENTS
    c[3], c[40], c[68] = dm.N_LATENTS, 5, dm.N_LATENTS          # (the streams the independence test decodes alone all decode something)
    return c


def envelope(af, gf, count, n_latents):
    """per latent index: max |af - gf| over the streams that decode that latent"""
    env = np.zeros(n_latents, np.float64)
    for l in range(n_latents):
        live = np.asarray(count) > l
        if live.any():
            env[l] = np.abs(af[live, 4 * l:4 * l + 4].astype(np.float64) - gf[live, 4 * l:4 * l + 4].astype(np.float64)).max()
    return env.astype(f32)


def main():
    import make_golden_dred as mg
    ref = os.path.join(pm.ROOT, "oracle", "_ref")
    gf_lib, af_lib = mg.load_ref(os.path.join(ref, "liblpcnet_ref_gf.so")), mg.load_ref(os.path.join(ref, "liblpcnet_ref_af.so"))
    old = np.load(os.path.join(pm.ROOT, "tests", "golden", "golden_dred_v1.npz"))
    res = {}

    def both(blob, state, latents, count):
        gf = mg.RefDecoder(gf_lib, blob).decode_all(state, latents, count)
        af = mg.RefDecoder(af_lib, blob).decode_all(state, latents, count)
        assert np.isfinite(gf).all() and np.isfinite(af).all()
        return gf, af

    for name in dm.SETS:
        blob = dm.set_blob(name)
        state, latents = dm.set_inputs(name)
        gf, af = both(blob, state, latents, dm.COUNT)
        assert np.array_equal(gf.view(np.uint32), old["feat_" + name].view(np.uint32)), name
        res["env_" + name] = envelope(af, gf, dm.COUNT, dm.N_LATENTS)
        res["blob_crc_" + name] = np.uint32(zlib.crc32(blob))
        res["in_crc_" + name] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
        print(name, "env", res["env_" + name], "rms", float(np.sqrt((gf.astype(np.float64) ** 2).mean())))
    blob = dm.set_blob(TILE_SET)
    state, latents = tile_inputs()
    count = tile_counts()
    assert {0, 1, dm.N_LATENTS} <= set(count.tolist())
    for T in (16, 32, 64):
        for t0 in range(0, TILE_STREAMS, T):
            assert len(set(count[t0:t0 + T].tolist())) > 1 or t0 + 1 >= TILE_STREAMS, (T, t0)
    gf, af = both(blob, state, latents, count)
    res["tile_gf"], res["tile_env"] = gf, envelope(af, gf, count, dm.N_LATENTS)
    res["tile_in_crc"] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes() + count.tobytes()))
    print("tile env", res["tile_env"])
    blob = dm.set_blob("w256")
    state, latents = dm.long_inputs()
    gf, af = both(blob, state, latents, dm.LONG_COUNT)
    assert np.array_equal(gf[dm.LONG_FULL_STREAM].view(np.uint32), old["long_full"].view(np.uint32))
    res["long_gf"], res["long_env"] = gf, envelope(af, gf, dm.LONG_COUNT, dm.LONG_LATENTS)
    res["long_in_crc"] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
    print("long env", res["long_env"])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_fast_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 333 * 1024


if __name__ == "__main__":
    main()
