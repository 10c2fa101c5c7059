#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_i8_v1.npz from the compiled reference's generic-C int8 (DOT_PROD) build (oracle/_ref/liblpcnet_ref_gi.so,
`make -C oracle ref`), driven through ctypes: make_golden_dred.py's chain -- _lpcnet_compute_dense and compute_gruB on ctypes mirrors of the layer
structs, in the sequence of dred_rdovae_dec_init_states / dred_rdovae_decode_qframe / DRED_rdovae_decode_all -- on int8 blobs, whose GRULayer
mirrors point at the int8 weight arrays.  In that build the dense layers run on float weights and the three GRUs (dec_dense2 / 4 / 6) through
sparse_sgemv_accum8x4 / sgemv_accum8x4 of src/vec.h:274-339.

Width sets, inputs and counts are dred_model's; the blobs are dred_i8_model.blob_dec's.  The fixture holds results:

  feat_<set>   [9][28][20] float32 for the width sets w256, mixed and small (7 latents, count = dred_model.COUNT; rows past 4 count[s] are zero)
  long_crc     [16] CRC-32 of every stream's decoded rows of the long run at width 256 (26 latents, count = dred_model.LONG_COUNT),
  long_full    [104][20] stream 3 of it in full
  blob_crc_<set>, in_crc_<set>, long_in_crc: CRC-32 of the model blobs and of the inputs

    python tests/tools/make_golden_dred_i8.py [OUT.npz]
"""
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

REF_I8 = os.path.join(pm.ROOT, "oracle", "_ref", "liblpcnet_ref_gi.so")


def main():
    L = load_ref(REF_I8)
    res = {}
    for name in dm.SETS:
        blob = di.blob_dec(name)
        state, latents = dm.set_inputs(name)
        ref = RefDecoder(L, blob).decode_all(state, latents, dm.COUNT)
        mine = di.DredDecNumpyI8(blob).decode_all(state, latents, dm.COUNT)      # (asserts |x| <= 1 at every quantisation point)
        same = np.array_equal(mine.view(np.uint32), ref.view(np.uint32))
        print(name, "NumPy restatement equals the reference:", same, "| finite:", bool(np.isfinite(ref).all()), "| max abs", float(np.abs(ref).max()))
        assert same and np.isfinite(ref).all()
        # the fixture senses the int8 arithmetic: with the accumulator left unscaled, outputs change
        loose = di.DredDecNumpyI8(blob, unscaled=True).decode_all(state, latents, dm.COUNT)
        changed = int((loose.view(np.uint32) != ref.view(np.uint32)).sum())
        print(name, "outputs that an unscaled accumulator changes:", changed, "of", int(80 * dm.COUNT.sum()))
        assert changed > 0
        # the blob with the PLC network holds the same decoder
        assert pm.blob_arrays(di.blob_dec(name, with_plc=True))["dec_dense2_weights"] == pm.blob_arrays(blob)["dec_dense2_weights"]
        res["feat_" + name] = ref
        res["blob_crc_" + name] = np.uint32(zlib.crc32(blob))
        res["in_crc_" + name] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
    blob = di.blob_dec("w256")
    state, latents = dm.long_inputs()
    ref = RefDecoder(L, blob).decode_all(state, latents, dm.LONG_COUNT)
    assert np.isfinite(ref).all()
    s = dm.LONG_FULL_STREAM
    assert np.array_equal(di.DredDecNumpyI8(blob).decode(state[s], latents[s], int(dm.LONG_COUNT[s])).view(np.uint32), ref[s].view(np.uint32))
    res["long_crc"] = dm.stream_crc(ref, dm.LONG_COUNT)
    res["long_full"] = ref[s]
    res["long_in_crc"] = np.uint32(zlib.crc32(state.tobytes() + latents.tobytes()))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_i8_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 150 * 1024


if __name__ == "__main__":
    main()
