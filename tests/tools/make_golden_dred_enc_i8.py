#!/usr/bin/env python3
"""Generate tests/golden/golden_dred_enc_i8_v1.npz from the compiled reference's generic-C int8 (DOT_PROD) build (oracle/_ref/liblpcnet_ref_gi.so,
`make -C oracle ref`), driven through ctypes: make_golden_dred_enc.py's chain (RefEncoder: dred_rdovae_encode_dframe, src/dred_rdovae_enc.c:38-95) on
int8 blobs.  In that build the dense layers and the conv1d bits_dense run on float weights and the three GRUs (enc_dense2 / 4 / 6) through
sparse_sgemv_accum8x4 / sgemv_accum8x4 of src/vec.h:274-339.  bits_dense is pinned as there: the window's sum comes from the reference's
_lpcnet_compute_dense at every width set, and compute_conv1d itself runs at `narrow` alone, whose window fits its 384-float stack buffer, where both
must agree in all bits.

Width sets, inputs and counts are dred_enc_model's; the blobs are dred_i8_model.blob_enc's.  The fixture holds results, under make_golden_dred_enc.py's
names:

  lat_<set>, init_<set>, gru_<set>, mem_crc_<set>, mem_full_<set>     for the width sets tf, w256 and narrow (count = dred_enc_model.COUNT)
  long_crc, long_lat, long_init, long_gru_crc, long_mem_crc           the long run at `tf` (26 double frames, LONG_COUNT; stream 3 in full)
  rt_feat      [2][28][20]: the reference's int8 DECODE of its own encoder output for streams 0 and 4 on dred_i8_model.blob_enc("tf", with_dec=True)
  blob_crc_<set>, blob_crc_rt, in_crc, long_in_crc: CRC-32 of the model blobs and of the inputs

    python tests/tools/make_golden_dred_enc_i8.py [OUT.npz]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dred_enc_model as em  # noqa: E402
import dred_i8_model as di  # noqa: E402
import plc_model as pm  # noqa: E402
from make_golden_dred import RefDecoder  # noqa: E402
from make_golden_dred_enc import RefEncoder, load_ref, same  # noqa: E402
from make_golden_dred_i8 import REF_I8  # noqa: E402

f32 = np.float32


def main():
    L = load_ref(REF_I8)
    res = {}
    feat = em.inputs()
    res["in_crc"] = np.uint32(zlib.crc32(feat.tobytes()))
    for name in em.SETS:
        blob = di.blob_enc(name)
        ref = RefEncoder(L, blob)
        lat, init, states = ref.encode_all(feat, em.COUNT)
        m_lat, m_init, m_states = di.DredEncNumpyI8(blob).encode_all(feat, em.COUNT)      # (asserts |x| <= 1 at every quantisation point)
        ok = same(m_lat, lat) and same(m_init, init) and same(m_states, states)
        finite = bool(np.isfinite(lat).all() and np.isfinite(init).all() and np.isfinite(states).all())
        print(name, "NumPy restatement equals the reference:", ok, "| finite:", finite, "| max abs latent", float(np.abs(lat).max()),
              "| double frames where compute_conv1d itself ran and agreed:", ref.conv_checked)
        assert ok and finite
        assert (ref.conv_checked == int(em.COUNT.sum())) == (name == "narrow")
        # the fixture senses the int8 arithmetic: with the accumulator left unscaled, outputs change
        l_lat, l_init, _ = di.DredEncNumpyI8(blob, unscaled=True).encode_all(feat, em.COUNT)
        changed = int((l_lat.view(np.uint32) != lat.view(np.uint32)).sum()) + int((l_init.view(np.uint32) != init.view(np.uint32)).sum())
        print(name, "latents and initial-state values that an unscaled accumulator changes:", changed, "of", int((ref.latent_dim + ref.state_dim) * em.COUNT.sum()))
        assert changed > 0
        res["lat_" + name], res["init_" + name] = lat, init
        res["gru_" + name] = states[:, :ref.gru_floats].copy()
        res["mem_crc_" + name] = em.mem_crc(states, ref.gru_floats)
        res["mem_full_" + name] = states[0, ref.gru_floats:].copy()
        res["blob_crc_" + name] = np.uint32(zlib.crc32(blob))
    # the long run at the training defaults
    blob = di.blob_enc("tf")
    feat = em.long_inputs()
    ref = RefEncoder(L, blob)
    lat, init, states = ref.encode_all(feat, em.LONG_COUNT)
    assert np.isfinite(lat).all() and np.isfinite(init).all() and np.isfinite(states).all()
    s = em.LONG_FULL_STREAM
    m_lat, m_init = (lambda net: net.encode(net.fresh(), feat[s], int(em.LONG_COUNT[s])))(di.DredEncNumpyI8(blob))
    assert same(m_lat, lat[s]) and same(m_init, init[s])
    res["long_crc"] = em.rows_crc(lat, init, em.LONG_COUNT)
    res["long_lat"], res["long_init"] = lat[s], init[s]
    res["long_gru_crc"] = np.array([zlib.crc32(st[:ref.gru_floats].tobytes()) for st in states], np.uint32)
    res["long_mem_crc"] = em.mem_crc(states, ref.gru_floats)
    res["long_in_crc"] = np.uint32(zlib.crc32(feat.tobytes()))
    # encoder -> decoder on a blob with both int8 halves: the reference's decode of the reference's encoder output, and the restatement's
    blob = di.blob_enc("tf", with_dec=True)
    assert pm.blob_arrays(blob)["bits_dense_weights"] == pm.blob_arrays(di.blob_enc("tf"))["bits_dense_weights"]
    dec, mine = RefDecoder(L, blob), di.DredDecNumpyI8(blob)
    assert (dec.latent_dim, dec.state_dim) == (em.SETS["tf"]["latent_dim"], em.SETS["tf"]["state_dim"])
    rt = []
    for s in em.RT_STREAMS:
        c = int(em.COUNT[s])
        assert c == em.N_DFRAMES
        rt.append(dec.decode(res["init_tf"][s, c - 1], res["lat_tf"][s, :c][::-1], c))
        assert same(mine.decode(res["init_tf"][s, c - 1], res["lat_tf"][s, :c][::-1], c), rt[-1])
    res["rt_feat"] = np.stack(rt)
    assert np.isfinite(res["rt_feat"]).all()
    res["blob_crc_rt"] = np.uint32(zlib.crc32(blob))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(pm.ROOT, "tests", "golden", "golden_dred_enc_i8_v1.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")
    assert os.path.getsize(out_path) < 150 * 1024


if __name__ == "__main__":
    main()
