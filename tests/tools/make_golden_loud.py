#!/usr/bin/env python3
"""Generate tests/golden/golden_loud_v1.npz: the REAL reference (oracle/_ref, generic-C float and int8 builds) driven over the
loud input families of tests/tools/loud_inputs.py -- teacher forcing at full scale through lpcnet_synthesize_impl, and the
resonator-LPC families through lpcnet_synthesize_tail_impl with the caller's LPC (oracle/ref_harness.c: ref_synthesize_tail).
Per family and flavour (f = float blob, i = int8 blob): the PCM and the final gru_a, gru_b, last_sig, last_exc, deemph_mem, rng.
The inputs are reproducible from their seeds; the fixture keeps a CRC of each family's inputs.  Arrays only.

    make -C oracle ref && python tests/tools/make_golden_loud.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import loud_inputs  # noqa: E402
from lpcnet_amd import synth  # noqa: E402
from oracle import ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "golden_loud_v1.npz")


def main():
    out = {}
    fams = loud_inputs.families()
    out["names"] = np.array([f.name for f in fams])
    out["n_frames"] = np.array(loud_inputs.T)
    out["input_crc"] = np.array([f.digest() for f in fams], np.uint32)
    for fl, flavour, kind in (("f", "gf", "float"), ("i", "gi", "int8")):
        lib = ref.RefLib(flavour)
        blob = synth.blob_bytes(synth.make_model(flavour=kind))
        for fam in fams:
            pcm, st = loud_inputs.run_reference(lib, blob, fam)
            assert np.isfinite(st["last_sig"]).all() and np.isfinite(st["deemph_mem"]) and np.isfinite(st["gru_a"]).all()
            out[f"pcm_{fl}_{fam.name}"] = pcm
            for k in loud_inputs.STATE_KEYS:
                out[f"{k}_{fl}_{fam.name}"] = np.asarray(st[k])
    # lin2ulaw where the loud families drive it (golden_v1's table ends at +-40000): magnitudes up to 4e6, which the resonator
    # families reach, and every float in a window around +-32768, where the conversion starts to clamp
    mags = np.concatenate([np.geomspace(30000.0, 4.0e6, 300), 32768.0 * (1.0 + np.arange(-300, 301) * 2.0 ** -21)]).astype(np.float32)
    xs = np.concatenate([mags, -mags])
    gf = ref.RefLib("gf")
    out["ulaw_x"] = xs
    out["lin2ulaw"] = np.array([gf.lib.ref_lin2ulaw(float(x)) for x in xs], np.int32)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
