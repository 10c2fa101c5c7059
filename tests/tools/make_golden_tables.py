#!/usr/bin/env python3
"""Generate tests/golden/ref_tables_v1.npz: the values of the reference's own constant tables (tansig_table.h; fft_bitrev,
fft_twiddles and dct_table of lpcnet_tables.c), parsed from a reference tree.  tests/test_tables.py holds the generated
tables (tools/gen_tables.py) against these pinned values, so the suite needs no reference tree.

    python tests/tools/make_golden_tables.py <reference>/src
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _floats(text):
    return np.array([float(x) for x in re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f", text)], np.float32)


def main(src):
    t = open(os.path.join(src, "lpcnet_tables.c")).read()
    out = {"tansig": _floats(open(os.path.join(src, "tansig_table.h")).read()),
           "fft_bitrev": np.array([int(x) for x in re.findall(r"-?\d+", re.search(r"fft_bitrev\[\d*\]\s*=\s*\{([^}]*)\}", t).group(1))], np.int32),
           "fft_twiddles": _floats(re.search(r"fft_twiddles\[\d*\]\s*=\s*\{(.*?)\};", t, re.S).group(1)).reshape(-1, 2),
           "dct_table": _floats(re.search(r"dct_table\[\d*\]\s*=\s*\{(.*?)\};", t, re.S).group(1))}
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_tables_v1.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
