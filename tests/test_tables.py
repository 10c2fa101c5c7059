"""The generated constant tables (tools/gen_tables.py) against the reference's own tables -- their values pinned in
tests/golden/ref_tables_v1.npz (tests/tools/make_golden_tables.py) -- and against their closed formulas."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tables  # noqa: E402


@pytest.fixture(scope="module")
def ref_tables():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_tables_v1.npz"))


def test_tansig_matches_reference_header(ref_tables):
    ref = ref_tables["tansig"]
    assert ref.dtype == np.float32 and ref.size == 201 and np.array_equal(ref, gen_tables.tansig())


def test_fft_and_dct_tables_match_reference(ref_tables):
    assert ref_tables["fft_bitrev"].size == 320 and np.array_equal(ref_tables["fft_bitrev"], gen_tables.fft_bitrev())
    tw = ref_tables["fft_twiddles"]
    assert tw.dtype == np.float32 and tw.shape == (320, 2) and np.array_equal(tw, gen_tables.fft_twiddles())
    dct = ref_tables["dct_table"]
    assert dct.dtype == np.float32 and dct.size == 324 and np.array_equal(dct, gen_tables.idct_table())


def test_headers_are_in_sync_with_generator():
    for path, prefix in ((os.path.join(ROOT, "lpcnet_amd", "csrc", "lpcnet_tables_gen.h"), "lpcn_"),
                         (os.path.join(ROOT, "oracle", "orc_tables_gen.h"), "orc_")):
        text = open(path).read()
        body = re.search(prefix + r"tansig\[201\] = \{(.*?)\};", text, re.S).group(1)
        vals = np.array([float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fp.+-]+f", body)], np.float32)
        assert np.array_equal(vals, gen_tables.tansig())


def test_formula_sanity():
    u = gen_tables.ulaw2lin()
    assert u[128] == 0.0 and 31000 < u[255] < 32768 and np.all(np.diff(u) > 0)
    lg = gen_tables.logit_table()
    assert abs(lg[0] + math.log(0.975 / 0.025)) < 1e-5 and np.all(np.diff(lg) > 0)
    assert sorted(gen_tables.fft_bitrev().tolist()) == list(range(320))
