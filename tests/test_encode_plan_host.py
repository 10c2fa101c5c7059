"""The launch plan of the encoder and the feature analysis (lpcnet_hip_encode_plan, api.encode_plan), no GPU: the chunk rule and the
items-per-wavefront rule are the ones the launch code uses (lpcnet_amd/csrc/encode_plan.h, one definition), so this shows which shapes reach
the VQ kernels' forms with 2, 3 and 4 items per wavefront, their ragged last workgroups and the second chunk of a call -- the shapes of
tests/test_gpu_encode_large.py do, and no shape of the other encoder and analysis tests does."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import encode_large_cases as cases  # noqa: E402
from lpcnet_amd import api  # noqa: E402

CSRC = os.path.join(ROOT, "lpcnet_amd", "csrc")


def test_the_large_cases_reach_ipw_4_3_2_ragged_workgroups_and_two_chunks(hip_lib):
    cases.check_plans()


@pytest.mark.parametrize("items,ipw_end,ipw_mid", [(4095, 1, 1), (4096, 1, 1), (8191, 1, 1), (8192, 2, 2), (12287, 2, 2), (12288, 3, 2),
                                                   (16383, 3, 2), (16384, 4, 2), (65536, 4, 2)])
def test_the_edges_of_the_items_per_wavefront_rule(hip_lib, items, ipw_end, ipw_mid):
    (r,) = api.encode_plan(items, items, 1)                                      # one packet per stream: items = active streams
    assert (r["packets"], r["items"], r["ipw_end"], r["ipw_mid"]) == (1, items, ipw_end, ipw_mid)
    for ipw, wg, last in ((ipw_end, r["wg_end"], r["last_end"]), (ipw_mid, r["wg_mid"], r["last_mid"])):
        per = 8 * ipw
        assert wg == -(-items // per) and last == items - (wg - 1) * per and 1 <= last <= per
        assert wg >= 512 or ipw == 1                                             # more than one item per wavefront only with two workgroups per CU left


def test_the_chunk_follows_the_capacity_and_the_launches_follow_the_active_count(hip_lib):
    assert [r["packets"] for r in api.encode_plan(2048, 5, 20)] == [8, 8, 4]
    assert [r["items"] for r in api.encode_plan(2048, 5, 20)] == [40, 40, 20]
    assert [r["frames"] for r in api.encode_plan(2048, 5, 70, analysis=True)] == [32, 32, 6]
    assert [r["packets"] for r in api.encode_plan(3000, 3000, 11)] == [5, 5, 1]   # 65536 / 3000 / 4
    assert [r["frames"] for r in api.encode_plan(3000, 3000, 43, analysis=True)] == [21, 21, 1]
    assert api.encode_plan(16384, 16384, 1) == [dict(packets=1, items=16384, ipw_end=4, ipw_mid=2, wg_end=512, last_end=32, wg_mid=1024, last_mid=16)]
    assert len(api.encode_plan(16384, 16384, 2)) == 2                            # 16384 x 4 frames fill the bound
    # a batch larger than the bound: one packet, one frame per chunk
    big = api.encode_plan(65537, 65537, 3)
    assert [r["packets"] for r in big] == [1, 1, 1] and all(r["items"] == 65537 and r["ipw_end"] == 4 and r["ipw_mid"] == 2 for r in big)
    assert (big[0]["wg_end"], big[0]["last_end"], big[0]["wg_mid"], big[0]["last_mid"]) == (2049, 1, 4097, 1)
    assert [r["frames"] for r in api.encode_plan(70000, 70000, 3, analysis=True)] == [1, 1, 1]
    assert api.encode_plan(2048, 0, 9) == [] and api.encode_plan(2048, 0, 9, analysis=True) == []      # no active stream: no launch


def test_argument_errors(hip_lib):
    for args in ((0, 0, 1), (4, 5, 1), (4, -1, 1), (4, 4, 0)):
        with pytest.raises(api.LPCNetError, match="bad arguments"):
            api.encode_plan(*args)
    out = np.zeros(8, np.int32)
    assert hip_lib.lpcnet_hip_encode_plan(2048, 2048, 9, 0, out.ctypes.data, 1) == 2 and out[0] == 8      # records beyond cap are counted, not written
    assert hip_lib.lpcnet_hip_encode_plan(2048, 2048, 9, 0, None, 1) == -4


def test_no_other_encoder_or_analysis_test_reaches_these_forms(hip_lib):
    """every (capacity, packets) of tests/test_gpu_encode.py and (capacity, frames) of tests/test_gpu_analysis.py (a sharded batch by its shards):
    one item per wavefront, one chunk"""
    encode = [(6, 64), (6, 30), (6, 18), (6, 12), (6, 10), (6, 5), (6, 4), (6, 3), (6, 2), (6, 1), (8, 30), (3, 5), (3, 4), (3, 3), (3, 2), (3, 1),
              (2048, 2), (64, 2), (1, 2), (151, 2), (150, 2), (151, 1), (150, 1), (2, 1)]
    analyze = [(6, 240), (6, 75), (6, 45), (6, 40), (6, 30), (6, 10), (6, 6), (6, 1), (1, 240), (8, 120), (3, 5), (3, 3), (3, 1), (2048, 3), (64, 3),
               (151, 2), (150, 2), (151, 1), (150, 1), (2, 1)]
    assert max(n * P for n, P in encode) == 4096 and max(n * T for n, T in analyze) == 6144      # below 8 192 items and 65 536 frame items
    for n, P in encode:
        (r,) = api.encode_plan(n, n, P)
        assert r["ipw_end"] == 1 and r["ipw_mid"] == 1, (n, P)
    for n, T in analyze:
        assert len(api.encode_plan(n, n, T, analysis=True)) == 1, (n, T)


def test_the_rule_has_one_definition_and_the_launch_code_uses_it():
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".c", ".cpp"))}
    for name in ("lpcn_encode_ipw", "lpcn_encode_chunk", "lpcn_analysis_chunk"):
        defs = [f for f, s in src.items() if re.search(r"static inline int " + name + r"\(", s)]
        assert defs == ["encode_plan.h"], (name, defs)
    assert [f for f, s in src.items() if re.search(r"#define\s+LPCN_AN_ITEMS_MAX", s)] == ["encode_plan.h"]
    assert src["encode_kernels.hip.h"].count("lpcn_encode_ipw(items, ") == 2
    codec = src["engine_codec.hip"]
    assert "const int chunk = lpcn_analysis_chunk(b->n, n_frames);" in codec and "const int want = lpcn_encode_chunk(b->n, n_packets);" in codec
    assert "const int chunk = want;" in codec and "+= b->an_chunk" not in codec and "b->enc_chunk < b->an_chunk" not in codec
    assert "lpcn_encode_ipw(items, LPCN_ENC_END_IPW)" in src["api_tools.c"] and "lpcn_encode_chunk(n, count)" in src["api_tools.c"]
