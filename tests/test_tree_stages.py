"""The two-stage form of the sampler's tree (lpcnet_amd/csrc/tree_stages.h, used by the two-group sample kernel): the reference visits 8 nodes
per sample, node 1 and then child 2 n + bit (src/nnet.c:186-211); the kernel evaluates the fixed top levels, walks them, and evaluates the subtree
under the node reached.  Checked here on the host, exhaustively, from the header the kernel includes: whatever the 8 decisions are, the nodes on the
path are among the ones evaluated, each at its level, and the two walks return the decisions."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tree_stages") / "libtree_stages_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "tree_stages_host.cpp"), "-o", out])
    L = C.CDLL(out)
    L.ts_stage_mask.restype = C.c_ulonglong
    L.ts_stage_walk.argtypes = [C.c_ulonglong, C.c_int]
    return L


def reference_path(leaf):
    """the (level, node) pairs sample_mdense visits for the 8 decisions `leaf` (first decision = highest bit)"""
    path, node = [], 1
    for level in range(8):
        path.append((level, node))
        node = 2 * node + ((leaf >> (7 - level)) & 1)
    return path


def stage_lanes(ts, stage, prefix):
    """{(node, channel): (lane, level)} of the lanes whose ballot bit counts (channel 0) and of their channel-1 partners"""
    mask = ts.ts_stage_mask(stage)
    out = {}
    for lane in range(64):
        if not (mask >> (lane & ~1)) & 1:
            continue
        k = ts.ts_lane_local(stage, lane)
        assert k == lane >> 1
        key = (ts.ts_node(stage, k, prefix), lane & 1)
        assert key not in out
        out[key] = (lane, ts.ts_level(stage, k))
    return out


def test_split_and_counts(ts):
    assert ts.ts_levels() == 8 and 1 <= ts.ts_top() <= 7
    top = ts.ts_top()
    assert ts.ts_stage_nodes(0) == 2 ** top - 1 and ts.ts_stage_nodes(1) == 2 ** (8 - top) - 1
    assert 2 * ts.ts_stage_nodes(0) + 2 <= 64 and 2 * ts.ts_stage_nodes(1) + 2 <= 64      # one (node, channel) per lane of a wave
    for stage in (0, 1):
        assert bin(ts.ts_stage_mask(stage)).count("1") == ts.ts_stage_nodes(stage)


def test_every_lane_addresses_a_valid_row(ts):
    """all 64 lanes load a row, counted or not: node in 1..255 for every lane, stage and prefix"""
    top = ts.ts_top()
    for stage in (0, 1):
        for prefix in range(2 ** top if stage else 1):
            for lane in range(64):
                k = ts.ts_lane_local(stage, lane)
                assert 1 <= k <= ts.ts_stage_nodes(stage)
                assert 1 <= ts.ts_node(stage, k, prefix) <= 255
                assert 0 <= ts.ts_level(stage, k) <= 7


def test_stage_lanes_are_distinct_node_channels_at_their_levels(ts):
    top = ts.ts_top()
    for stage in (0, 1):
        for prefix in range(2 ** top if stage else 1):
            lanes = stage_lanes(ts, stage, prefix)
            assert len(lanes) == 2 * ts.ts_stage_nodes(stage)
            for (node, chan), (lane, level) in lanes.items():
                assert level == node.bit_length() - 1                     # the threshold a node is compared with is its level's
                assert lanes[(node, chan ^ 1)][0] == lane ^ 1              # the two channels of a node sit in neighbouring lanes (quad_perm [1,0,3,2])


def test_all_256_leaves_path_nodes_are_evaluated_and_walked(ts):
    top = ts.ts_top()
    for leaf in range(256):
        path = reference_path(leaf)
        prefix = leaf >> (8 - top)
        s0, s1 = stage_lanes(ts, 0, 0), stage_lanes(ts, 1, prefix)
        nodes0 = {n for n, _ in s0}
        nodes1 = {n for n, _ in s1}
        assert not nodes0 & nodes1
        assert {n for _, n in path} <= nodes0 | nodes1
        assert {n for _, n in path[:top]} <= nodes0 and {n for _, n in path[top:]} <= nodes1
        # ballots in which exactly the decisions of this leaf are set on the path -- and the OPPOSITE bit on every other node, so a walk that
        # looks at a node off the path returns something else
        ballots = []
        for stage, lanes in ((0, s0), (1, s1)):
            m = 0
            for (node, chan), (lane, level) in lanes.items():
                if chan:
                    continue
                on_path = (level, node) in path
                bit = (leaf >> (7 - level)) & 1
                if bit if on_path else not bit:
                    m |= 1 << lane
            assert m & ~ts.ts_stage_mask(stage) == 0
            ballots.append(m)
        got0 = ts.ts_stage_walk(ballots[0], top)
        assert got0 == prefix
        got1 = ts.ts_stage_walk(ballots[1], 8 - top)
        assert (got0 << (8 - top)) | got1 == leaf
