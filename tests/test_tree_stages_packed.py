"""The packed stage 2 of the sampler's tree (lpcnet_amd/csrc/tree_stages.h, round 9 of the two-group sample kernel): ONE wave evaluates the last
three levels of FOUR streams, lane 16 f + l being local lane l of stream f with stream f's own five-bit prefix, takes one 64-bit ballot and walks
each 16-bit field.  Checked here on the host, exhaustively, from the header the kernel includes: for every leaf and every field the nodes the
reference visits on its last three levels (src/nnet.c:186-211) are among the field's lanes, each at its level, and the field's walk returns the
reference's decisions whatever the other three fields hold."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tree_stages_packed") / "libtree_stages_packed_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "tree_stages_packed_host.cpp"), "-o", out])
    L = C.CDLL(out)
    L.tp_mask.restype = C.c_ulonglong
    L.tp_walk.argtypes = [C.c_ulonglong, C.c_int]
    return L


def reference_path(leaf):
    """the (level, node) pairs sample_mdense visits for the 8 decisions `leaf` (first decision = highest bit)"""
    path, node = [], 1
    for level in range(8):
        path.append((level, node))
        node = 2 * node + ((leaf >> (7 - level)) & 1)
    return path


def field_lanes(tp, field, prefix):
    """{(node, channel): (lane, level)} of the lanes of `field` whose ballot bit counts (channel 0) and of their channel-1 partners"""
    mask, fl = tp.tp_mask(), tp.tp_field_lanes()
    out = {}
    for lane in range(fl * field, fl * (field + 1)):
        if not (mask >> (lane & ~1)) & 1:
            continue
        assert tp.tp_field(lane) == field
        assert tp.tp_local(lane) == (lane % fl) >> 1
        key = (tp.tp_node(lane, prefix), lane & 1)
        assert key not in out
        out[key] = (lane, tp.tp_level(lane))
    return out


def test_fields_and_counts(tp):
    assert tp.tp_levels() == 8 and tp.tp_fields() == 4 and tp.tp_fields() * tp.tp_field_lanes() == 64
    n2 = tp.ts_stage_nodes(1)
    assert n2 == 2 ** (8 - tp.tp_top()) - 1 and 2 * n2 + 2 <= tp.tp_field_lanes()
    mask = tp.tp_mask()
    assert bin(mask).count("1") == 4 * n2
    for f in range(4):                                       # the same bits in every field, none on a channel-1 lane or on local node 0
        fm = (mask >> (16 * f)) & 0xFFFF
        assert fm == mask & 0xFFFF and fm & 0xAAAA == 0 and fm & 3 == 0


def test_every_lane_addresses_a_valid_row(tp):
    """all 64 lanes load a row, counted or not: node in 1..255 and a level of stage 2, for every lane and every prefix of its field"""
    top = tp.tp_top()
    for prefix in range(2 ** top):
        for lane in range(64):
            assert 0 <= tp.tp_field(lane) < 4
            assert 1 <= tp.tp_local(lane) <= tp.ts_stage_nodes(1)
            node = tp.tp_node(lane, prefix)
            assert 1 <= node <= 255
            assert top <= tp.tp_level(lane) <= 7 and tp.tp_level(lane) == node.bit_length() - 1
            assert node == tp.ts_node(1, tp.tp_local(lane), prefix)      # the single-stream stage 2's node for the same local node


def test_field_lanes_are_distinct_node_channels_at_their_levels(tp):
    top = tp.tp_top()
    for field in range(4):
        for prefix in range(2 ** top):
            lanes = field_lanes(tp, field, prefix)
            assert len(lanes) == 2 * tp.ts_stage_nodes(1)
            for (node, chan), (lane, level) in lanes.items():
                assert level == node.bit_length() - 1                     # the threshold a node is compared with is its level's
                assert lanes[(node, chan ^ 1)][0] == lane ^ 1              # the two channels of a node sit in neighbouring lanes (quad_perm [1,0,3,2])
                assert node >> (level - top) == (1 << top) | prefix       # inside the subtree the prefix names


def test_all_256_leaves_walk_in_every_field(tp):
    """the field under test carries leaf `leaf`; the other three carry three other leaves (other prefixes, other decisions) at the same time"""
    top = tp.tp_top()
    low = 8 - top
    for leaf in range(256):
        path = reference_path(leaf)
        for field in range(4):
            leaves = [(leaf * 37 + 91 * (g - field)) % 256 if g != field else leaf for g in range(4)]
            ballot = 0
            for g in range(4):
                pg = reference_path(leaves[g])
                lanes = field_lanes(tp, g, leaves[g] >> low)
                assert {n for _, n in pg[top:]} <= {n for n, _ in lanes}
                # exactly the decisions of the field's leaf on its path -- and the OPPOSITE bit on every other node, so a walk that looks at a
                # node off the path, or into another field, returns something else
                for (node, chan), (lane, level) in lanes.items():
                    if chan:
                        continue
                    on_path = (level, node) in pg
                    bit = (leaves[g] >> (7 - level)) & 1
                    if bit if on_path else not bit:
                        ballot |= 1 << lane
            assert ballot & ~tp.tp_mask() == 0
            for g in range(4):
                assert ((leaves[g] >> low) << low) | tp.tp_walk(ballot, g) == leaves[g], (leaf, field, g)
            assert {n for _, n in path[top:]} <= {n for n, _ in field_lanes(tp, field, leaf >> low)}
