// The sampler's dual-FC tree (src/nnet.c:163-214: 255 nodes in heap order, node n's children 2 n and 2 n + 1, 8 levels) evaluated
// in TWO dependent stages by one wave per stream (sample_kernel_x2.hip.h): stage 1 speculates over the fixed top
// LPCN_TREE_TOP levels, a walk over its ballot names the node the path reaches on the next level, stage 2 speculates over the
// subtree under that node.  31 + 7 node evaluations instead of 255; the 8 nodes on the path are among them whatever the walk
// decides (tests/test_tree_stages.py checks this for all 256 leaves).  Plain constexpr functions: host code and tests include
// this header too.
#pragma once
#include "lpcnet_math.h"      // LPCN_HD

#define LPCN_TREE_LEVELS 8
#define LPCN_TREE_TOP 5                                    // levels of stage 1 (nodes 1..31); stage 2 takes the other 3 (7 nodes)

// A lane of either stage is (local node k = lane >> 1, channel = lane & 1); k counts the stage's nodes in heap order from 1,
// so bit 2 k of the stage's ballot belongs to local node k and a walk over it is the reference's walk over node numbers.
// Lanes whose k is outside the stage evaluate the stage's first node again (a valid row; their ballot bits are masked off).
LPCN_HD constexpr int lpcn_tree_stage_nodes(const int stage) { return stage == 0 ? (1 << LPCN_TREE_TOP) - 1 : (1 << (LPCN_TREE_LEVELS - LPCN_TREE_TOP)) - 1; }
LPCN_HD constexpr int lpcn_tree_lane_local(const int stage, const int lane)
{
    const int k = lane >> 1;
    return (k >= 1 && k <= lpcn_tree_stage_nodes(stage)) ? k : 1;
}
LPCN_HD constexpr int lpcn_tree_local_level(const int k) { return k >= 16 ? 4 : k >= 8 ? 3 : k >= 4 ? 2 : k >= 2 ? 1 : 0; }      // floor(log2 k), k in 1..31
// tree level (0 = root) and node number of local node k; `prefix` = the LPCN_TREE_TOP bits stage 1's walk has decided (stage 0: unused)
LPCN_HD constexpr int lpcn_tree_level(const int stage, const int k) { return (stage == 0 ? 0 : LPCN_TREE_TOP) + lpcn_tree_local_level(k); }
LPCN_HD constexpr int lpcn_tree_node(const int stage, const int k, const int prefix)
{
    const int l = lpcn_tree_local_level(k), root = stage == 0 ? 1 : (1 << LPCN_TREE_TOP) | prefix;
    return (root << l) | (k - (1 << l));
}
// ballot bits that count: channel-0 lanes of the stage's nodes
LPCN_HD constexpr unsigned long long lpcn_tree_stage_mask(const int stage)
{
    return 0x5555555555555555ull & ((1ull << (2 * lpcn_tree_stage_nodes(stage) + 1)) - 1) & ~3ull;      // (stage 0: 2 * 31 + 1 = 63 bits)
}
// the walk over a stage's ballot: `levels` decisions from local node 1; returns the decided bits, first decision highest
LPCN_HD constexpr int lpcn_tree_stage_walk(const unsigned long long ballot, const int levels)
{
    int val = 0;
    for (int b = 0; b < levels; ++b) val = (val << 1) | (int)((ballot >> (2 * ((1 << b) | val))) & 1ull);
    return val;
}

// ---- stage 2 of FOUR streams in one pass of one wave (round 9): the wave is four 16-lane FIELDS, field f = lane >> 4 belongs to stream f of
// the group and is a stage-2 wave cut to 16 lanes -- local lane l = lane & 15 is (local node l >> 1, channel l & 1), the 7 nodes of the subtree
// under the node stream f's own prefix names; lanes 0, 1 of a field evaluate the subtree's first node again (a valid row, masked off).  The
// 64-bit ballot is four 16-bit stage ballots, each walked like a stage-2 ballot (tests/test_tree_stages_packed.py).
#define LPCN_TREE_FIELD_LANES 16
#define LPCN_TREE_FIELDS 4
LPCN_HD constexpr int lpcn_tree_packed_field(const int lane) { return lane / LPCN_TREE_FIELD_LANES; }
LPCN_HD constexpr int lpcn_tree_packed_local(const int lane) { return lpcn_tree_lane_local(1, lane % LPCN_TREE_FIELD_LANES); }      // 1..7
LPCN_HD constexpr int lpcn_tree_packed_level(const int lane) { return lpcn_tree_level(1, lpcn_tree_packed_local(lane)); }
LPCN_HD constexpr int lpcn_tree_packed_node(const int lane, const int prefix) { return lpcn_tree_node(1, lpcn_tree_packed_local(lane), prefix); }      // prefix: the lane's field's
// ballot bits that count: the stage-2 mask in every field
LPCN_HD constexpr unsigned long long lpcn_tree_packed_mask()
{
    unsigned long long m = 0;
    for (int f = 0; f < LPCN_TREE_FIELDS; ++f) m |= lpcn_tree_stage_mask(1) << (LPCN_TREE_FIELD_LANES * f);
    return m;
}
// the walk over field f of the packed ballot: the last LPCN_TREE_LEVELS - LPCN_TREE_TOP decisions of stream f
LPCN_HD constexpr int lpcn_tree_packed_walk(const unsigned long long ballot, const int field)
{
    return lpcn_tree_stage_walk((ballot >> (LPCN_TREE_FIELD_LANES * field)) & ((1ull << LPCN_TREE_FIELD_LANES) - 1), LPCN_TREE_LEVELS - LPCN_TREE_TOP);
}
static_assert(2 * lpcn_tree_stage_nodes(1) + 2 <= LPCN_TREE_FIELD_LANES && LPCN_TREE_FIELDS * LPCN_TREE_FIELD_LANES == 64, "a stage-2 subtree fits a 16-lane field");
