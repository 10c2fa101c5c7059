// Host build of the two-stage tree mapping the two-group sample kernel uses (lpcnet_amd/csrc/tree_stages.h), for tests/test_tree_stages.py.
#include "tree_stages.h"

extern "C" {
int ts_levels(void) { return LPCN_TREE_LEVELS; }
int ts_top(void) { return LPCN_TREE_TOP; }
int ts_stage_nodes(int stage) { return lpcn_tree_stage_nodes(stage); }
int ts_lane_local(int stage, int lane) { return lpcn_tree_lane_local(stage, lane); }
int ts_level(int stage, int k) { return lpcn_tree_level(stage, k); }
int ts_node(int stage, int k, int prefix) { return lpcn_tree_node(stage, k, prefix); }
unsigned long long ts_stage_mask(int stage) { return lpcn_tree_stage_mask(stage); }
int ts_stage_walk(unsigned long long ballot, int levels) { return lpcn_tree_stage_walk(ballot, levels); }
}
