// Host build of the packed stage-2 mapping of the two-group sample kernel (lpcnet_amd/csrc/tree_stages.h: four 16-lane fields, one per stream),
// for tests/test_tree_stages_packed.py.
#include "tree_stages.h"

extern "C" {
int tp_levels(void) { return LPCN_TREE_LEVELS; }
int tp_top(void) { return LPCN_TREE_TOP; }
int tp_fields(void) { return LPCN_TREE_FIELDS; }
int tp_field_lanes(void) { return LPCN_TREE_FIELD_LANES; }
int tp_field(int lane) { return lpcn_tree_packed_field(lane); }
int tp_local(int lane) { return lpcn_tree_packed_local(lane); }
int tp_level(int lane) { return lpcn_tree_packed_level(lane); }
int tp_node(int lane, int prefix) { return lpcn_tree_packed_node(lane, prefix); }
unsigned long long tp_mask(void) { return lpcn_tree_packed_mask(); }
int tp_walk(unsigned long long ballot, int field) { return lpcn_tree_packed_walk(ballot, field); }
// the single-stream stage 2 the packed form must agree with
int ts_stage_nodes(int stage) { return lpcn_tree_stage_nodes(stage); }
int ts_node(int stage, int k, int prefix) { return lpcn_tree_node(stage, k, prefix); }
}
