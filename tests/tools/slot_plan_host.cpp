// Host build of lpcnet_amd/csrc/slot_plan.h for tests/test_slot_plan.py: the plan's fields, and the slot start / walk / close of P1 exactly as
// sample_kernel_x2.hip.h runs them from the plan (restated here statement by statement: the kernel's own code needs a GPU, tests/test_gpu_x2_slots.py), on SYMBOLIC values -- a value is (origin, first item added, one past the last item added) with
// origin k = the content slot k's cell has when P1 begins, 3 + k = bias + diag*h of slot k's rows, 6 = the dummy cell a lane without a row reads.
#include "slot_plan.h"

extern "C" {
int sp_plan(int live, int cand, int b1, int b2, int b3, int head) { return lpcn_slot_plan(live, cand, b1, b2, b3, head); }
int sp_live(int plan, int k) { return lpcn_slot_live(plan, k); }
int sp_parked(int plan, int k) { return lpcn_slot_parked(plan, k); }
int sp_forms_start(int plan, int k) { return lpcn_slot_forms_start(plan, k); }
int sp_plain_start(int plan) { return lpcn_slot_plain_start(plan); }
int sp_first(int plan) { return lpcn_slot_first(plan); }
int sp_last(int plan) { return lpcn_slot_last(plan); }
int sp_with_items(int plan) { return lpcn_slot_with_items(plan); }

struct Val { int origin, lo, hi; };
enum { EMPTY = 0, UPDATE_RESET = 1, CANDIDATE = 2, DUMMY = 6 };

// kind[k]: what the row of the lane under test in slot k is; other[k]: what another lane of the same wave holds there (the plan is the wave's: the ballots
// see both); NW: items per lane of the kernel variant.  out: [3] the value the lane's first item is added to (origin -1: the wave has no items), then
// [3][3] the final contents of the lane's cells
void sp_run(const int *kind, const int *other, int parked, int b1, int b2, int b3, int NW, int *out)
{
    int live = 0, cand = 0;
    for (int k = 0; k < 3; ++k) {
        if (kind[k] != EMPTY || other[k] != EMPTY) live |= 1 << k;
        if (kind[k] == CANDIDATE || other[k] == CANDIDATE) cand |= 1 << k;
    }
    const int plan = lpcn_slot_plan(live, cand, b1, b2, b3, parked);
    Val cell[3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}}, acc = {DUMMY, 0, 0};
    auto read = [&](int k) { return kind[k] != EMPTY ? cell[k] : Val{DUMMY, 0, 0}; };
    // ---- slot start
    const int first = lpcn_slot_first(plan);
    if (lpcn_slot_plain_start(plan)) {
        acc = read(first);
    } else {
        for (int k = 0; k < 3; ++k) {
            if (k > 0 && !lpcn_slot_forms_start(plan, k)) continue;
            const bool live_row = kind[k] != EMPTY, candidate = kind[k] == CANDIDATE, parked_k = lpcn_slot_parked(plan, k);
            const Val bv = {3 + k, 0, 0};
            if (k == 0) acc = (candidate && !parked_k) ? bv : read(0);
            else if (candidate && live_row) cell[k] = bv;
        }
    }
    auto row_swap = [&](int done, int next) { if (kind[done] != EMPTY) cell[done] = acc; acc = read(next); };
    // ---- items
    const int jend = b3;
    int nextb = first >= 1 ? (first >= 2 || b2 <= 0 ? NW : b2) : b1;
    out[0] = -1; out[1] = out[2] = 0;
    for (int j = 0; j < NW; ++j) {
        if (j >= jend) break;
        if (j == nextb) {
            if (lpcn_slot_moves(plan, 1, j, b1)) row_swap(0, 1);
            if (lpcn_slot_moves(plan, 2, j, b2)) row_swap(1, 2);
            nextb = b1 > j ? b1 : (b2 > j ? b2 : NW);
        }
        if (j == 0) { out[0] = acc.origin; out[1] = acc.lo; out[2] = acc.hi; }
        if (acc.lo == acc.hi) acc.lo = j;
        acc.hi = j + 1;
    }
    // ---- close
    const int last = lpcn_slot_last(plan);
    if (kind[last] != EMPTY) cell[last] = acc;
    for (int k = 0; k < 3; ++k) { out[3 + 3 * k] = cell[k].origin; out[4 + 3 * k] = cell[k].lo; out[5 + 3 * k] = cell[k].hi; }
}
}
