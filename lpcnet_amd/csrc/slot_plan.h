// What the slot start and the close of P1 have to do on ONE wave of the two-group kernel (sample_kernel_x2.hip.h), derived once per
// launch from the wave's dealing: a wave owns up to three slots of GRU-A rows (one row per lane and slot), slot k runs items
// [b_k, b_k+1) with b_0 = 0; a slot holds update / reset rows (they start from the cell the start-value pass has written), candidate
// rows (they start from bias + diag*h, formed in P1 -- unless slot 0's head has parked its partial sums in the cell one sample ahead),
// or nothing.  The generic walk -- open slot 0, move from slot to slot at the boundaries, close through slot 2 -- reads and rewrites
// cells that already hold their values wherever a slot has no items: a parked slot 0 whose items all ran in the head, the empty
// slots behind the last item.  The plan names the slot the start opens and the slot the close stores, and which slots need
// bias + diag*h formed at all.
// Plain constexpr functions of wave-uniform values: host code and tests include this header too (tests/test_slot_plan.py).
#pragma once
#include "lpcnet_math.h"      // LPCN_HD

// one word (an SGPR): bit k slot k has a row on some lane | bit 3 + k some row of slot k is a candidate row | bit 6 slot 0 is parked by a
// head | bits 8..9 the first slot that has items | bits 10..11 the slot the last item belongs to | bits 12..13 the number of slots that have items
LPCN_HD constexpr int lpcn_slot_plan(const int live, const int cand, const int b1, const int b2, const int b3, const int head)
{
    const int first = b3 <= 0 ? 0 : (b1 <= 0 ? 1 : 0) + (b2 <= 0 ? 1 : 0);      // (a wave without items: slot 0)
    const int last = (b1 < b3 ? 1 : 0) + (b2 < b3 ? 1 : 0);
    const int with_items = (b1 > 0 ? 1 : 0) + (b2 > b1 ? 1 : 0) + (b3 > b2 ? 1 : 0);
    return (live & 7) | ((cand & 7) << 3) | ((head > 0 ? 1 : 0) << 6) | (first << 8) | (last << 10) | (with_items << 12);
}
// (which slots have rows, and how many slots have items: not used by the kernel -- for tests and tools that print a wave's plan)
LPCN_HD constexpr bool lpcn_slot_live(const int plan, const int k) { return ((plan >> k) & 1) != 0; }
LPCN_HD constexpr bool lpcn_slot_parked(const int plan, const int k) { return k == 0 && ((plan >> 6) & 1) != 0; }
LPCN_HD constexpr int lpcn_slot_with_items(const int plan) { return (plan >> 12) & 3; }
// slot k holds candidate rows that no head has parked: the start forms bias + diag*h for them
LPCN_HD constexpr bool lpcn_slot_forms_start(const int plan, const int k) { return ((plan >> (3 + k)) & 1) != 0 && !lpcn_slot_parked(plan, k); }
// no slot of the wave does: every running row starts from its cell
LPCN_HD constexpr bool lpcn_slot_plain_start(const int plan) { return !lpcn_slot_forms_start(plan, 0) && !lpcn_slot_forms_start(plan, 1) && !lpcn_slot_forms_start(plan, 2); }
// the slot the start opens: on a plain wave the first one that has items (the slots in front of it keep their cells); a wave that forms start
// values opens slot 0 and walks (an unparked candidate slot without items still has to get bias + diag*h into its cell)
LPCN_HD constexpr int lpcn_slot_first(const int plan) { return lpcn_slot_plain_start(plan) ? (plan >> 8) & 3 : 0; }
// the slot the close stores: the one the last item belongs to (slot 0 on a wave without items)
LPCN_HD constexpr int lpcn_slot_last(const int plan) { return (plan >> 10) & 3; }
// the walk moves from slot k - 1 to slot k in front of item j (b = b_k): never in front of item 0 into a slot the start has opened or skipped
LPCN_HD constexpr bool lpcn_slot_moves(const int plan, const int k, const int j, const int b) { return j == b && (j > 0 || lpcn_slot_first(plan) < k); }
