// Packet-loss concealment, host half: lpcnet_plc_update / lpcnet_plc_conceal in causal mode for every stream (src/lpcnet_plc.c:188-340;
// DESIGN.md §4.4).  No branch of the reference looks at audio: the options, skip_analysis, blend, pcm_fill, loss_count, the FEC ring positions
// and fec_skip decide, and they follow from the loss flags and the FEC calls.  So the host keeps that control state (lpcn_plc_ctl), derives
// every stream's branch for a step without reading anything back, and lists the streams of every phase; the data stays on the device.  Plain
// C++: nothing here needs a device (lpcn_plc_ctl_reset and lpcn_plc_ctl_fec_add of lpcnet_engine.h are defined beside the planner).
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>
#include "lpcnet_engine.h"
#include "plc_records.h"

enum { PLC_T_BURG, PLC_T_PRED, PLC_T_MIX, PLC_T_GROUP, PLC_T_ANALYSIS };
struct PlcLaunch {
    int type = 0, op = 0, off = 0, cnt = 0;
    // groups: what runs on the compacted streams, where its features and PCM come from and go to
    int kind = 0, N = LPCN_FRAME_SIZE, preload = 0;
    int feat_src = 0;          // 0 st->features, 1 + k: entry k of the deferred queue
    int pcm_src = 0;           // preload source: 0 none, 1 head of the PCM queue, 2 the call's frame at pcm_off
    int pcm_dst = 0;           // 0 nowhere (the group's compacted PCM is left for a cross-fade), 1 the call's frame at pcm_off
    int pcm_off = 0;
    bool scatter = true, keep = false;
    // the group schedule (plc_plan's `lanes` > 1): launches of different lanes before PLC_T_ANALYSIS name disjoint streams and may run side by side;
    // a group works in rows [slot, slot + cnt) of the engine's group buffers, and the slot ranges of different lanes are disjoint
    int lane = 0, slot = 0;
};
struct PlcPlan { std::vector<int> ctl; std::vector<PlcLaunch> launches; };
constexpr int PLC_MAX_LANES = 4;
constexpr int PLC_LANES_REC = 10;      // ints per launch of lpcn_plc_plan_lanes
// most groups one step can plan: per chain of lost streams (one per number of queue rounds, 0 .. 3) the flushes, two groups a round, the tail and the
// concealed half; the received streams' trial and teacher-forced halves
constexpr int PLC_MAX_GROUPS = 4 * (LPCN_PLC_FBUF + 2 * 3 + 2) + 2;

inline int float_bits(float f) { int i; memcpy(&i, &f, 4); return i; }

// One step of every stream's control state, and the launches it takes.  summary (may be NULL): LPCN_PLC_SUMMARY ints per stream.
// Returns 0, or LPCN_E_ARG with the message in err.
// lanes == 1: one chain of launches, in the order a single stream runs them.  lanes 2 .. PLC_MAX_LANES: the lost streams are split by the number of
// queue rounds they take in this step into up to four chains, each with its own flush, prediction, round, shift, tail and concealed-half launches, and
// the chains are dealt to the lanes, longest first, onto the lane with the least work so far; the received streams' chain stays on lane 0, and so does
// everything from PLC_T_ANALYSIS on.  Every stream sees the launches of the one-lane plan, in their order, all in one lane.
int plc_plan(int options, int n, lpcn_plc_ctl *ctl, const unsigned char *lost, PlcPlan &P, int *summary, char *err, size_t err_len, int lanes = 1);
// ints per record of a launch's list
inline int plc_rec_size(const PlcLaunch &L) { return L.type == PLC_T_PRED ? lpcn::PLC_PRED_REC : L.type == PLC_T_MIX ? lpcn::PLC_MIX_REC : L.type == PLC_T_ANALYSIS ? 0 : 1; }

// A batched FEC feed (lpcnet_batch_plc_fec_feed): per stream lpcnet_plc_fec_clear if clear[s], skip[s] NULL adds, then count[s] vectors through
// lpcnet_plc_fec_add (src/lpcnet_plc.c:111-132), planned from the ring positions alone.  A stream's vectors are rows [off, off + count[s]) of the
// packed source, off the sum of the counts before it.  The ring takes a = min(count, 100 - fill) rows at row fill; if vectors remain and
// keep > 0 the one compaction a call can cause follows (rows [keep, 100) to the front: keep grows in steps, not in adds), then up to keep more
// rows; the rest -- always the tail of the stream's list -- is dropped.  One record of PLC_FEED_REC ints per stream that stores something, in
// stream order: {stream, off, a, fill, keep, 100 - keep, b, 100 - keep}, the last four 0 without a compaction.  skip and clear may be NULL,
// dropped too ([n] otherwise).  Returns the number of records, or LPCN_E_ARG (negative count or skip, a total beyond INT_MAX, ring positions
// out of order) with ctl untouched; *any_dropped (may be NULL) says whether a vector was dropped.
int plc_fec_feed_plan(int n, lpcn_plc_ctl *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped, int *any_dropped,
                      char *err, size_t err_len);
