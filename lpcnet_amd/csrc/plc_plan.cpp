// The host half of the packet-loss concealment (plc_plan.h): no device, no HIP.
#include <stdio.h>
#include <string.h>
#include "plc_plan.h"
using namespace lpcn;
#define LPCNET_PLC_CAUSAL_OPT 0      /* LPCNET_PLC_CAUSAL of include/lpcnet.h (2 = LPCNET_PLC_CODEC, | 4 = LPCNET_PLC_DC_FILTER) */

extern "C" void lpcn_plc_ctl_reset(lpcn_plc_ctl *c)
{
    memset(c, 0, sizeof(*c));
    c->pcm_fill = LPCN_PLC_BUF_SIZE;      // src/lpcnet_plc.c:52-58
}

// get_fec_or_pred's decision and bookkeeping (src/lpcnet_plc.c:148-168)
static bool plc_take_fec(lpcn_plc_ctl &c, int *row)
{
    if (c.fec_read != c.fec_fill && c.fec_skip == 0) {
        *row = c.fec_read++;
        const int k = c.fec_read - LPCN_FEATURES_DELAY - 1;
        c.fec_keep = c.fec_keep > k ? c.fec_keep : k;
        if (c.fec_keep < 0) c.fec_keep = 0;
        return true;
    }
    if (c.fec_skip > 0) c.fec_skip--;
    *row = 0;
    return false;
}

extern "C" int lpcn_plc_ctl_fec_add(lpcn_plc_ctl *c, int is_null)      // src/lpcnet_plc.c:109-127
{
    if (is_null) { c->fec_skip++; return 0; }
    int moved = 0;
    if (c->fec_fill == LPCN_PLC_MAX_FEC) {
        if (c->fec_keep == 0) return 1;
        c->fec_fill -= c->fec_keep;
        c->fec_read -= c->fec_keep;
        c->fec_keep = 0;
        moved = 2;
    }
    c->fec_fill++;
    return moved;
}

int plc_fec_feed_plan(int n, lpcn_plc_ctl *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped, int *any_dropped,
                      char *err, size_t err_len)
{
    long long total = 0;
    for (int s = 0; s < n; ++s) {      // (everything is checked before anything changes)
        const lpcn_plc_ctl &c = ctl[s];
        if (count[s] < 0 || (skip && skip[s] < 0)) { snprintf(err, err_len, "FEC feed: stream %d has a negative count", s); return LPCN_E_ARG; }
        if (c.fec_keep < 0 || c.fec_keep > c.fec_read || c.fec_read > c.fec_fill || c.fec_fill > LPCN_PLC_MAX_FEC || c.fec_skip < 0 ||
            (skip && skip[s] > 0x7fffffff - c.fec_skip)) {
            snprintf(err, err_len, "stream %d: inconsistent PLC control state", s); return LPCN_E_ARG;
        }
        if ((total += count[s]) > 0x7fffffff) { snprintf(err, err_len, "FEC feed: more than 2^31 - 1 vectors"); return LPCN_E_ARG; }
    }
    int n_rec = 0, off = 0, any = 0;
    for (int s = 0; s < n; ++s) {
        lpcn_plc_ctl &c = ctl[s];
        if (clear && clear[s]) c.fec_keep = c.fec_read = c.fec_fill = c.fec_skip = 0;      // src/lpcnet_plc.c:130-132
        if (skip) c.fec_skip += skip[s];
        int left = count[s];
        const int room = LPCN_PLC_MAX_FEC - c.fec_fill, a = left < room ? left : room, at_a = c.fec_fill;
        c.fec_fill += a; left -= a;
        int from = 0, rows = 0, b = 0, at_b = 0;
        if (left > 0 && c.fec_keep > 0) {      // the ring is full and has rows to give up: :116-125, once
            from = c.fec_keep; rows = LPCN_PLC_MAX_FEC - from; at_b = rows;
            b = left < from ? left : from;
            c.fec_read -= from; c.fec_keep = 0; c.fec_fill = rows + b;
            left -= b;
        }
        if (dropped) dropped[s] = left;      // "FEC buffer full", :117-120
        any |= left > 0;
        if (a + b > 0) {
            const int r[PLC_FEED_REC] = {s, off, a, at_a, from, rows, b, at_b};
            memcpy(rec + (size_t)n_rec++ * PLC_FEED_REC, r, sizeof(r));
        }
        off += count[s];
    }
    if (any_dropped) *any_dropped = any;
    return n_rec;
}

static void plc_emit(PlcPlan &P, int type, int op, const std::vector<int> &recs, int rec_size)
{
    if (recs.empty()) return;
    PlcLaunch L;
    L.type = type; L.op = op; L.off = (int)P.ctl.size(); L.cnt = (int)recs.size() / rec_size;
    P.ctl.insert(P.ctl.end(), recs.begin(), recs.end());
    P.launches.push_back(L);
}
static void plc_emit_group(PlcPlan &P, const std::vector<int> &map, int kind, int N, int preload, int feat_src, int pcm_src, int pcm_dst, int pcm_off, bool scatter, bool keep)
{
    if (map.empty()) return;
    PlcLaunch L;
    L.type = PLC_T_GROUP; L.off = (int)P.ctl.size(); L.cnt = (int)map.size();
    L.kind = kind; L.N = N; L.preload = preload; L.feat_src = feat_src; L.pcm_src = pcm_src; L.pcm_dst = pcm_dst; L.pcm_off = pcm_off; L.scatter = scatter; L.keep = keep;
    P.ctl.insert(P.ctl.end(), map.begin(), map.end());
    P.launches.push_back(L);
}

int plc_plan(int options, int n, lpcn_plc_ctl *ctl, const unsigned char *lost, PlcPlan &P, int *summary, char *err, size_t err_len, int lanes)
{
    if (lanes < 1 || lanes > PLC_MAX_LANES) { snprintf(err, err_len, "PLC plan: lanes must be 1 .. %d", PLC_MAX_LANES); return LPCN_E_ARG; }
    const bool blending = (options & 3) == LPCNET_PLC_CAUSAL_OPT, remove_dc = (options & 4) != 0;
    static const float att_table[10] = {0, 0, -.2, -.2, -.4, -.4, -.8, -.8, -1.6, -1.6};      // src/lpcnet_plc.c:295
    P.ctl.clear(); P.launches.clear();
    for (int s = 0; s < n; ++s) {
        const lpcn_plc_ctl &c = ctl[s];
        const bool fill_ok = c.pcm_fill == 0 || c.pcm_fill == 80 || c.pcm_fill == 240 || c.pcm_fill == LPCN_PLC_BUF_SIZE;
        if (!fill_ok || (!lost[s] && c.skip_analysis && !c.blend && c.pcm_fill + LPCN_FRAME_SIZE > LPCN_PLC_BUF_SIZE) || c.fbuf_fill < 0 || c.fbuf_fill > LPCN_PLC_FBUF ||
            c.fec_keep < 0 || c.fec_keep > c.fec_read || c.fec_read > c.fec_fill || c.fec_fill > LPCN_PLC_MAX_FEC || c.fec_skip < 0 || c.skip_analysis < 0 || c.loss_count < 0) {
            snprintf(err, err_len, "stream %d: inconsistent PLC control state", s); return LPCN_E_ARG;
        }
    }
    // the lost streams' lists, per chain: chain c holds the streams that take c queue rounds in this step (one lane: everything is chain 0)
    struct LostChain { std::vector<int> flush[LPCN_PLC_FBUF], rpred[3], r160[3], r80[3], rshift[3], fpred, lostmap; };
    LostChain chain[4];
    std::vector<int> dclost;
    std::vector<int> burg, bpred, fa1, fa2, resetsig, xgrp, xfade, qtail, qappend, post_pred, fa3, qpush, dcrecv;
    int zero[LPCN_PLC_SUMMARY];
    for (int s = 0; s < n; ++s) {
        lpcn_plc_ctl &c = ctl[s];
        int *sm = summary ? summary + (size_t)s * LPCN_PLC_SUMMARY : zero;
        memset(sm, 0, sizeof(int) * LPCN_PLC_SUMMARY);
        if (lost[s]) {                                       // lpcnet_plc_conceal_causal, src/lpcnet_plc.c:296-340
            sm[0] = 1; sm[1] = c.fbuf_fill;
            int rounds = 0;
            for (int left = c.pcm_fill; left > 0 && rounds < 3; ++rounds) left -= left < LPCN_FRAME_SIZE ? left : LPCN_FRAME_SIZE;
            LostChain &ch = chain[lanes > 1 ? rounds : 0];
            std::vector<int> *const flush = ch.flush, *const rpred = ch.rpred, *const r160 = ch.r160, *const r80 = ch.r80, *const rshift = ch.rshift;
            std::vector<int> &fpred = ch.fpred, &lostmap = ch.lostmap;
            for (int k = 0; k < c.fbuf_fill; ++k) flush[k].push_back(s);
            c.fbuf_fill = 0;
            for (int r = 0; c.pcm_fill > 0 && r < 3; ++r) {
                const int N = c.pcm_fill < LPCN_FRAME_SIZE ? c.pcm_fill : LPCN_FRAME_SIZE;
                int row = 0;
                const bool fec = plc_take_fec(c, &row);
                const int fl = PLC_F_ROT | ((fec ? PLC_IN_FEC : PLC_IN_ZEROS) << PLC_F_INPUT_SHIFT) | PLC_F_COMPUTE | (fec ? 0 : PLC_F_KEEP);
                const int rec[PLC_PRED_REC] = {s, fl, row, 0, 0, 0};
                rpred[r].insert(rpred[r].end(), rec, rec + PLC_PRED_REC);
                (N == LPCN_FRAME_SIZE ? r160 : r80)[r].push_back(s);
                const int mr[PLC_MIX_REC] = {s, 0, 0};
                rshift[r].insert(rshift[r].end(), mr, mr + PLC_MIX_REC);
                c.pcm_fill -= N;
                c.skip_analysis++;
                sm[2]++; sm[3] += N; sm[4] += fec ? 1 : 0;
            }
            int row = 0;
            const bool fec = plc_take_fec(c, &row);
            if (fec) c.loss_count = 0; else c.loss_count++;
            const float a1 = c.loss_count >= 10 ? att_table[9] : att_table[c.loss_count];
            const float a2 = c.loss_count >= 10 ? (float)(2 * (c.loss_count - 9)) : 0.f;
            const int fl = PLC_F_ROT | ((fec ? PLC_IN_FEC : PLC_IN_ZEROS) << PLC_F_INPUT_SHIFT) | PLC_F_COMPUTE | (fec ? 0 : PLC_F_KEEP) | PLC_F_ATT;
            const int rec[PLC_PRED_REC] = {s, fl, row, float_bits(a1), float_bits(a2), 0};
            fpred.insert(fpred.end(), rec, rec + PLC_PRED_REC);
            lostmap.push_back(s);
            c.blend = 1;
            sm[4] += fec ? 1 : 0; sm[9] = c.loss_count;
            const int mr[PLC_MIX_REC] = {s, 0, 0};
            if (remove_dc) dclost.insert(dclost.end(), mr, mr + PLC_MIX_REC);
            continue;
        }
        // lpcnet_plc_update_causal, src/lpcnet_plc.c:188-290
        burg.push_back(s);
        const int mr[PLC_MIX_REC] = {s, 0, 0};
        if (c.skip_analysis) {
            if (c.blend) {
                if (blending) {
                    const int rec[PLC_PRED_REC] = {s, (2 << PLC_F_RESTORE_SHIFT) | (PLC_IN_BURG << PLC_F_INPUT_SHIFT) | PLC_F_COMPUTE | PLC_F_KEEP, 0, 0, 0, 0};
                    bpred.insert(bpred.end(), rec, rec + PLC_PRED_REC);
                    for (int k = 0; k < LPCN_FEATURES_DELAY; ++k) {
                        const int fr[PLC_MIX_REC] = {s, c.fbuf_fill, 0};
                        std::vector<int> &fa = k ? fa2 : fa1;
                        fa.insert(fa.end(), fr, fr + PLC_MIX_REC);
                        if (c.fbuf_fill < LPCN_PLC_FBUF) c.fbuf_fill++;
                    }
                    const int xr[PLC_MIX_REC] = {s, (int)xgrp.size(), 0};
                    xfade.insert(xfade.end(), xr, xr + PLC_MIX_REC);
                    xgrp.push_back(s);
                    sm[5] = 1; sm[8] += LPCN_FEATURES_DELAY;
                } else {
                    const int rec[PLC_PRED_REC] = {s, 1 << PLC_F_RESTORE_SHIFT, 0, 0, 0, 0};
                    bpred.insert(bpred.end(), rec, rec + PLC_PRED_REC);
                    c.fec_read -= LPCN_FEATURES_DELAY;                      // fec_rewind, :170-175
                    if (c.fec_read < c.fec_keep) c.fec_read = c.fec_keep;
                    resetsig.insert(resetsig.end(), mr, mr + PLC_MIX_REC);
                    sm[5] = 2;
                }
                qtail.insert(qtail.end(), mr, mr + PLC_MIX_REC);
                c.pcm_fill = 80;
                sm[6] = 1;
            } else {
                const int qr[PLC_MIX_REC] = {s, c.pcm_fill, 0};
                qappend.insert(qappend.end(), qr, qr + PLC_MIX_REC);
                c.pcm_fill += LPCN_FRAME_SIZE;
                sm[6] = 2;
            }
        }
        if (!c.blend) {
            const int rec[PLC_PRED_REC] = {s, (PLC_IN_BURG_FEAT << PLC_F_INPUT_SHIFT) | PLC_F_COMPUTE | PLC_F_KEEP, 0, 0, 0, 0};
            post_pred.insert(post_pred.end(), rec, rec + PLC_PRED_REC);
            if (c.fec_skip) c.fec_skip--;
            else if (c.fec_read < c.fec_fill) c.fec_read++;
            const int k = c.fec_read - LPCN_FEATURES_DELAY - 1;
            c.fec_keep = c.fec_keep > k ? c.fec_keep : k;
            if (c.fec_keep < 0) c.fec_keep = 0;
            sm[7] = 1;
        }
        bool append = false;
        if (c.skip_analysis) {
            append = blending;
            c.skip_analysis--;
        } else {
            qpush.insert(qpush.end(), mr, mr + PLC_MIX_REC);
            append = true;
            sm[6] = 3;
        }
        if (append) {
            const int fr[PLC_MIX_REC] = {s, c.fbuf_fill, 1};
            fa3.insert(fa3.end(), fr, fr + PLC_MIX_REC);
            if (c.fbuf_fill < LPCN_PLC_FBUF) c.fbuf_fill++;
            sm[8]++;
        }
        c.loss_count = 0;
        if (remove_dc) dcrecv.insert(dcrecv.end(), mr, mr + PLC_MIX_REC);
        c.blend = 0;
    }
    // lost streams, chain by chain: flush, the queued samples round by round, the concealed frame
    size_t chain_first[5];
    for (int c = 0; c < 4; ++c) {
        const LostChain &ch = chain[c];
        chain_first[c] = P.launches.size();
        for (int k = 0; k < LPCN_PLC_FBUF; ++k) plc_emit_group(P, ch.flush[k], LPCN_GROUP_FRAMES, LPCN_FRAME_SIZE, 0, 1 + k, 0, 0, 0, true, false);
        for (int r = 0; r < 3; ++r) {
            plc_emit(P, PLC_T_PRED, 0, ch.rpred[r], PLC_PRED_REC);
            plc_emit_group(P, ch.r160[r], LPCN_GROUP_FRAME_SAMPLES, LPCN_FRAME_SIZE, LPCN_FRAME_SIZE, 0, 1, 0, 0, true, true);
            plc_emit_group(P, ch.r80[r], LPCN_GROUP_FRAME_SAMPLES, 80, 80, 0, 1, 0, 0, true, true);
            plc_emit(P, PLC_T_MIX, PLC_MIX_QSHIFT, ch.rshift[r], PLC_MIX_REC);
        }
        plc_emit_group(P, ch.lostmap, LPCN_GROUP_TAIL, 80, 0, 0, 0, 1, 0, true, false);
        plc_emit(P, PLC_T_PRED, 0, ch.fpred, PLC_PRED_REC);
        plc_emit_group(P, ch.lostmap, LPCN_GROUP_FRAME_SAMPLES, 80, 0, 0, 0, 1, 80, true, true);
    }
    chain_first[4] = P.launches.size();
    // received streams up to the analysis
    if (!burg.empty()) { plc_emit(P, PLC_T_BURG, 0, burg, 1); }
    plc_emit(P, PLC_T_PRED, 0, bpred, PLC_PRED_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_FAPPEND, fa1, PLC_MIX_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_FAPPEND, fa2, PLC_MIX_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_RESETSIG, resetsig, PLC_MIX_REC);
    plc_emit_group(P, xgrp, LPCN_GROUP_FRAME_SAMPLES, 80, 0, 0, 0, 0, 0, false, false);      // into the group's PCM; the states are not written back (the reference's copy / restore)
    plc_emit(P, PLC_T_MIX, PLC_MIX_XFADE, xfade, PLC_MIX_REC);
    plc_emit_group(P, xgrp, LPCN_GROUP_FRAME_SAMPLES, 80, 80, 0, 2, 0, 0, true, true);
    plc_emit(P, PLC_T_MIX, PLC_MIX_QTAIL, qtail, PLC_MIX_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_QAPPEND, qappend, PLC_MIX_REC);
    if (lanes > 1) {
        // the chains onto the lanes: by the sample steps they take, longest first, each onto the lane with the least so far (lane 0 starts with the
        // received streams' chain); then one range of group rows per lane, as long as the lane's largest group -- the lanes hold disjoint streams,
        // so the ranges fit the n rows
        auto steps = [&](size_t first, size_t last) { int t = 0; for (size_t k = first; k < last; ++k) if (P.launches[k].type == PLC_T_GROUP && P.launches[k].kind != LPCN_GROUP_FRAMES) t += P.launches[k].N; return t; };
        int load[PLC_MAX_LANES] = {steps(chain_first[4], P.launches.size())}, cost[4];
        bool dealt[4] = {false, false, false, false};
        for (int c = 0; c < 4; ++c) cost[c] = steps(chain_first[c], chain_first[c + 1]);
        for (int pass = 0; pass < 4; ++pass) {
            int c = -1, l = 0;
            for (int k = 0; k < 4; ++k) if (!dealt[k] && chain_first[k + 1] > chain_first[k] && (c < 0 || cost[k] > cost[c])) c = k;
            if (c < 0) break;
            for (int k = 1; k < lanes; ++k) if (load[k] < load[l]) l = k;
            for (size_t k = chain_first[c]; k < chain_first[c + 1]; ++k) P.launches[k].lane = l;
            load[l] += cost[c]; dealt[c] = true;
        }
        int rows[PLC_MAX_LANES] = {0, 0, 0, 0}, base[PLC_MAX_LANES];
        for (const PlcLaunch &L : P.launches) if (L.type == PLC_T_GROUP && L.cnt > rows[L.lane]) rows[L.lane] = L.cnt;
        for (int l = 0, at = 0; l < PLC_MAX_LANES; ++l) { base[l] = at; at += rows[l]; }
        for (PlcLaunch &L : P.launches) L.slot = base[L.lane];
    }
    { PlcLaunch L; L.type = PLC_T_ANALYSIS; P.launches.push_back(L); }
    plc_emit(P, PLC_T_PRED, 0, post_pred, PLC_PRED_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_FAPPEND, fa3, PLC_MIX_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_QPUSH, qpush, PLC_MIX_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_DCRECV, dcrecv, PLC_MIX_REC);
    plc_emit(P, PLC_T_MIX, PLC_MIX_DCLOST, dclost, PLC_MIX_REC);
    return 0;
}

// The planner with lanes as plain arrays (lpcnet_hip_plc_plan_lanes of include/lpcnet_batch.h): launch[k] = {type, op, lane, slot, cnt, offset of its
// records in lists, ints per record, kind, N, preload}.  Returns the number of launches, or LPCN_E_ARG (message in err) when the arguments or the
// control state are bad or an output array is too short.
extern "C" int lpcn_plc_plan_lanes(int options, int n, int lanes, lpcn_plc_ctl *ctl, const unsigned char *lost, int *summary, int *launch, int launch_cap,
                                   int *lists, int lists_cap, char *err, size_t err_len)
{
    if (n < 1 || !ctl || !lost || !launch || !lists || launch_cap < 0 || lists_cap < 0 || (options & 3) == 1 || (options & 3) == 3 || (options & ~7)) {
        snprintf(err, err_len, "bad PLC plan arguments"); return LPCN_E_ARG;
    }
    PlcPlan P;
    std::vector<lpcn_plc_ctl> before(ctl, ctl + n);
    const int rc = plc_plan(options, n, ctl, lost, P, summary, err, err_len, lanes);
    if (rc) return rc;
    if (P.launches.size() > (size_t)launch_cap || P.ctl.size() > (size_t)lists_cap) {
        memcpy(ctl, before.data(), sizeof(lpcn_plc_ctl) * (size_t)n);      // (nothing has happened)
        snprintf(err, err_len, "PLC plan: %zu launches and %zu list entries do not fit the arrays given", P.launches.size(), P.ctl.size()); return LPCN_E_ARG;
    }
    for (size_t k = 0; k < P.launches.size(); ++k) {
        const PlcLaunch &L = P.launches[k];
        const int r[PLC_LANES_REC] = {L.type, L.op, L.lane, L.slot, L.cnt, L.off, plc_rec_size(L), L.kind, L.N, L.preload};
        memcpy(launch + k * PLC_LANES_REC, r, sizeof(r));
    }
    if (!P.ctl.empty()) memcpy(lists, P.ctl.data(), sizeof(int) * P.ctl.size());
    return (int)P.launches.size();
}

// Records per workgroup of a prediction launch over n_records records on a device of `cus` compute units (engine_plc.hip: launch_plc_pred), for a PLC
// network of widths d1 / g1 / g2, float or int8.  pinned: 1, 2, 4 or 8, or 0 for the table.  Either way halved until the form's LDS (plc_records.h:
// plc_pred_lds_bytes) fits a CU's.  LPCN_E_ARG for anything else.
// The table, as measured on one MI355X (profiles/plc_pred_forms.json) -- it is NOT the DRED kernels' rule.  A workgroup is four waves,
// one per SIMD, and its time is that of its dependent add chains, so a CU has to hold several workgroups to be busy: a form pays while four of its
// workgroups still share a CU's LDS (40 KB each) and there are records enough to fill those four places on every CU: the table is the largest such
// form, else one record per workgroup.  On 256 CUs that is 1 below 2 K records (measured at 256, 512 and 1 024: the fastest or within the run's
// spread of it), 2 from 2 K (measured at 2 048: the fastest in every row), and from 4 K and 8 K on also 4 and 8 where the LDS allows: at 8 192 records 8 at
// widths 128 / 16 / 16, 4 at 128 / 256 / 256 and 2 at 512 / 512 / 512, each the fastest pinned form of its row.
constexpr int PLC_PRED_FORM_SHARE = 4;
extern "C" int lpcn_plc_pred_form(int n_records, int cus, int d1, int g1, int g2, int int8, int pinned)
{
    if (pinned != 0 && pinned != 1 && pinned != 2 && pinned != 4 && pinned != 8) return LPCN_E_ARG;
    if (n_records < 0 || cus < 1 || d1 < 1 || g1 < 1 || g2 < 1) return LPCN_E_ARG;
    int S = pinned;
    if (!S) {
        S = 1;
        for (int k = 2; k <= 8; k *= 2)
            if (plc_pred_lds_bytes(k, d1, g1, g2, int8 != 0) <= PLC_PRED_FORM_LDS_LIMIT / PLC_PRED_FORM_SHARE && (n_records + k - 1) / k >= (long long)PLC_PRED_FORM_SHARE * cus) S = k;
    }
    while (S > 1 && plc_pred_lds_bytes(S, d1, g1, g2, int8 != 0) > PLC_PRED_FORM_LDS_LIMIT) S /= 2;
    return S;
}

