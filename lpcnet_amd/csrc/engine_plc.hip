// Compacted groups, their lanes and schedule, the per-stream step, packet-loss concealment and its FEC feed.  Owns plc_kernels.hip.h.
#include "engine_core.h"
#include "plc_kernels.hip.h"
#include <mutex>

// ---- compacted groups: a subset of the batch's streams through the ordinary frame and sample kernels (the per-stream-arguments step below
// and the packet-loss concealment, whose streams take different branches in one step).  The streams of a group are named by an index map on
// the device; their states, their features or kept frame products and their imposed PCM are gathered into dense arrays by small kernels,
// the launch runs on those in the batch's form -- or, under the group schedule, the cost table's form for the group's size (group_shape) -- and
// the results are scattered back by the same map: the hot kernels stay untouched.  A group runs the sample kernel far below its throughput.
// the buffers every group uses: the compacted states, features and PCM, and every stream's most recent frame products (zero until a stream has some)
int group_alloc(lpcn_batch_dev *b)
{
    if (b->d_keep_lpc) return 0;      // (the last one allocated)
    const size_t n = (size_t)b->n;
    int rc = 0;
    if ((rc = b->d_state_tmp.alloc(n)) || (rc = b->d_gfeat.alloc(n * LPCN_NB_FEAT)) || (rc = b->d_gpcm.alloc(n * LPCN_FRAME_SIZE)) || (rc = b->d_map.alloc(n)) ||
        (rc = b->d_keep_a.alloc(n * LPCN_ROWS_A, true)) || (rc = b->d_keep_b.alloc(n * LPCN_ROWS_B, true))) return rc;
    return b->d_keep_lpc.alloc(n * LPCN_LPC_ORDER, true);
}

// What one group runs (LPCN_GROUP_*): FRAMES the frame network alone, FRAME_SAMPLES the frame network and N samples (lpcnet_synthesize_impl,
// src/lpcnet.c:273-277), TAIL N samples from the products of each stream's most recent kept frame (lpcnet_synthesize_tail_impl, :235-271).
// Per-stream rows are given as (pointer, stride in elements): stream s's row starts at pointer + s * stride.
struct GroupRun {
    const int *map;                    // device: the group's stream indices
    int cnt, kind, N, preload;         // streams; LPCN_GROUP_*; samples per frame and how many of them are imposed
    const float *feat;                 // kinds with a frame step: every stream's feature vector
    size_t feat_stride;
    const short *pcm_src;              // the samples to impose (NULL: none are gathered)
    size_t pcm_src_stride;
    short *pcm_dst;                    // where the N samples go (NULL: they stay in the compacted d_gpcm, e.g. for a cross-fade)
    size_t pcm_dst_stride;
    bool keep;                         // remember the frame products per stream (lpcnet->gru_a_condition, gru_b_condition, lpc of the reference's state)
    bool scatter;                      // write the states back (false: a trial run)
    int slot = 0, lane = 0;            // the group's rows of the group buffers: [slot, slot + cnt); the lane it was dealt to (for lpcn_batch_dev_last_groups)
};
// The form a compacted group of cnt streams launches in.  Under the group schedule's `form`, with the batch's streams per workgroup chosen by
// the engine and PARITY arithmetic (every form gives the same bits there; FAST's output depends on the form), the cost table's form for cnt
// streams -- a table look-up, never a measurement -- and the twelve-wave form only where the batch already runs it at eight; else the batch's.
static LaunchShape group_shape(const lpcn_batch_dev *b, int cnt, int N, int slot)
{
    if (b->sched_form && b->S_auto && !b->e->fast) {
        const int S = auto_streams_per_wg(b, cnt);
        return {cnt, N, b->d_state_tmp + slot, S, use_pack2(b, cnt, S), S == 8 && b->S == 8 && b->x3, slot, 0};
    }
    return {cnt, N, b->d_state_tmp + slot, b->S, b->pack2, b->x3, slot, 0};
}
static bool aligned16(const void *p, size_t stride_bytes) { return ((uintptr_t)p | (uintptr_t)stride_bytes) % 16 == 0; }
// Enqueues only; the caller checks hipGetLastError() after its groups.  One gather launch, the frame and sample kernels on rows
// [slot, slot + cnt) of the group buffers, one scatter launch.
static int run_group(lpcn_batch_dev *b, hipStream_t st, const GroupRun &g)
{
    const int cnt = g.cnt;
    if (g.slot < 0 || cnt < 1 || g.slot + cnt > b->n) { snprintf(g_err, sizeof(g_err), "group rows [%d, %d) outside the batch", g.slot, g.slot + cnt); return LPCN_E_ARG; }
    LaunchShape sh = group_shape(b, cnt, g.N, g.slot);
    sh.arg = b->args_next;
    const SamplePlan sp = plan_sample(b, sh, 1);
    b->last_groups.push_back({{g.lane, g.slot, cnt, g.kind, g.N, g.preload, sp.S, sp.grid}});
    const bool frames = g.kind != LPCN_GROUP_TAIL, samples = g.kind != LPCN_GROUP_FRAMES;
    short *gpcm = b->d_gpcm + (size_t)g.slot * LPCN_FRAME_SIZE;
    lpcn::GroupRows r{};
    r.map = g.map; r.cnt = cnt;
    r.states = b->d_state; r.gstates = sh.d_state;
    r.gfeat = b->d_gfeat + (size_t)g.slot * LPCN_NB_FEAT;
    r.keep_a = b->d_keep_a; r.keep_b = b->d_keep_b; r.keep_lpc = b->d_keep_lpc;
    r.cond_a = b->d_cond_a + (size_t)g.slot * LPCN_ROWS_A; r.cond_b = b->d_cond_b + (size_t)g.slot * LPCN_ROWS_B; r.lpc = b->d_lpc + (size_t)g.slot * LPCN_LPC_ORDER;
    r.gpcm = gpcm; r.N = g.N;
    lpcn::GroupRows in = r;
    if (frames) { in.feat = g.feat; in.feat_stride = g.feat_stride; in.feat_vec = aligned16(g.feat, g.feat_stride * sizeof(float)); }
    in.keep = frames ? 0 : 1;
    if (samples && g.pcm_src) { in.pcm = const_cast<short *>(g.pcm_src); in.pcm_stride = g.pcm_src_stride; in.pcm_vec = aligned16(g.pcm_src, g.pcm_src_stride * sizeof(short)); }
    hipLaunchKernelGGL(lpcn::group_gather_kernel, dim3(cnt), dim3(lpcn::PLC_GROUP_THREADS), 0, st, in);
    int rc = 0;
    if (frames && (rc = launch_frames(b, sh, st, r.gfeat, LPCN_NB_FEAT, (size_t)LPCN_NB_FEAT, 1))) return rc;
    if (samples) {
        if ((rc = launch_sample(b, sh, st, gpcm, (size_t)LPCN_FRAME_SIZE, 1, g.preload, frames))) return rc;
        b->args_next++;
    }
    lpcn::GroupRows out = r;
    if (samples && g.pcm_dst) { out.pcm = g.pcm_dst; out.pcm_stride = g.pcm_dst_stride; out.pcm_vec = aligned16(g.pcm_dst, g.pcm_dst_stride * sizeof(short)); }
    out.keep = frames && g.keep ? 1 : 0;
    out.state_back = g.scatter ? 1 : 0;
    if (out.pcm || out.keep || out.state_back)
        hipLaunchKernelGGL(lpcn::group_scatter_kernel, dim3(cnt), dim3(lpcn::PLC_GROUP_THREADS), 0, st, out);
    return 0;
}
// The lanes of a step: lane 0 is the caller's stream, lanes 1 .. are the batch's own streams.  lanes_fork lets them start after what the caller's
// stream holds so far (the step's uploads); lanes_join makes the caller's stream wait for every lane that was given work.
struct Lanes {
    hipStream_t st[PLC_MAX_LANES];
    bool used[PLC_MAX_LANES] = {false, false, false, false};
    bool forked = false;
};
static int lanes_use(lpcn_batch_dev *b, Lanes &ln, int lane, hipStream_t *out)
{
    if (lane < 0 || lane >= b->sched_lanes) { snprintf(g_err, sizeof(g_err), "lane %d of %d", lane, b->sched_lanes); return LPCN_E_ARG; }
    if (lane > 0 && !ln.used[lane]) {
        if (!ln.forked) { HIP_TRY(hipEventRecord(b->ev_fork, ln.st[0])); ln.forked = true; }
        HIP_TRY(hipStreamWaitEvent(ln.st[lane], b->ev_fork, 0));
        ln.used[lane] = true;
    }
    *out = ln.st[lane];
    return 0;
}
static Lanes lanes_begin(lpcn_batch_dev *b, hipStream_t st)
{
    Lanes ln;
    ln.st[0] = st;
    for (int l = 1; l < PLC_MAX_LANES; ++l) ln.st[l] = b->side[l - 1];
    return ln;
}
static int lanes_join(lpcn_batch_dev *b, Lanes &ln)
{
    for (int l = 1; l < PLC_MAX_LANES; ++l)
        if (ln.used[l]) {
            HIP_TRY(hipEventRecord(b->ev_join[l - 1], ln.st[l]));
            HIP_TRY(hipStreamWaitEvent(ln.st[0], b->ev_join[l - 1], 0));
            ln.used[l] = false;
        }
    ln.forked = false;
    return 0;
}

extern "C" int lpcn_batch_dev_set_group_schedule(lpcn_batch_dev *b, int form, int lanes)
{
    if (form < 0 || form > 1 || lanes < 1 || lanes > PLC_MAX_LANES) { snprintf(g_err, sizeof(g_err), "group schedule: form must be 0 or 1 and lanes 1 .. %d", PLC_MAX_LANES); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (lanes > 1 && !b->ev_fork.e) {
        // (each handle is made once: a call that failed part-way is completed by the next one)
        for (auto &sd : b->side) if (!sd.s && hipStreamCreateWithFlags(&sd.s, hipStreamNonBlocking) != hipSuccess) { snprintf(g_err, sizeof(g_err), "group schedule: hipStreamCreate failed"); return LPCN_E_HIP; }
        for (auto &ev : b->ev_join) if (!ev.e && hipEventCreateWithFlags(&ev.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "group schedule: hipEventCreate failed"); return LPCN_E_HIP; }
        if (hipEventCreateWithFlags(&b->ev_fork.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "group schedule: hipEventCreate failed"); return LPCN_E_HIP; }
    }
    b->sched_form = form; b->sched_lanes = lanes;
    return 0;
}
extern "C" int lpcn_batch_dev_get_group_schedule(const lpcn_batch_dev *b, int *form, int *lanes)
{
    if (form) *form = b->sched_form;
    if (lanes) *lanes = b->sched_lanes;
    return 0;
}
extern "C" int lpcn_batch_dev_group_form(const lpcn_batch_dev *b, int cnt)
{
    if (cnt < 1 || cnt > b->n) { snprintf(g_err, sizeof(g_err), "group form: 1 .. %d streams", b->n); return LPCN_E_ARG; }
    return plan_sample(b, group_shape(b, cnt, LPCN_FRAME_SIZE, 0), 1).S;
}
extern "C" int lpcn_batch_dev_last_groups(const lpcn_batch_dev *b, int *rec, int cap)
{
    const int k = (int)b->last_groups.size();
    for (int i = 0; rec && i < k && i < cap; ++i) memcpy(rec + (size_t)i * 8, b->last_groups[(size_t)i].v, sizeof(int) * 8);
    return k;
}

// ---- one frame step with PER-STREAM arguments (src/lpcnet_plc.c calls lpcnet_synthesize_impl(N = TRAINING_OFFSET, preload),
// lpcnet_synthesize_tail_impl(N, preload) and plain frames per stream, depending on which of its streams lost a packet).  mode[s]: 0 = leave
// the stream alone, 1 = frame network on features[s] + n_samples[s] samples, 2 = n_samples[s] samples from the products of the stream's most
// recent frame; the first preload[s] samples of pcm[s] are imposed (teacher forcing).  Streams with equal (mode, n_samples, preload) form a
// group.  The call's features and PCM go up once, the groups run one after the other (run_group), the PCM comes back once.
extern "C" int lpcn_batch_dev_step_host(lpcn_batch_dev *b, const float *features, int feat_stride, short *pcm,
                                        const int *n_samples, const int *preload, const int *mode)
{
    if (!features || !pcm || !n_samples || !preload || !mode || feat_stride < LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "bad step arguments"); return LPCN_E_ARG; }
    const int na = b->active;          // (the arguments of the streams beyond the active prefix are not looked at: those streams are left alone, like mode 0)
    for (int s = 0; s < na; ++s) {
        if (mode[s] < 0 || mode[s] > 2) { snprintf(g_err, sizeof(g_err), "stream %d: mode must be 0, 1 or 2", s); return LPCN_E_ARG; }
        if (mode[s] && (n_samples[s] < 1 || n_samples[s] > LPCN_FRAME_SIZE || preload[s] < 0 || preload[s] > n_samples[s])) {
            snprintf(g_err, sizeof(g_err), "stream %d: n_samples must be 1..160 and preload 0..n_samples", s); return LPCN_E_ARG;
        }
    }
    // a tail-only step continues the frame of the stream's last mode-1 step: the reference's lpcnet_synthesize_tail_impl uses
    // whatever the last run_frame_network left in the state, but this engine keeps frame products per stream only for
    // steps that went through this call -- a stream advanced by the ordinary synthesize / decode calls has none
    if (b->keep_ok.size() != (size_t)b->n) b->keep_ok.assign((size_t)b->n, 0);
    for (int s = 0; s < na; ++s)
        if (mode[s] == 2 && !b->keep_ok[s]) {
            snprintf(g_err, sizeof(g_err), "stream %d: a tail-only step (mode 2) needs a preceding frame step (mode 1) of lpcnet_batch_synthesize_step", s);
            return LPCN_E_ARG;
        }
    if (!na) return 0;
    DeviceGuard guard(b->e->device);
    const size_t nfeat = (size_t)(na - 1) * feat_stride + LPCN_NB_FEAT, npcm = (size_t)na * LPCN_FRAME_SIZE;
    int rc = ensure_staging(b, nfeat, npcm);
    if (!rc) rc = group_alloc(b);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    if ((rc = tune_if_due(b, st))) return rc;
    struct Group { int off, cnt, mode, N, preload; };      // (off: the group's place in `map`, which holds every group's streams)
    std::vector<Group> groups;
    std::vector<int> map;
    std::vector<char> done((size_t)na, 0);
    for (int s0 = 0; s0 < na; ++s0) {
        if (done[s0] || mode[s0] == 0) continue;
        const int off = (int)map.size();
        for (int s = s0; s < na; ++s)
            if (!done[s] && mode[s] == mode[s0] && n_samples[s] == n_samples[s0] && preload[s] == preload[s0]) { map.push_back(s); done[s] = 1; }
        groups.push_back({off, (int)map.size() - off, mode[s0], n_samples[s0], preload[s0]});
    }
    if (groups.empty()) return 0;
    HIP_TRY(hipMemcpyAsync(b->d_map, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_feat, features, sizeof(float) * nfeat, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_pcm, pcm, sizeof(short) * npcm, hipMemcpyHostToDevice, st));
    b->args_next = 0; b->last_groups.clear();
    Lanes ln = lanes_begin(b, st);
    int next_lane = 0;
    for (const Group &g : groups) {
        // (only the first N samples of a stream's frame are written: the rest of d_pcm, and the streams of mode 0, go back as they came)
        // The groups hold disjoint streams: with more than one lane they are dealt round-robin, each in the rows of its own place in the map.
        const int lane = next_lane, slot = b->sched_lanes > 1 ? g.off : 0;
        next_lane = (next_lane + 1) % b->sched_lanes;
        hipStream_t lst = st;
        if ((rc = lanes_use(b, ln, lane, &lst))) return rc;
        const GroupRun r = {b->d_map + g.off, g.cnt, g.mode == 1 ? LPCN_GROUP_FRAME_SAMPLES : LPCN_GROUP_TAIL, g.N, g.preload, b->d_feat, (size_t)feat_stride,
                            g.preload > 0 ? b->d_pcm.p : nullptr, (size_t)LPCN_FRAME_SIZE, b->d_pcm, (size_t)LPCN_FRAME_SIZE, g.mode == 1, true, slot, lane};
        if ((rc = run_group(b, lst, r))) { (void)lanes_join(b, ln); return rc; }
    }
    if ((rc = lanes_join(b, ln))) return rc;
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "per-stream step: kernel launch failed"); return LPCN_E_HIP; }
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, sizeof(short) * npcm, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // only now do the streams of the mode-1 groups own frame products a later tail-only step may continue from (the flag used to
    // be set before the sample launch and the state scatter had succeeded)
    for (const Group &g : groups)
        if (g.mode == 1) for (int i = 0; i < g.cnt; ++i) b->keep_ok[(size_t)map[(size_t)g.off + i]] = 1;
    return 0;
}

// ------------------------------------------------------------------------------- packet-loss concealment -----
// lpcnet_plc_update / lpcnet_plc_conceal in causal mode for every stream (src/lpcnet_plc.c:188-340).  The host keeps the control
// state and plans every step (plc_plan.h: no device needed); the data stays on the device.  A step is one upload of the planner's lists and
// a fixed order of launches with no host synchronisation between them.
extern "C" int lpcn_plc_plan(int options, int n, lpcn_plc_ctl *ctl, const unsigned char *lost, int *summary)
{
    if (n < 1 || !ctl || !lost || (options & 3) == 1 || (options & 3) == 3 || (options & ~7)) { snprintf(g_err, sizeof(g_err), "bad PLC plan arguments"); return LPCN_E_ARG; }
    PlcPlan P;
    return plc_plan(options, n, ctl, lost, P, summary, g_err, sizeof(g_err));
}

extern "C" int lpcn_engine_plc_present(const lpcn_engine *e) { return e->plc_present; }
extern "C" int lpcn_batch_dev_plc_enabled(const lpcn_batch_dev *b) { return b->plc ? 1 : 0; }
extern "C" int lpcn_batch_dev_plc_flavour(const lpcn_batch_dev *b)
{
    if (!b->plc) { snprintf(g_err, sizeof(g_err), "packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; }
    return b->e->is_int8 ? 1 : 0;
}
// compute_plc_pred in the flavour of the engine's blob: the same records and data, the float or the int8 network
// ---- records per workgroup.  One workgroup per record reads the whole network through L2 for its one stream; the forms with S = 2, 4, 8 records per
// workgroup (plc_pred_s_kernel<S>) load a weight once for S streams.  The rule and the measurements behind it: plc_plan.cpp: lpcn_plc_pred_form,
// DESIGN.md §4.4.
static int plc_pred_d1(const lpcn_engine *e) { return e->is_int8 ? e->plcq.d1 : e->plc.d1; }
extern "C" int lpcn_batch_dev_plc_pred_form(const lpcn_batch_dev *b, int n)
{
    if (!b->plc) { snprintf(g_err, sizeof(g_err), "packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; }
    if (n < 0) { snprintf(g_err, sizeof(g_err), "PLC prediction form: a negative number of records"); return LPCN_E_ARG; }
    return lpcn_plc_pred_form(n, b->plc->cus, plc_pred_d1(b->e), plc_units(b->e, 0), plc_units(b->e, 1), b->e->is_int8 ? 1 : 0, b->plc->pred_form);
}
extern "C" int lpcn_batch_dev_plc_pred_set_form(lpcn_batch_dev *b, int S)
{
    if (!b->plc) { snprintf(g_err, sizeof(g_err), "packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; }
    if (S != 0 && S != 1 && S != 2 && S != 4 && S != 8) { snprintf(g_err, sizeof(g_err), "PLC prediction form: 1, 2, 4 or 8 records per workgroup, 0 = the table's choice"); return LPCN_E_ARG; }
    b->plc->pred_form = S;
    return 0;
}
template <int S, typename Net>
static int plc_pred_launch_form(const Net &P, int grid, int lds, hipStream_t st, const int *ctl, int cnt, const lpcn::PlcData &D, float *raw_out)
{
    // the dynamic-LDS limit of a form is raised once per (device, size), not at every launch
    static std::mutex mu;
    static int limit[64];
    const auto kernel = [] { if constexpr (std::is_same<Net, lpcn::PlcNet>::value) return lpcn::plc_pred_s_kernel<S>; else return lpcn::plc_pred_s_int8_kernel<S>; }();
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> g(mu);
        if (dev < 0 || dev >= 64 || limit[dev] < lds) {
            HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            if (dev >= 0 && dev < 64) limit[dev] = lds;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(lpcn::PLC_PRED_THREADS), lds, st, P, ctl, cnt, D, raw_out);
    return 0;
}
template <typename Net>
static int plc_pred_launch(const Net &P, int S, int lds, hipStream_t st, const int *ctl, int cnt, const lpcn::PlcData &D, float *raw_out)
{
    const int grid = (cnt + S - 1) / S;
    switch (S) {
    case 2: return plc_pred_launch_form<2>(P, grid, lds, st, ctl, cnt, D, raw_out);
    case 4: return plc_pred_launch_form<4>(P, grid, lds, st, ctl, cnt, D, raw_out);
    default: return plc_pred_launch_form<8>(P, grid, lds, st, ctl, cnt, D, raw_out);
    }
}
// compute_plc_pred in the flavour of the engine's blob: the same records and data, the float or the int8 network, in the form for `cnt` records.  The
// single launch site: the step's prediction phases and the parity seam.
static int launch_plc_pred(lpcn_batch_dev *b, hipStream_t st, const int *ctl, int cnt, float *raw_out)
{
    const lpcn_engine *e = b->e;
    const int S = lpcn_batch_dev_plc_pred_form(b, cnt);
    if (S < 0) return S;
    if (S > 1) {
        const int lds = lpcn::plc_pred_lds_bytes(S, plc_pred_d1(e), plc_units(e, 0), plc_units(e, 1), e->is_int8 ? 1 : 0);
        return e->is_int8 ? plc_pred_launch(e->plcq, S, lds, st, ctl, cnt, b->plc->D, raw_out) : plc_pred_launch(e->plc, S, lds, st, ctl, cnt, b->plc->D, raw_out);
    }
    if (e->is_int8) hipLaunchKernelGGL(lpcn::plc_pred_i8_kernel, dim3(cnt), dim3(lpcn::PLC_PRED_THREADS), 0, st, e->plcq, ctl, cnt, b->plc->D, raw_out);
    else hipLaunchKernelGGL(lpcn::plc_pred_kernel, dim3(cnt), dim3(lpcn::PLC_PRED_THREADS), 0, st, e->plc, ctl, cnt, b->plc->D, raw_out);
    return 0;
}
static size_t plc_net_floats(const lpcn_batch_dev *b) { return 4 * (size_t)(plc_units(b->e, 0) + plc_units(b->e, 1)); }
// lpcnet_plc_reset (src/lpcnet_plc.c:46-60) on streams [first, first + count): the PLC's own fields, the synthesis state, the analysis state
static int plc_reset_range(lpcn_batch_dev *b, int first, int count)
{
    lpcn_plc_host *p = b->plc.get();
    int rc = lpcn_batch_dev_reset(b, first, count);      // (waits for everything enqueued)
    if (!rc) rc = lpcn_batch_dev_analysis_reset(b, first, count);
    if (rc || !count) return rc;
    const size_t G4 = plc_net_floats(b);
#define ZR(buf, per) HIP_TRY(hipMemset((buf).p + (size_t)first * (per), 0, sizeof(*(buf).p) * (size_t)count * (per)))
    ZR(p->q, LPCN_PLC_QUEUE); ZR(p->feat, LPCN_NB_FEAT); ZR(p->net, G4); ZR(p->dc, 2); ZR(p->delta, 1);
    ZR(p->fec, LPCN_PLC_MAX_FEC * LPCN_NB_FEAT); ZR(p->fbuf, LPCN_PLC_FBUF * LPCN_NB_FEAT); ZR(p->lp, LPCN_FRAME_SIZE);
    ZR(p->burg, 2 * LPCN_NB_BANDS); ZR(p->an, LPCN_AN_NB_FEATURES);
    ZR(b->d_keep_a, LPCN_ROWS_A); ZR(b->d_keep_b, LPCN_ROWS_B); ZR(b->d_keep_lpc, LPCN_LPC_ORDER);
#undef ZR
    for (int s = first; s < first + count; ++s) lpcn_plc_ctl_reset(&p->ctl[s]);
    return 0;
}

extern "C" int lpcn_batch_dev_plc_enable(lpcn_batch_dev *b, int options)
{
    if ((options & 3) == 1 || (options & 3) == 3 || (options & ~7)) { snprintf(g_err, sizeof(g_err), "PLC options: LPCNET_PLC_CAUSAL or LPCNET_PLC_CODEC, optionally | LPCNET_PLC_DC_FILTER (the non-causal mode needs a model without feature delay)"); return LPCN_E_ARG; }
    if (b->e->plc_present == 0) { snprintf(g_err, sizeof(g_err), "the model blob has no PLC network (plc_dense1_*, plc_gru1_*, plc_gru2_*, plc_out_*)"); return LPCN_E_MODEL; }
    if (b->e->plc_present != 1 && b->e->plc_present != 2) { snprintf(g_err, sizeof(g_err), "the blob's PLC arrays are incomplete or do not fit together"); return LPCN_E_MODEL; }
    if (b->e->plc_present == 2 && !b->e->plc_servable) { snprintf(g_err, sizeof(g_err), "the blob's PLC network is int8 but its LPCNet model is float: a PLC network is served in its blob's own flavour"); return LPCN_E_MODEL; }
    if (!b->e->plc_servable) { snprintf(g_err, sizeof(g_err), "the blob's PLC network is float but its LPCNet model is int8: a PLC network is served in its blob's own flavour"); return LPCN_E_MODEL; }
    DeviceGuard guard(b->e->device);
    int rc = lpcn_batch_dev_analysis_enable(b, 1);
    if (rc) return rc;
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (!b->plc) {
        auto p = std::make_unique<lpcn_plc_host>();      // (a failure below frees what it holds; the batch stays without PLC)
        const size_t n = (size_t)b->n;
        if ((rc = p->q.alloc(n * LPCN_PLC_QUEUE)) || (rc = p->feat.alloc(n * LPCN_NB_FEAT)) || (rc = p->net.alloc(n * plc_net_floats(b))) || (rc = p->dc.alloc(n * 2)) ||
            (rc = p->delta.alloc(n)) || (rc = p->fec.alloc(n * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT)) || (rc = p->fbuf.alloc(n * LPCN_PLC_FBUF * LPCN_NB_FEAT)) ||
            (rc = p->lp.alloc(n * LPCN_FRAME_SIZE)) || (rc = p->burg.alloc(n * 2 * LPCN_NB_BANDS)) || (rc = p->an.alloc(n * LPCN_AN_NB_FEATURES)) ||
            (rc = p->d_pcm.alloc(n * LPCN_FRAME_SIZE)) || (rc = p->d_ident.alloc(n)) || (rc = p->d_ctl.alloc(64 * n + 64)) ||
            (rc = p->d_feed.alloc(lpcn::PLC_FEED_REC * n)) || (rc = p->h_ctl.reserve(sizeof(int) * (p->d_ctl.cap + p->d_feed.cap))) || (rc = group_alloc(b))) return rc;
        p->D = {p->q, p->feat, p->net, p->dc, p->delta, p->fec, p->fbuf, p->lp, p->burg, p->an};
        if (hipEventCreateWithFlags(&p->ev_ctl.e, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&p->ev_feed.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "PLC: hipEventCreate failed"); return LPCN_E_HIP; }
        std::vector<int> ident(n);
        for (size_t i = 0; i < n; ++i) ident[i] = (int)i;
        if (hipMemcpy(p->d_ident, ident.data(), sizeof(int) * n, hipMemcpyHostToDevice) != hipSuccess) { snprintf(g_err, sizeof(g_err), "PLC: upload failed"); return LPCN_E_HIP; }
        p->ctl.resize(n);
        b->plc = std::move(p);
    }
    b->plc->options = options; b->plc->remove_dc = (options & 4) != 0;
    b->plc->cus = device_cus(b->e);
    return plc_reset_range(b, 0, b->n);
}
#define NEED_PLC(b) do { if (!(b)->plc) { snprintf(g_err, sizeof(g_err), "packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; } } while (0)

extern "C" int lpcn_batch_dev_plc_reset(lpcn_batch_dev *b, int first, int count)
{
    NEED_PLC(b);
    if (check_range(b, first, count, "PLC reset")) return LPCN_E_ARG;
    DeviceGuard guard(b->e->device);
    return plc_reset_range(b, first, count);
}

// a group of the plan: its sources and destinations among the PLC's arrays and the call's frame
static GroupRun plc_group(lpcn_plc_host *p, const PlcLaunch &L, short *d_pcm)
{
    const bool queued = L.feat_src != 0;      // the features are entry feat_src - 1 of the deferred queue, else st->features
    return {p->d_ctl + L.off, L.cnt, L.kind, L.N, L.preload,
            queued ? p->fbuf + (size_t)(L.feat_src - 1) * LPCN_NB_FEAT : p->feat.p, queued ? (size_t)LPCN_PLC_FBUF * LPCN_NB_FEAT : (size_t)LPCN_NB_FEAT,
            L.pcm_src == 1 ? p->q.p : L.pcm_src == 2 ? d_pcm + L.pcm_off : nullptr, L.pcm_src == 1 ? (size_t)LPCN_PLC_QUEUE : (size_t)LPCN_FRAME_SIZE,
            L.pcm_dst == 1 ? d_pcm + L.pcm_off : nullptr, (size_t)LPCN_FRAME_SIZE, L.keep, L.scatter, L.slot, L.lane};
}
extern "C" int lpcn_batch_dev_plc_step(lpcn_batch_dev *b, short *d_pcm, const unsigned char *lost, void *hip_stream)
{
    NEED_PLC(b);
    if (!d_pcm || !lost) { snprintf(g_err, sizeof(g_err), "bad PLC step arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) {
        snprintf(g_err, sizeof(g_err), "a PLC step cannot be captured: its launch sequence depends on the loss flags"); return LPCN_E_ARG;
    }
    if (!b->active) return 0;
    { int rco = order_begin(b, st); if (rco) return rco; }
    if (p->ctl_pending) { HIP_TRY(hipEventSynchronize(p->ev_ctl)); p->ctl_pending = false; }      // (the previous step's lists have left the pinned buffer: long done)
    // (the planner and its lists run over the active prefix: the control state of the other streams does not move)
    int rc = plc_plan(p->options, b->active, p->ctl.data(), lost, p->plan, nullptr, g_err, sizeof(g_err), b->sched_lanes);
    if (rc) return rc;
    const PlcPlan &P = p->plan;
    if (P.ctl.size() > p->d_ctl.cap) { snprintf(g_err, sizeof(g_err), "PLC step: control lists exceed their buffer"); return LPCN_E_HIP; }
    if (!P.ctl.empty()) {
        memcpy(p->h_ctl.p, P.ctl.data(), sizeof(int) * P.ctl.size());
        HIP_TRY(hipMemcpyAsync(p->d_ctl, p->h_ctl.p, sizeof(int) * P.ctl.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(p->ev_ctl, st));
        p->ctl_pending = true;
    }
    forget_keep(b);      // (lpcn_batch_dev_step_host's products are the PLC's now)
    b->args_next = 0; b->last_groups.clear();
    // Lanes run side by side from here -- the lists are up -- to the join in front of the analysis; from there on everything is on the caller's stream.
    Lanes ln = lanes_begin(b, st);
    const hipStream_t caller = st;
    for (const PlcLaunch &L : P.launches) {
        const int *ctl = p->d_ctl + L.off;
        if (L.type == PLC_T_ANALYSIS) rc = lanes_join(b, ln);
        if (!rc) rc = lanes_use(b, ln, L.lane, &st);      // (st: the launch's lane from here on)
        if (rc) { (void)lanes_join(b, ln); return rc; }
        switch (L.type) {
        case PLC_T_BURG:
            hipLaunchKernelGGL(lpcn::plc_burg_kernel, dim3(L.cnt), dim3(lpcn::PLC_BURG_THREADS), 0, st, b->e->fmodel, ctl, L.cnt, d_pcm, p->D, p->remove_dc ? 1 : 0);
            break;
        case PLC_T_PRED:
            if ((rc = launch_plc_pred(b, st, ctl, L.cnt, nullptr))) { (void)lanes_join(b, ln); return rc; }
            break;
        case PLC_T_MIX:
            hipLaunchKernelGGL(lpcn::plc_mix_kernel, dim3(L.cnt), dim3(lpcn::PLC_MIX_THREADS), 0, st, L.op, ctl, L.cnt, d_pcm, (const short *)b->d_gpcm + (size_t)L.slot * LPCN_FRAME_SIZE, p->D, b->d_state);
            break;
        case PLC_T_GROUP:
            if ((rc = run_group(b, st, plc_group(p, L, d_pcm)))) { (void)lanes_join(b, ln); return rc; }
            break;
        case PLC_T_ANALYSIS:
            if ((rc = lpcn_launch_analysis_kernels(b->e->fmodel, st, b->active, 1, d_pcm, 0, (size_t)LPCN_FRAME_SIZE, b->d_an_state, p->D.an, LPCN_AN_NB_FEATURES,
                                                   (size_t)LPCN_AN_NB_FEATURES, b->d_an_resid, b->d_an_xc, b->d_an_fw, g_err, sizeof(g_err)))) return rc;
            break;
        }
    }
    if ((rc = lanes_join(b, ln))) return rc;      // (a plan always has its analysis launch: nothing is left to join)
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "PLC step: kernel launch failed"); return LPCN_E_HIP; }
    return order_end(b, caller);
}

extern "C" int lpcn_batch_dev_plc_step_host(lpcn_batch_dev *b, short *pcm, const unsigned char *lost)
{
    NEED_PLC(b);
    if (!pcm || !lost) { snprintf(g_err, sizeof(g_err), "bad PLC step arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    int rc = order_begin(b, st);
    if (rc) return rc;
    if ((rc = tune_if_due(b, st))) return rc;
    if (!b->active) return 0;
    const size_t bytes = sizeof(short) * (size_t)b->active * LPCN_FRAME_SIZE;
    HIP_TRY(hipMemcpyAsync(p->d_pcm, pcm, bytes, hipMemcpyHostToDevice, st));
    if ((rc = lpcn_batch_dev_plc_step(b, p->d_pcm, lost, st))) return rc;
    HIP_TRY(hipMemcpyAsync(pcm, p->d_pcm, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_plc_fec_add(lpcn_batch_dev *b, int s, const float *features20)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    lpcn_plc_host *p = b->plc.get();
    lpcn_plc_ctl &c = p->ctl[s];
    const int keep = c.fec_keep, fill = c.fec_fill;
    const int r = lpcn_plc_ctl_fec_add(&c, features20 == nullptr);
    if (!features20) return 0;
    if (r == 1) { snprintf(g_err, sizeof(g_err), "stream %d: FEC buffer full", s); return 1; }      // (the reference prints this and drops the vector)
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    float *ring = p->fec + (size_t)s * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT;
    if (r == 2) {
        hipLaunchKernelGGL(lpcn::plc_fec_move_kernel, dim3(1), dim3(256), 0, b->e->stream, ring, keep, fill - keep);
        HIP_TRY(hipStreamSynchronize(b->e->stream));
    }
    HIP_TRY(hipMemcpy(ring + (size_t)(c.fec_fill - 1) * LPCN_NB_FEAT, features20, sizeof(float) * LPCN_NB_FEAT, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int lpcn_batch_dev_plc_fec_clear(lpcn_batch_dev *b, int s)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    lpcn_plc_ctl &c = b->plc->ctl[s];
    c.fec_keep = c.fec_read = c.fec_fill = c.fec_skip = 0;      // src/lpcnet_plc.c:129-131
    return 0;
}

// lpcnet_plc_fec_clear / lpcnet_plc_fec_add for every stream in one call (plc_plan.h: plc_fec_feed_plan): the host plans every ring's rows from
// the control state, the records go up through the pinned list buffer and one launch moves the vectors.  Enqueue only; count, skip, clear and
// dropped are host arrays, d_features the packed vectors on the device.  Returns 1 when a vector was dropped ("FEC buffer full").
extern "C" int lpcn_plc_fec_feed_plan(int n, lpcn_plc_ctl *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped)
{
    if (n < 1 || !ctl || !count || !rec) { snprintf(g_err, sizeof(g_err), "bad FEC feed plan arguments"); return LPCN_E_ARG; }
    return plc_fec_feed_plan(n, ctl, count, skip, clear, rec, dropped, nullptr, g_err, sizeof(g_err));
}

extern "C" int lpcn_batch_dev_plc_fec_feed(lpcn_batch_dev *b, const float *d_features, const int *count, const int *skip, const unsigned char *clear,
                                           int *dropped, void *hip_stream)
{
    NEED_PLC(b);
    bool vectors = false;
    for (int s = 0; count && s < b->n; ++s) vectors |= count[s] > 0;
    if (!count || (vectors && !d_features)) { snprintf(g_err, sizeof(g_err), "bad FEC feed arguments"); return LPCN_E_ARG; }
    // (a stream beyond the active prefix takes no vectors -- rows of the packed array for it would make every later stream's rows ambiguous -- and its
    // skip and clear are ignored: its ring does not move)
    for (int s = b->active; s < b->n; ++s) if (count[s] != 0) { snprintf(g_err, sizeof(g_err), "FEC feed: stream %d is not active and has a count", s); return LPCN_E_ARG; }
    for (int s = b->active; dropped && s < b->n; ++s) dropped[s] = 0;
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) {
        snprintf(g_err, sizeof(g_err), "an FEC feed cannot be captured: its launch depends on the rings' positions"); return LPCN_E_ARG;
    }
    if (p->feed_pending) { HIP_TRY(hipEventSynchronize(p->ev_feed)); p->feed_pending = false; }      // (the previous feed's records have left the pinned buffer)
    int *h_rec = (int *)p->h_ctl.p + p->d_ctl.cap, any = 0;
    const int n_rec = plc_fec_feed_plan(b->active, p->ctl.data(), count, skip, clear, h_rec, dropped, &any, g_err, sizeof(g_err));
    if (n_rec < 0) return n_rec;
    if (any) snprintf(g_err, sizeof(g_err), "FEC buffer full");      // (the reference prints this and drops the vector)
    if (n_rec == 0) return any;
    { int rco = order_begin(b, st); if (rco) return rco; }
    HIP_TRY(hipMemcpyAsync(p->d_feed, h_rec, sizeof(int) * lpcn::PLC_FEED_REC * (size_t)n_rec, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->ev_feed, st));
    p->feed_pending = true;
    hipLaunchKernelGGL(lpcn::plc_fec_feed_kernel, dim3(n_rec), dim3(lpcn::PLC_FEED_THREADS), 0, st, (const int *)p->d_feed, n_rec, d_features, p->D.fec);
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "FEC feed: kernel launch failed"); return LPCN_E_HIP; }
    { int rco = order_end(b, st); if (rco) return rco; }
    return any;
}

extern "C" int lpcn_batch_dev_plc_fec_feed_host(lpcn_batch_dev *b, const float *features, const int *count, const int *skip, const unsigned char *clear, int *dropped)
{
    NEED_PLC(b);
    if (!count) { snprintf(g_err, sizeof(g_err), "bad FEC feed arguments"); return LPCN_E_ARG; }
    size_t total = 0;
    for (int s = 0; s < b->n; ++s) {
        if (count[s] < 0) { snprintf(g_err, sizeof(g_err), "FEC feed: stream %d has a negative count", s); return LPCN_E_ARG; }
        if (count[s] && s >= b->active) { snprintf(g_err, sizeof(g_err), "FEC feed: stream %d is not active and has a count", s); return LPCN_E_ARG; }
        total += (size_t)count[s];
    }
    if (total && !features) { snprintf(g_err, sizeof(g_err), "bad FEC feed arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    int rc = p->d_feed_src.reserve(b, total * LPCN_NB_FEAT);
    if (rc) return rc;
    if (total) HIP_TRY(hipMemcpyAsync(p->d_feed_src, features, sizeof(float) * total * LPCN_NB_FEAT, hipMemcpyHostToDevice, st));
    if ((rc = lpcn_batch_dev_plc_fec_feed(b, p->d_feed_src, count, skip, clear, dropped, st)) < 0) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// one stream's record, both halves: the device arrays' part field by field, down into *h or up from it
static int plc_state_copy(lpcn_batch_dev *b, int s, lpcn_plc_state_rec *h, bool up)
{
    lpcn_plc_host *p = b->plc.get();
    const size_t i = (size_t)s, G = (size_t)(plc_units(b->e, 0) + plc_units(b->e, 1));
    const struct { void *dev, *host; size_t bytes; } fields[] = {
        {p->delta + i, &h->delta, sizeof(int)}, {p->dc + 2 * i, h->dc, sizeof(h->dc)}, {p->q + i * LPCN_PLC_QUEUE, h->q, sizeof(h->q)},
        {p->feat + i * LPCN_NB_FEAT, h->feat, sizeof(h->feat)},
        {p->net + (4 * i + 0) * G, h->net[0], sizeof(float) * G}, {p->net + (4 * i + 1) * G, h->net[1], sizeof(float) * G},
        {p->net + (4 * i + 2) * G, h->net[2], sizeof(float) * G}, {p->net + (4 * i + 3) * G, h->net[3], sizeof(float) * G},
        {p->fec + i * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT, h->fec, sizeof(h->fec)}, {p->fbuf + i * LPCN_PLC_FBUF * LPCN_NB_FEAT, h->fbuf, sizeof(h->fbuf)},
        {b->d_keep_a + i * LPCN_ROWS_A, h->keep_a, sizeof(h->keep_a)}, {b->d_keep_b + i * LPCN_ROWS_B, h->keep_b, sizeof(h->keep_b)},
        {b->d_keep_lpc + i * LPCN_LPC_ORDER, h->keep_lpc, sizeof(h->keep_lpc)}};
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (up) p->ctl[i] = h->ctl;
    for (const auto &f : fields) HIP_TRY(up ? hipMemcpy(f.dev, f.host, f.bytes, hipMemcpyHostToDevice) : hipMemcpy(f.host, f.dev, f.bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lpcn_batch_dev_get_plc_state(lpcn_batch_dev *b, int s, lpcn_plc_state_rec *h)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n || !h) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    memset(h, 0, sizeof(*h));
    h->ctl = b->plc->ctl[s]; h->g1 = plc_units(b->e, 0); h->g2 = plc_units(b->e, 1);
    return plc_state_copy(b, s, h, false);
}

extern "C" int lpcn_batch_dev_set_plc_state(lpcn_batch_dev *b, int s, const lpcn_plc_state_rec *h)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n || !h) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    const int g1 = plc_units(b->e, 0), g2 = plc_units(b->e, 1);
    if (h->g1 != g1 || h->g2 != g2) { snprintf(g_err, sizeof(g_err), "PLC state of a %d / %d network on a %d / %d network", h->g1, h->g2, g1, g2); return LPCN_E_ARG; }
    {   // (the planner's own consistency check, on a copy)
        lpcn_plc_ctl c = h->ctl;
        const unsigned char one = 1;
        PlcPlan P;
        int rc = plc_plan(b->plc->options, 1, &c, &one, P, nullptr, g_err, sizeof(g_err));
        if (rc) return rc;
    }
    return plc_state_copy(b, s, const_cast<lpcn_plc_state_rec *>(h), true);      // (up: *h is only read)
}

// parity seam: burg_cepstral_analysis on one frame per stream.  x holds PCM values as the PLC feeds them (x[i] = pcm[i], src/lpcnet_plc.c:206):
// integers of the int16 range.
extern "C" int lpcn_batch_dev_plc_burg_host(lpcn_batch_dev *b, const float *x, float *ceps36)
{
    NEED_PLC(b);
    if (!x || !ceps36) { snprintf(g_err, sizeof(g_err), "bad arguments"); return LPCN_E_ARG; }
    const int na = b->active;
    if (!na) return 0;
    const size_t count = (size_t)na * LPCN_FRAME_SIZE;
    std::vector<short> pc(count);
    for (size_t i = 0; i < count; ++i) {
        if (!(x[i] >= -32768.f && x[i] <= 32767.f) || x[i] != (float)(int)x[i]) { snprintf(g_err, sizeof(g_err), "plc_burg: samples must be integers of the int16 range"); return LPCN_E_ARG; }
        pc[i] = (short)(int)x[i];
    }
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    HIP_TRY(hipMemcpy(p->d_pcm, pc.data(), sizeof(short) * count, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(lpcn::plc_burg_kernel, dim3(na), dim3(lpcn::PLC_BURG_THREADS), 0, st, b->e->fmodel, (const int *)p->d_ident, na, p->d_pcm, p->D, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(ceps36, p->burg, sizeof(float) * (size_t)na * 2 * LPCN_NB_BANDS, hipMemcpyDeviceToHost));
    return 0;
}

// parity seam: compute_plc_pred on every stream's network state (which advances), any 57 inputs
extern "C" int lpcn_batch_dev_plc_pred_host(lpcn_batch_dev *b, const float *in57, float *out20)
{
    NEED_PLC(b);
    if (!in57 || !out20) { snprintf(g_err, sizeof(g_err), "bad arguments"); return LPCN_E_ARG; }
    const int na = b->active;
    if (!na) return 0;
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    std::vector<int> recs((size_t)na * lpcn::PLC_PRED_REC, 0);
    if (recs.size() > p->d_ctl.cap) { snprintf(g_err, sizeof(g_err), "plc_pred: control buffer"); return LPCN_E_HIP; }
    for (int s = 0; s < na; ++s) {
        const float *in = in57 + (size_t)s * LPCN_PLC_IN;
        int *r = &recs[(size_t)s * lpcn::PLC_PRED_REC];
        r[0] = s; r[1] = lpcn::PLC_F_COMPUTE | lpcn::PLC_F_RAW; r[3] = float_bits(in[LPCN_PLC_IN - 1]);
        HIP_TRY(hipMemcpy(p->burg + (size_t)s * 2 * LPCN_NB_BANDS, in, sizeof(float) * 2 * LPCN_NB_BANDS, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(p->an + (size_t)s * LPCN_AN_NB_FEATURES, in + 2 * LPCN_NB_BANDS, sizeof(float) * LPCN_NB_FEAT, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(p->d_ctl, recs.data(), sizeof(int) * recs.size(), hipMemcpyHostToDevice));
    { int rcl = launch_plc_pred(b, st, p->d_ctl, na, b->d_gfeat.p); if (rcl) return rcl; }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out20, b->d_gfeat, sizeof(float) * (size_t)na * LPCN_NB_FEAT, hipMemcpyDeviceToHost));
    return 0;
}
