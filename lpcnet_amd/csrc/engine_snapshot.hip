// Stream snapshots: m streams' complete records to or from one contiguous buffer in one launch (lpcn_batch_dev_snapshot / _restore), the host
// forms on top of them, and the copy of streams into another batch (lpcn_batch_dev_copy_streams_to).  The record, its layout and the rule by
// which a layout fits a batch are snapshot_plan.h; the arrays are those of the stream copies (engine_core.h: each_stream_array).  Owns
// snapshot_kernels.hip.h.
#include "engine_core.h"
#include "snapshot_kernels.hip.h"
#include <stdint.h>

extern "C" int lpcn_batch_dev_snapshot_layout(const lpcn_batch_dev *b, int *layout)
{
    int cfg[SNAP_C_COUNT] = {0};
    cfg[SNAP_C_FLAVOUR] = b->e->is_int8; cfg[SNAP_C_ANALYSIS] = b->d_an_state.p != nullptr; cfg[SNAP_C_ENCODER] = b->d_enc_vq_mem.p != nullptr;
    cfg[SNAP_C_KEEP] = b->d_keep_lpc.p != nullptr;
    if (const lpcn_plc_host *p = b->plc.get()) { cfg[SNAP_C_PLC] = 1; cfg[SNAP_C_PLC_OPTIONS] = p->options; cfg[SNAP_C_G1] = plc_units(b->e, 0); cfg[SNAP_C_G2] = plc_units(b->e, 1); }
    if (const lpcn_denc_host *p = b->denc.get()) { cfg[SNAP_C_DENC_FLOATS] = (int)p->rec; cfg[SNAP_C_DENC_DFRAMES] = p->max_dframes; }
    const int ddec = b->dred && b->dred->st ? (int)b->dred->st_rec : 0;
    const int n = snap_layout_build_dec(cfg, ddec, 0, layout);
    if (n < 0) { snprintf(g_err, sizeof(g_err), "snapshot: the batch's per-stream arrays have no layout"); return LPCN_E_HIP; }
    return n;
}

// The copy table of the batch as it is now, section by section of its own layout `mine`.  snap == nullptr, a gather: every section at its own offset.
// Else a scatter of records laid out by `snap`: a section at the snapshot's offset, or fresh where the snapshot has none.
static int snap_table(lpcn_batch_dev *b, const int *mine, const int *snap, lpcn::SnapTable &T)
{
    T.rows = 0;
    T.record_bytes = (unsigned)(snap ? snap : mine)[SNAP_L_RECORD];
    T.meta_ints = LPCNET_SNAP_META;
    int k = 0;
    bool ok = true;
    auto host_halves = [&]() {             // (the host halves stand where their ids put them: in front of the next array's section)
        for (; ok && k < mine[SNAP_L_SECTIONS] && snap_is_host_half(snap_section(mine, k)[0]); ++k) {
            const int *s = snap_section(mine, k);
            if (snap) continue;
            if (T.rows >= lpcn::SNAP_MAX_ROWS) { ok = false; return; }
            T.row[T.rows++] = {nullptr, (unsigned)s[1], (unsigned)s[2], s[0] == LPCNET_SNAP_KEEP_FLAG ? (unsigned)LPCNET_SNAP_META - 1 : 0u};
        }
    };
    each_stream_array(b, [&](auto &buf, size_t per) {
        host_halves();
        const size_t bytes = per * sizeof(*buf.p);
        if (!ok || k >= mine[SNAP_L_SECTIONS] || T.rows >= lpcn::SNAP_MAX_ROWS || (size_t)snap_section(mine, k)[1] != bytes) { ok = false; return; }
        const int *s = snap_section(mine, k++), *from = snap ? snap_find(snap, s[0]) : s;
        const unsigned vec = (bytes % 16 == 0 && (uintptr_t)buf.p % 16 == 0) ? 16 : (bytes % 8 == 0 && (uintptr_t)buf.p % 8 == 0) ? 8 : 4;
        T.row[T.rows++] = {(char *)buf.p, (unsigned)bytes, from ? (unsigned)from[2] : lpcn::SNAP_FRESH, vec};
    });
    host_halves();
    if (!ok || k != mine[SNAP_L_SECTIONS]) { snprintf(g_err, sizeof(g_err), "snapshot: per-stream arrays do not fit the copy table"); return LPCN_E_HIP; }
    return 0;
}

// a list of m streams: every index inside the capacity, all distinct (a gather may also read one stream into several records: the sources of a copy)
static int check_list(lpcn_batch_dev *b, const int *streams, int m, const char *what, bool distinct = true)
{
    if (m < 0 || m > b->n || (m && !streams)) { snprintf(g_err, sizeof(g_err), "%s: bad arguments", what); return LPCN_E_ARG; }
    b->snap_mark.assign((size_t)b->n, 0);
    for (int i = 0; i < m; ++i) {
        if (streams[i] < 0 || streams[i] >= b->n) { snprintf(g_err, sizeof(g_err), "%s: entry %d (stream %d) outside the batch's %d streams", what, i, streams[i], b->n); return LPCN_E_ARG; }
        if (distinct && b->snap_mark[(size_t)streams[i]]) { snprintf(g_err, sizeof(g_err), "%s: stream %d is listed twice (entry %d)", what, streams[i], i); return LPCN_E_ARG; }
        b->snap_mark[(size_t)streams[i]] = 1;
    }
    return 0;
}

// list (and, for a gather, the meta rows behind it) through the pinned buffer, then the one launch
static int snap_launch(lpcn_batch_dev *b, const lpcn::SnapTable &T, const int *streams, const int *meta, char *d_out, const char *d_in, hipStream_t st, const char *what)
{
    int rc = 0;
    if (b->pairs_pending) { HIP_TRY(hipEventSynchronize(b->ev_pairs)); b->pairs_pending = false; }      // (the previous call's list has left the pinned buffer)
    int *h = (int *)b->h_pairs.p;
    const size_t m = (size_t)T.m, ints = m + (meta ? m * LPCNET_SNAP_META : 0);
    memcpy(h, streams, sizeof(int) * m);
    if (meta) memcpy(h + m, meta, sizeof(int) * m * LPCNET_SNAP_META);
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_pairs, h, sizeof(int) * ints, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(b->ev_pairs, st));
    b->pairs_pending = true;
    if (d_out) hipLaunchKernelGGL(lpcn::stream_gather_kernel, dim3(T.m), dim3(lpcn::SNAP_THREADS), 0, st, T, (const int *)b->d_pairs, d_out);
    else hipLaunchKernelGGL(lpcn::stream_scatter_kernel, dim3(T.m), dim3(lpcn::SNAP_THREADS), 0, st, T, (const int *)b->d_pairs, d_in);
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: kernel launch failed", what); return LPCN_E_HIP; }
    return order_end(b, st);
}

static int snapshot_any(lpcn_batch_dev *b, const int *streams, int m, void *d_records, int *meta, void *hip_stream, bool distinct)
{
    int rc = check_list(b, streams, m, "snapshot", distinct);
    if (rc) return rc;
    if (m && (!d_records || !meta || (uintptr_t)d_records % 16)) { snprintf(g_err, sizeof(g_err), "snapshot: the records need a 16-byte aligned buffer and a meta array"); return LPCN_E_ARG; }
    if (!m) return 0;
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) { snprintf(g_err, sizeof(g_err), "snapshot cannot be captured: it uploads its stream list"); return LPCN_E_ARG; }
    int mine[LPCN_SNAP_LAYOUT_MAX];
    if ((rc = lpcn_batch_dev_snapshot_layout(b, mine)) < 0 || (rc = stream_list_buffers(b))) return rc;
    lpcn::SnapTable T{};
    if ((rc = snap_table(b, mine, nullptr, T))) return rc;
    T.m = m;
    // the host halves are taken now: the planners run at enqueue time too, in call order
    for (int i = 0; i < m; ++i) {
        int *row = meta + (size_t)i * LPCNET_SNAP_META;
        const size_t s = (size_t)streams[i];
        if (b->plc) memcpy(row, &b->plc->ctl[s], sizeof(lpcn_plc_ctl)); else memset(row, 0, sizeof(lpcn_plc_ctl));
        row[LPCNET_SNAP_META - 1] = s < b->keep_ok.size() ? b->keep_ok[s] != 0 : 0;
    }
    return snap_launch(b, T, streams, meta, (char *)d_records, nullptr, st, "snapshot");
}
extern "C" int lpcn_batch_dev_snapshot(lpcn_batch_dev *b, const int *streams, int m, void *d_records, int *meta, void *hip_stream)
{
    return snapshot_any(b, streams, m, d_records, meta, hip_stream, true);
}

// 0, 1 (the host form must enable subsystems first: lpcn_batch_dev_snapshot_enable) or LPCN_E_MODEL with the message; nothing changes
extern "C" int lpcn_batch_dev_snapshot_match(const lpcn_batch_dev *b, const int *layout, int enqueue_only)
{
    int mine[LPCN_SNAP_LAYOUT_MAX];
    const int rc = lpcn_batch_dev_snapshot_layout(b, mine);
    if (rc < 0) return rc;
    const int fit = snap_layout_match(layout, mine, enqueue_only, nullptr, g_err, sizeof(g_err));
    return fit < 0 ? LPCN_E_MODEL : fit;
}
// the subsystems whose sections the snapshot has and the batch lacks: what a stream brings with it is allocated where it arrives
extern "C" int lpcn_batch_dev_snapshot_enable(lpcn_batch_dev *b, const int *layout)
{
    DeviceGuard guard(b->e->device);
    int rc = 0;
    // (the one subsystem a snapshot cannot bring along: its max_latents is the batch's to say.  Refused before anything is enabled)
    if (snap_find(layout, LPCNET_SNAP_DRED_DEC) && !b->dred) { snprintf(g_err, sizeof(g_err), "snapshot: section DRED_DEC needs the DRED decoder enabled on the batch first (lpcnet_batch_dred_enable)"); return LPCN_E_MODEL; }
    if (snap_find(layout, LPCNET_SNAP_AN) && !b->d_an_state && (rc = lpcn_batch_dev_analysis_enable(b, 1))) return rc;
    if (snap_find(layout, LPCNET_SNAP_ENC_VQ) && !b->d_enc_vq_mem && (rc = lpcn_batch_dev_encoder_enable(b, 1))) return rc;
    if (snap_find(layout, LPCNET_SNAP_KEEP_LPC) && !b->d_keep_lpc && (rc = group_alloc(b))) return rc;
    if (snap_find(layout, LPCNET_SNAP_DRED_ENC) && !b->denc && (rc = lpcn_batch_dev_dred_enc_enable(b, layout[SNAP_L_DENC_DFRAMES] > 0 ? layout[SNAP_L_DENC_DFRAMES] : 1))) return rc;
    if (snap_find(layout, LPCNET_SNAP_DRED_DEC) && !(b->dred && b->dred->st) && (rc = lpcn_batch_dev_dred_state_enable(b))) return rc;      // (after dred_enable alone)
    return 0;
}

extern "C" int lpcn_batch_dev_restore(lpcn_batch_dev *b, const int *streams, int m, const void *d_records, const int *meta, const int *layout, void *hip_stream)
{
    int rc = check_list(b, streams, m, "restore");
    if (rc) return rc;
    if (!layout || !snap_layout_valid(layout, LPCN_SNAP_LAYOUT_MAX)) { snprintf(g_err, sizeof(g_err), "restore: not a snapshot layout"); return LPCN_E_ARG; }
    if (m && (!d_records || !meta || (uintptr_t)d_records % 16)) { snprintf(g_err, sizeof(g_err), "restore: the records need a 16-byte aligned buffer and a meta array"); return LPCN_E_ARG; }
    int mine[LPCN_SNAP_LAYOUT_MAX];
    if ((rc = lpcn_batch_dev_snapshot_layout(b, mine)) < 0) return rc;
    if (snap_layout_match(layout, mine, 1, nullptr, g_err, sizeof(g_err))) return LPCN_E_MODEL;
    if (!m) return 0;
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) { snprintf(g_err, sizeof(g_err), "restore cannot be captured: it uploads its stream list"); return LPCN_E_ARG; }
    if ((rc = stream_list_buffers(b))) return rc;
    lpcn::SnapTable T{};
    if ((rc = snap_table(b, mine, layout, T))) return rc;
    T.m = m;
    if ((rc = snap_launch(b, T, streams, nullptr, nullptr, (const char *)d_records, st, "restore"))) return rc;
    // the host halves arrive now, as the stream copies' do; a snapshot without the kept products leaves a fresh stream's flag
    const bool keep = b->d_keep_lpc && snap_find(layout, LPCNET_SNAP_KEEP_LPC);
    for (int i = 0; i < m; ++i) {
        const int *row = meta + (size_t)i * LPCNET_SNAP_META;
        const size_t d = (size_t)streams[i];
        if (b->plc) memcpy(&b->plc->ctl[d], row, sizeof(lpcn_plc_ctl));
        const char ok = keep && row[LPCNET_SNAP_META - 1] != 0;
        if (b->keep_ok.size() != (size_t)b->n && ok) b->keep_ok.assign((size_t)b->n, 0);
        if (d < b->keep_ok.size()) b->keep_ok[d] = ok;
    }
    return 0;
}

// ---- the host forms: records [.][record bytes] and meta [.][LPCNET_SNAP_META] are the two areas of a blob; entry j of the list is record pos[j]
// of them (pos == nullptr: j) -- a shard of a sharded batch owns some of a blob's records.  Through the batch's staging buffer and its pinned copy;
// both synchronise before they return.
static int snap_staging(lpcn_batch_dev *b, size_t bytes, bool pinned)
{
    int rc = b->d_snap.reserve(b, bytes);
    if (!rc && pinned && bytes > b->h_snap.cap) { if ((rc = wait_all(b))) return rc; rc = b->h_snap.reserve(bytes); }
    return rc;
}
extern "C" int lpcn_batch_dev_snapshot_host(lpcn_batch_dev *b, const int *streams, const int *pos, int m, void *records, int *meta)
{
    int mine[LPCN_SNAP_LAYOUT_MAX], rc = check_list(b, streams, m, "snapshot");
    if (rc || (rc = lpcn_batch_dev_snapshot_layout(b, mine)) < 0) return rc;
    if (!m) return 0;
    DeviceGuard guard(b->e->device);
    const size_t rb = (size_t)mine[SNAP_L_RECORD];
    if ((rc = snap_staging(b, rb * (size_t)m, true))) return rc;
    b->snap_meta.resize((size_t)b->n * LPCNET_SNAP_META);
    if ((rc = lpcn_batch_dev_snapshot(b, streams, m, b->d_snap.p, b->snap_meta.data(), nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(b->h_snap.p, b->d_snap.p, rb * (size_t)m, hipMemcpyDeviceToHost, b->e->stream));
    if ((rc = wait_all(b))) return rc;
    for (int j = 0; j < m; ++j) {
        const size_t at = (size_t)(pos ? pos[j] : j);
        memcpy((char *)records + at * rb, (const char *)b->h_snap.p + (size_t)j * rb, rb);
        memcpy(meta + at * LPCNET_SNAP_META, &b->snap_meta[(size_t)j * LPCNET_SNAP_META], sizeof(int) * LPCNET_SNAP_META);
    }
    return 0;
}
extern "C" int lpcn_batch_dev_restore_host(lpcn_batch_dev *b, const int *streams, const int *pos, int m, const void *records, const int *meta, const int *layout)
{
    int rc = check_list(b, streams, m, "restore");
    if (rc) return rc;
    if (!layout || !snap_layout_valid(layout, LPCN_SNAP_LAYOUT_MAX)) { snprintf(g_err, sizeof(g_err), "restore: not a snapshot layout"); return LPCN_E_ARG; }
    if (!m) return 0;
    DeviceGuard guard(b->e->device);
    const size_t rb = (size_t)layout[SNAP_L_RECORD];
    if ((rc = snap_staging(b, rb * (size_t)m, true))) return rc;
    b->snap_meta.resize((size_t)b->n * LPCNET_SNAP_META);
    for (int j = 0; j < m; ++j) {
        const size_t at = (size_t)(pos ? pos[j] : j);
        memcpy((char *)b->h_snap.p + (size_t)j * rb, (const char *)records + at * rb, rb);
        memcpy(&b->snap_meta[(size_t)j * LPCNET_SNAP_META], meta + at * LPCNET_SNAP_META, sizeof(int) * LPCNET_SNAP_META);
    }
    if ((rc = order_begin(b, b->e->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_snap.p, b->h_snap.p, rb * (size_t)m, hipMemcpyHostToDevice, b->e->stream));
    if ((rc = lpcn_batch_dev_restore(b, streams, m, b->d_snap.p, b->snap_meta.data(), layout, nullptr))) { (void)wait_all(b); return rc; }
    return wait_all(b);
}

// Streams src[i] of `from` -> streams dst[i] of `to` (dst distinct; a source may feed several destinations): a gather on the source's stream into its staging buffer, the transfer, a scatter on the
// destination's stream behind an event.  Only enqueued once the staging buffers have their size.  The source's stream then waits for the scatter:
// its staging buffer is free again before anything later on that stream -- the next copy's gather -- can touch it.
extern "C" int lpcn_batch_dev_copy_streams_to(lpcn_batch_dev *from, const int *src, lpcn_batch_dev *to, const int *dst, int m)
{
    if (!from || !to || from == to) { snprintf(g_err, sizeof(g_err), "copy_streams_to: needs two batches"); return LPCN_E_ARG; }
    int rc = 0, lay[LPCN_SNAP_LAYOUT_MAX];
    if ((rc = check_list(from, src, m, "copy_streams_to (source)", false)) || (rc = check_list(to, dst, m, "copy_streams_to (destination)"))) return rc;
    if ((rc = lpcn_batch_dev_snapshot_layout(from, lay)) < 0) return rc;
    if ((rc = lpcn_batch_dev_snapshot_match(to, lay, 0)) < 0) return rc;
    if (rc == 1 && (rc = lpcn_batch_dev_snapshot_enable(to, lay))) return rc;
    if (!m) return 0;
    const size_t bytes = (size_t)lay[SNAP_L_RECORD] * (size_t)m;
    const bool same = from->e->device == to->e->device;
    int peer = 1;
    if (!same && hipDeviceCanAccessPeer(&peer, to->e->device, from->e->device) != hipSuccess) peer = 0;
    {
        DeviceGuard guard(from->e->device);
        if ((rc = snap_staging(from, bytes, !same && !peer))) return rc;
        from->snap_meta.resize((size_t)from->n * LPCNET_SNAP_META);
        if ((rc = snapshot_any(from, src, m, from->d_snap.p, from->snap_meta.data(), nullptr, false))) return rc;
        if (!same && !peer) {
            HIP_TRY(hipMemcpyAsync(from->h_snap.p, from->d_snap.p, bytes, hipMemcpyDeviceToHost, from->e->stream));
            if ((rc = order_end(from, from->e->stream))) return rc;
        }
    }
    const char *d_in = from->d_snap.p;
    {
        DeviceGuard guard(to->e->device);
        if (!same && (rc = snap_staging(to, bytes, false))) return rc;
        if ((rc = order_begin(to, to->e->stream))) return rc;
        HIP_TRY(hipStreamWaitEvent(to->e->stream, from->ev_last, 0));         // (the gather, and the copy to the host behind it)
        if (!same) {
            if (peer) HIP_TRY(hipMemcpyPeerAsync(to->d_snap.p, to->e->device, from->d_snap.p, from->e->device, bytes, to->e->stream));
            else HIP_TRY(hipMemcpyAsync(to->d_snap.p, from->h_snap.p, bytes, hipMemcpyHostToDevice, to->e->stream));
            d_in = to->d_snap.p;
        }
        if ((rc = lpcn_batch_dev_restore(to, dst, m, d_in, from->snap_meta.data(), lay, nullptr))) return rc;
    }
    DeviceGuard guard(from->e->device);
    HIP_TRY(hipStreamWaitEvent(from->e->stream, to->ev_last, 0));
    return 0;
}
