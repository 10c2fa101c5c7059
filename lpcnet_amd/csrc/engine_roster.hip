// Streams that come and go: the device-side copy of everything a batch keeps per stream, inside one batch (one launch) and across two batches
// (through the host), and the decoder's VQ memory as a per-stream record.  Owns roster_kernels.hip.h.
#include "engine_core.h"
#include "roster_kernels.hip.h"

// Every per-stream array of the batch that is allocated now, as (base, bytes per stream).  `fn(buffer, elements per stream)`.
template <typename F>
static void each_stream_array(lpcn_batch_dev *b, F fn)
{
    fn(b->d_state, (size_t)1);
    fn(b->d_vq_mem, (size_t)LPCN_NB_BANDS);
    if (b->d_an_state) fn(b->d_an_state, (size_t)1);
    if (b->d_enc_vq_mem) fn(b->d_enc_vq_mem, (size_t)LPCN_NB_BANDS);
    if (b->d_keep_lpc) { fn(b->d_keep_a, (size_t)LPCN_ROWS_A); fn(b->d_keep_b, (size_t)LPCN_ROWS_B); fn(b->d_keep_lpc, (size_t)LPCN_LPC_ORDER); }
    if (lpcn_plc_host *p = b->plc.get()) {
        fn(p->q, (size_t)LPCN_PLC_QUEUE); fn(p->feat, (size_t)LPCN_NB_FEAT); fn(p->net, 4 * (size_t)(plc_units(b->e, 0) + plc_units(b->e, 1))); fn(p->dc, (size_t)2);
        fn(p->delta, (size_t)1); fn(p->fec, (size_t)LPCN_PLC_MAX_FEC * LPCN_NB_FEAT); fn(p->fbuf, (size_t)LPCN_PLC_FBUF * LPCN_NB_FEAT);
        fn(p->lp, (size_t)LPCN_FRAME_SIZE); fn(p->burg, (size_t)2 * LPCN_NB_BANDS); fn(p->an, (size_t)LPCN_AN_NB_FEATURES);
    }
    if (lpcn_denc_host *p = b->denc.get()) fn(p->state, p->rec);
}
static int roster_table(lpcn_batch_dev *b, lpcn::RosterTable &T)
{
    T.rows = 0;
    bool ok = true;
    each_stream_array(b, [&](auto &buf, size_t per) {
        const size_t bytes = per * sizeof(*buf.p);
        if (T.rows >= lpcn::ROSTER_MAX_ROWS || bytes % 4 || bytes > 0xffffffffu) { ok = false; return; }
        const unsigned vec = (bytes % 16 == 0 && (uintptr_t)buf.p % 16 == 0) ? 16 : (bytes % 8 == 0 && (uintptr_t)buf.p % 8 == 0) ? 8 : 4;
        T.row[T.rows++] = {(char *)buf.p, (unsigned)bytes, vec};
    });
    if (!ok) { snprintf(g_err, sizeof(g_err), "copy_streams: per-stream arrays do not fit the copy table"); return LPCN_E_HIP; }
    return 0;
}
// the host halves of a stream: the PLC's control state and whether the kept frame products exist
static void copy_host_half(lpcn_batch_dev *from, int s, lpcn_batch_dev *to, int d)
{
    if (from->plc && to->plc) to->plc->ctl[(size_t)d] = from->plc->ctl[(size_t)s];
    const char ok = (size_t)s < from->keep_ok.size() ? from->keep_ok[(size_t)s] : 0;
    if (to->keep_ok.size() != (size_t)to->n && ok) to->keep_ok.assign((size_t)to->n, 0);
    if ((size_t)d < to->keep_ok.size()) to->keep_ok[(size_t)d] = ok;
}

extern "C" int lpcn_batch_dev_copy_streams(lpcn_batch_dev *b, const int *src, const int *dst, int m, void *hip_stream)
{
    if (m < 0 || m > b->n || (m && (!src || !dst))) { snprintf(g_err, sizeof(g_err), "copy_streams: bad arguments"); return LPCN_E_ARG; }
    for (int i = 0; i < m; ++i)
        if (src[i] < 0 || src[i] >= b->n || dst[i] < 0 || dst[i] >= b->n || src[i] == dst[i]) { snprintf(g_err, sizeof(g_err), "copy_streams: pair %d (%d -> %d) outside the batch's %d streams", i, src[i], dst[i], b->n); return LPCN_E_ARG; }
    if (!m) return 0;
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) { snprintf(g_err, sizeof(g_err), "copy_streams cannot be captured: it uploads its pair list"); return LPCN_E_ARG; }
    int rc = 0;
    if (!b->d_pairs) {                 // (the first copy of a batch: the list's two buffers and its event)
        if ((rc = b->d_pairs.alloc(2 * (size_t)b->n)) || (rc = b->h_pairs.reserve(sizeof(int) * 2 * (size_t)b->n))) { b->d_pairs.release(); return rc; }
        if (!b->ev_pairs.e && hipEventCreateWithFlags(&b->ev_pairs.e, hipEventDisableTiming) != hipSuccess) { b->d_pairs.release(); snprintf(g_err, sizeof(g_err), "copy_streams: hipEventCreate failed"); return LPCN_E_HIP; }
    }
    lpcn::RosterTable T{};
    if ((rc = roster_table(b, T))) return rc;
    T.pairs = m;
    if (b->pairs_pending) { HIP_TRY(hipEventSynchronize(b->ev_pairs)); b->pairs_pending = false; }      // (the previous call's list has left the pinned buffer)
    int *h = (int *)b->h_pairs.p;
    for (int i = 0; i < m; ++i) { h[2 * i] = src[i]; h[2 * i + 1] = dst[i]; }
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_pairs, h, sizeof(int) * 2 * (size_t)m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(b->ev_pairs, st));
    b->pairs_pending = true;
    hipLaunchKernelGGL(lpcn::stream_copy_kernel, dim3(m), dim3(lpcn::ROSTER_THREADS), 0, st, T, (const int *)b->d_pairs);
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "copy_streams: kernel launch failed"); return LPCN_E_HIP; }
    // the host halves move now: the planners run at enqueue time too, in call order
    for (int i = 0; i < m; ++i) copy_host_half(b, src[i], b, dst[i]);
    return order_end(b, st);
}

// Across two batches (two shards of one LPCNetBatch): through pinned host memory, after everything enqueued for both.  An array that only the
// source batch has is allocated in the destination first; one that only the destination has gets the record of a fresh stream (zeros).
extern "C" int lpcn_batch_dev_copy_stream_across(lpcn_batch_dev *from, int s, lpcn_batch_dev *to, int d)
{
    if (!from || !to || from == to || s < 0 || s >= from->n || d < 0 || d >= to->n) { snprintf(g_err, sizeof(g_err), "copy_streams: bad cross-shard pair"); return LPCN_E_ARG; }
    if ((from->plc != nullptr) != (to->plc != nullptr) || (from->plc && (from->plc->options != to->plc->options || plc_units(from->e, 0) != plc_units(to->e, 0) || plc_units(from->e, 1) != plc_units(to->e, 1)))) {
        snprintf(g_err, sizeof(g_err), "copy_streams: the shards' packet-loss concealment differs"); return LPCN_E_MODEL;
    }
    int rc = 0;
    {
        DeviceGuard guard(to->e->device);
        if (from->d_an_state && !to->d_an_state && (rc = lpcn_batch_dev_analysis_enable(to, 1))) return rc;
        if (from->d_enc_vq_mem && !to->d_enc_vq_mem && (rc = lpcn_batch_dev_encoder_enable(to, 1))) return rc;
        if (from->d_keep_lpc && !to->d_keep_lpc && (rc = group_alloc(to))) return rc;
        if (from->denc && !to->denc && (rc = lpcn_batch_dev_dred_enc_enable(to, from->denc->max_dframes))) return rc;
        if ((rc = wait_all(to))) return rc;
    }
    struct Part { const char *src; char *dst; size_t bytes; };
    std::vector<Part> parts;
    size_t total = 0;
    auto add = [&](const void *fp, void *tp, size_t per_bytes) {
        parts.push_back({fp ? (const char *)fp + (size_t)s * per_bytes : nullptr, (char *)tp + (size_t)d * per_bytes, per_bytes});
        if (fp) total += per_bytes;
    };
    add(from->d_state.p, to->d_state.p, sizeof(lpcn_stream_state));
    add(from->d_vq_mem.p, to->d_vq_mem.p, sizeof(float) * LPCN_NB_BANDS);
    if (to->d_an_state) add(from->d_an_state.p, to->d_an_state.p, sizeof(lpcn_analysis_state));
    if (to->d_enc_vq_mem) add(from->d_enc_vq_mem.p, to->d_enc_vq_mem.p, sizeof(float) * LPCN_NB_BANDS);
    if (to->d_keep_lpc) {
        add(from->d_keep_a.p, to->d_keep_a.p, sizeof(float) * LPCN_ROWS_A); add(from->d_keep_b.p, to->d_keep_b.p, sizeof(float) * LPCN_ROWS_B);
        add(from->d_keep_lpc.p, to->d_keep_lpc.p, sizeof(float) * LPCN_LPC_ORDER);
    }
    if (lpcn_plc_host *p = from->plc.get()) {
        lpcn_plc_host *q = to->plc.get();
        const size_t G4 = 4 * (size_t)(plc_units(from->e, 0) + plc_units(from->e, 1));
        add(p->q.p, q->q.p, sizeof(short) * LPCN_PLC_QUEUE); add(p->feat.p, q->feat.p, sizeof(float) * LPCN_NB_FEAT); add(p->net.p, q->net.p, sizeof(float) * G4);
        add(p->dc.p, q->dc.p, sizeof(double) * 2); add(p->delta.p, q->delta.p, sizeof(int)); add(p->fec.p, q->fec.p, sizeof(float) * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT);
        add(p->fbuf.p, q->fbuf.p, sizeof(float) * LPCN_PLC_FBUF * LPCN_NB_FEAT); add(p->lp.p, q->lp.p, sizeof(short) * LPCN_FRAME_SIZE);
        add(p->burg.p, q->burg.p, sizeof(float) * 2 * LPCN_NB_BANDS); add(p->an.p, q->an.p, sizeof(float) * LPCN_AN_NB_FEATURES);
    }
    if (to->denc) add(from->denc ? from->denc->state.p : nullptr, to->denc->state.p, sizeof(float) * to->denc->rec);
    char *pin = nullptr;
    {
        DeviceGuard guard(from->e->device);
        if ((rc = wait_all(from)) || (rc = from->h_pin.reserve(total))) return rc;
        pin = (char *)from->h_pin.p;
        size_t off = 0;
        for (const Part &pt : parts) if (pt.src) { HIP_TRY(hipMemcpy(pin + off, pt.src, pt.bytes, hipMemcpyDeviceToHost)); off += pt.bytes; }
    }
    {
        DeviceGuard guard(to->e->device);
        size_t off = 0;
        for (const Part &pt : parts) {
            if (pt.src) { HIP_TRY(hipMemcpy(pt.dst, pin + off, pt.bytes, hipMemcpyHostToDevice)); off += pt.bytes; }
            else HIP_TRY(hipMemset(pt.dst, 0, pt.bytes));
        }
    }
    copy_host_half(from, s, to, d);
    return 0;
}

// the decoder's VQ memory (float[18], src/lpcnet_private.h:52), modelled on the encoder's pair
extern "C" int lpcn_batch_dev_get_decoder_vq_mem(lpcn_batch_dev *b, int s, float *out18) { return stream_rec(b, s, b->d_vq_mem, LPCN_NB_BANDS, out18, nullptr); }
extern "C" int lpcn_batch_dev_set_decoder_vq_mem(lpcn_batch_dev *b, int s, const float *in18) { return stream_rec(b, s, b->d_vq_mem, LPCN_NB_BANDS, nullptr, in18); }
