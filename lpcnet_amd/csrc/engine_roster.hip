// Streams that come and go: the device-side copy of everything a batch keeps per stream inside one batch (one launch; across two batches it is
// engine_snapshot.hip's gather and scatter), and the decoder's VQ memory as a per-stream record.  Owns roster_kernels.hip.h.
#include "engine_core.h"
#include "roster_kernels.hip.h"

// The list of a call (copy_streams: its pairs; a snapshot: its streams and their meta rows), its pinned source and the event that guards it: made by
// the first copy or snapshot of a batch, for the largest list either can have
int stream_list_buffers(lpcn_batch_dev *b)
{
    if (b->d_pairs) return 0;
    const size_t ints = (size_t)(1 + LPCNET_SNAP_META) * (size_t)b->n;      // (a snapshot's: at least the 2 n of a pair list)
    int rc = 0;
    if ((rc = b->d_pairs.alloc(ints)) || (rc = b->h_pairs.reserve(sizeof(int) * ints))) { b->d_pairs.release(); return rc; }
    if (!b->ev_pairs.e && hipEventCreateWithFlags(&b->ev_pairs.e, hipEventDisableTiming) != hipSuccess) { b->d_pairs.release(); snprintf(g_err, sizeof(g_err), "copy_streams: hipEventCreate failed"); return LPCN_E_HIP; }
    return 0;
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
    if ((rc = stream_list_buffers(b))) return rc;
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

// the decoder's VQ memory (float[18], src/lpcnet_private.h:52), modelled on the encoder's pair
extern "C" int lpcn_batch_dev_get_decoder_vq_mem(lpcn_batch_dev *b, int s, float *out18) { return stream_rec(b, s, b->d_vq_mem, LPCN_NB_BANDS, out18, nullptr); }
extern "C" int lpcn_batch_dev_set_decoder_vq_mem(lpcn_batch_dev *b, int s, const float *in18) { return stream_rec(b, s, b->d_vq_mem, LPCN_NB_BANDS, nullptr, in18); }
