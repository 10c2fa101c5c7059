// Feature analysis and the encoder.  Owns analysis_kernels.hip.h and encode_kernels.hip.h.
#include "engine_core.h"
#include "encode_kernels.hip.h"

// ------------------------------------------------------------------------------- feature analysis -----
// A call runs in chunks of lpcn_analysis_chunk frames (encode_plan.h), which bounds the kernels' scratch.

// the analysis state (if absent) and the kernels' scratch for `chunk` frames per launch
static int analysis_alloc(lpcn_batch_dev *b, int chunk)
{
    int rc = 0;
    if (!b->d_an_state && (rc = b->d_an_state.alloc((size_t)b->n, true))) return rc;      // zeroed: lpcnet_encoder_init (src/lpcnet_enc.c:471-475)
    if (chunk <= b->an_chunk) return 0;
    const size_t items = (size_t)b->n * chunk;
    b->an_chunk = 0;                                         // (until all three have grown)
    if ((rc = b->d_an_resid.reserve(b, items * LPCN_FRAME_SIZE)) || (rc = b->d_an_xc.reserve(b, items * 2 * LPCN_PITCH_MAX_PERIOD)) ||
        (rc = b->d_an_fw.reserve(b, items * 2))) return rc;
    b->an_chunk = chunk;
    return 0;
}
extern "C" int lpcn_batch_dev_analysis_enable(lpcn_batch_dev *b, int max_frames)
{
    if (max_frames < 1) { snprintf(g_err, sizeof(g_err), "analysis: bad frame count"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    return analysis_alloc(b, lpcn_analysis_chunk(b->n, max_frames));
}

extern "C" int lpcn_batch_dev_analyze(lpcn_batch_dev *b, const void *d_pcm, int pcm_is_float, float *d_features, int feat_stride, int n_frames,
                                      void *hip_stream)
{
    if (!d_pcm || !d_features || n_frames < 1 || feat_stride < LPCN_AN_NB_FEATURES) { snprintf(g_err, sizeof(g_err), "bad analysis arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (!b->d_an_state || lpcn_analysis_chunk(b->n, n_frames) > b->an_chunk) {
        if (stream_is_capturing(st)) {      // (a capture executes nothing and allocates nothing)
            snprintf(g_err, sizeof(g_err), "analysis state / scratch for %d frames per call must exist before a capture: call lpcnet_batch_analysis_enable first", n_frames);
            return LPCN_E_ARG;
        }
        int rc = lpcn_batch_dev_analysis_enable(b, n_frames);
        if (rc) return rc;
    }
    { int rco = order_begin(b, st); if (rco) return rco; }
    const int is_float = pcm_is_float ? 1 : 0;
    const size_t pcm_stride = (size_t)n_frames * LPCN_FRAME_SIZE, feat_stream_stride = (size_t)n_frames * feat_stride;
    const int chunk = lpcn_analysis_chunk(b->n, n_frames);      // (<= b->an_chunk: the scratch may be larger than this call needs)
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        const void *p = is_float ? (const void *)((const float *)d_pcm + (size_t)f0 * LPCN_FRAME_SIZE) : (const void *)((const short *)d_pcm + (size_t)f0 * LPCN_FRAME_SIZE);
        int rc = lpcn_launch_analysis_kernels(b->e->fmodel, st, b->active, nf, p, is_float, pcm_stride, b->d_an_state, d_features + (size_t)f0 * feat_stride,
                                              feat_stride, feat_stream_stride, b->d_an_resid, b->d_an_xc, b->d_an_fw, g_err, sizeof(g_err));
        if (rc) return rc;
    }
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_analyze_host(lpcn_batch_dev *b, const void *pcm, int pcm_is_float, float *features, int feat_stride, int n_frames)
{
    if (!pcm || !features || n_frames < 1 || feat_stride < LPCN_AN_NB_FEATURES) { snprintf(g_err, sizeof(g_err), "bad analysis arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t npcm = (size_t)b->active * n_frames * LPCN_FRAME_SIZE * (pcm_is_float ? sizeof(float) : sizeof(short));      // (the active streams' rows lead the arrays)
    const size_t nfeat = (size_t)b->active * n_frames * LPCN_AN_NB_FEATURES;      // (staged densely; the caller's stride is applied by the copy out)
    int rc = b->d_an_pcm.reserve(b, npcm);
    if (!rc) rc = b->d_an_feat.reserve(b, nfeat);
    if (rc) return rc;
    if ((rc = lpcn_batch_dev_analysis_enable(b, n_frames))) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(b->d_an_pcm, pcm, npcm, hipMemcpyHostToDevice, st));
    rc = lpcn_batch_dev_analyze(b, b->d_an_pcm.p, pcm_is_float, b->d_an_feat, LPCN_AN_NB_FEATURES, n_frames, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(features, (size_t)feat_stride * sizeof(float), b->d_an_feat, LPCN_AN_NB_FEATURES * sizeof(float),
                             LPCN_AN_NB_FEATURES * sizeof(float), (size_t)b->active * n_frames, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_analysis_reset(lpcn_batch_dev *b, int first, int count)
{
    if (check_range(b, first, count, "analysis reset")) return LPCN_E_ARG;
    DeviceGuard guard(b->e->device);
    if (!b->d_an_state) return lpcn_batch_dev_analysis_enable(b, 1);      // (a fresh state IS the reset state)
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (count) HIP_TRY(hipMemset(b->d_an_state + first, 0, sizeof(lpcn_analysis_state) * (size_t)count));
    if (count && b->d_enc_vq_mem) HIP_TRY(hipMemset(b->d_enc_vq_mem + (size_t)first * LPCN_NB_BANDS, 0, sizeof(float) * LPCN_NB_BANDS * (size_t)count));
    return 0;
}
extern "C" int lpcn_batch_dev_get_analysis_state(lpcn_batch_dev *b, int s, lpcn_analysis_state *host)
{
    return stream_rec(b, s, b->d_an_state, 1, host, nullptr, lpcn_batch_dev_analysis_enable);
}
extern "C" int lpcn_batch_dev_set_analysis_state(lpcn_batch_dev *b, int s, const lpcn_analysis_state *host)
{
    return stream_rec(b, s, b->d_an_state, 1, nullptr, host, lpcn_batch_dev_analysis_enable);
}

// ------------------------------------------------------------------------------- encoder -----
// lpcnet_encode / lpcnet_compute_features per stream and packet (encode_kernels.hip.h).  A chunk is a whole number of packets within the
// analysis scratch's item bound (at least one packet, whatever the batch size): lpcn_encode_chunk (encode_plan.h).
extern "C" int lpcn_batch_dev_encoder_enable(lpcn_batch_dev *b, int max_packets)
{
    if (max_packets < 1) { snprintf(g_err, sizeof(g_err), "encoder: bad packet count"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const int chunk = lpcn_encode_chunk(b->n, max_packets);
    int rc = analysis_alloc(b, 4 * chunk);
    if (rc) return rc;
    if (!b->d_enc_vq_mem && (rc = b->d_enc_vq_mem.alloc(LPCN_NB_BANDS * (size_t)b->n, true))) return rc;
    if (chunk <= b->enc_chunk) return 0;
    const size_t items = (size_t)b->n * chunk;
    b->enc_chunk = 0;                                        // (until all three have grown)
    if ((rc = b->d_enc_feat.reserve(b, items * 4 * LPCN_AN_NB_FEATURES)) || (rc = b->d_enc_qf3.reserve(b, (size_t)b->n * (chunk + 1) * LPCN_NB_BANDS)) ||
        (rc = b->d_enc_pk.reserve(b, items * lpcn::ENC_PK))) return rc;
    b->enc_chunk = chunk;
    return 0;
}

// d_packets != NULL: encode; else compute_features into d_features
static int encode_impl(lpcn_batch_dev *b, const short *d_pcm, unsigned char *d_packets, float *d_features, int feat_stride, int n_packets, void *hip_stream)
{
    if (!d_pcm || (!d_packets && !d_features) || n_packets < 1 || (!d_packets && feat_stride < LPCN_AN_NB_FEATURES)) {
        snprintf(g_err, sizeof(g_err), "bad encoder arguments");
        return LPCN_E_ARG;
    }
    if (d_packets && !b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    const int want = lpcn_encode_chunk(b->n, n_packets);
    if (!b->d_an_state || !b->d_enc_vq_mem || want > b->enc_chunk || 4 * want > b->an_chunk) {
        if (stream_is_capturing(st)) {      // (a capture executes nothing and allocates nothing)
            snprintf(g_err, sizeof(g_err), "encoder state / scratch for %d packets per call must exist before a capture: call lpcnet_batch_encoder_enable first", n_packets);
            return LPCN_E_ARG;
        }
        int rc = lpcn_batch_dev_encoder_enable(b, n_packets);
        if (rc) return rc;
    }
    { int rco = order_begin(b, st); if (rco) return rco; }
    const int chunk = want;      // (<= b->enc_chunk, b->an_chunk / 4: the scratch may be larger than this call needs)
    const size_t pcm_stride = (size_t)n_packets * 4 * LPCN_FRAME_SIZE;
    for (int p0 = 0; p0 < n_packets; p0 += chunk) {
        const int np = n_packets - p0 < chunk ? n_packets - p0 : chunk;
        const short *p = d_pcm + (size_t)p0 * 4 * LPCN_FRAME_SIZE;
        int rc;
        if (d_packets)
            rc = lpcn_launch_encode_kernels(b->e->fmodel, b->e->enc, st, b->active, np, p, pcm_stride, b->d_an_state, b->d_enc_feat, LPCN_AN_NB_FEATURES,
                                            (size_t)np * 4 * LPCN_AN_NB_FEATURES, b->d_an_resid, b->d_an_xc, b->d_an_fw, b->d_enc_vq_mem, b->d_enc_qf3, b->d_enc_pk,
                                            d_packets + (size_t)p0 * 8, n_packets, g_err, sizeof(g_err));
        else
            rc = lpcn_launch_encode_kernels(b->e->fmodel, b->e->enc, st, b->active, np, p, pcm_stride, b->d_an_state, d_features + (size_t)p0 * 4 * feat_stride, feat_stride,
                                            (size_t)n_packets * 4 * feat_stride, b->d_an_resid, b->d_an_xc, b->d_an_fw, b->d_enc_vq_mem, b->d_enc_qf3, b->d_enc_pk,
                                            nullptr, n_packets, g_err, sizeof(g_err));
        if (rc) return rc;
    }
    return order_end(b, st);
}
extern "C" int lpcn_batch_dev_encode(lpcn_batch_dev *b, const short *d_pcm, unsigned char *d_packets, int n_packets, void *hip_stream)
{
    if (!d_packets) { snprintf(g_err, sizeof(g_err), "bad encoder arguments"); return LPCN_E_ARG; }
    return encode_impl(b, d_pcm, d_packets, nullptr, 0, n_packets, hip_stream);
}
extern "C" int lpcn_batch_dev_compute_features(lpcn_batch_dev *b, const short *d_pcm, float *d_features, int feat_stride, int n_packets, void *hip_stream)
{
    if (!d_features) { snprintf(g_err, sizeof(g_err), "bad encoder arguments"); return LPCN_E_ARG; }
    return encode_impl(b, d_pcm, nullptr, d_features, feat_stride, n_packets, hip_stream);
}

// host pointers: copy in, run, copy out, synchronise.  packets != NULL: encode; else compute_features
extern "C" int lpcn_batch_dev_encode_host(lpcn_batch_dev *b, const short *pcm, unsigned char *packets, float *features, int feat_stride, int n_packets)
{
    if (!pcm || (!packets && !features) || n_packets < 1 || (!packets && feat_stride < LPCN_AN_NB_FEATURES)) {
        snprintf(g_err, sizeof(g_err), "bad encoder arguments");
        return LPCN_E_ARG;
    }
    if (packets && !b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t npcm = (size_t)b->active * n_packets * 4 * LPCN_FRAME_SIZE * sizeof(short);
    const size_t nfeat = packets ? 0 : (size_t)b->active * n_packets * 4 * LPCN_AN_NB_FEATURES, nbytes = packets ? (size_t)b->active * n_packets * 8 : 0;
    int rc = b->d_an_pcm.reserve(b, npcm);
    if (!rc) rc = b->d_an_feat.reserve(b, nfeat);
    if (!rc) rc = b->d_packets.reserve(b, nbytes);
    if (!rc) rc = lpcn_batch_dev_encoder_enable(b, n_packets);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(b->d_an_pcm, pcm, npcm, hipMemcpyHostToDevice, st));
    rc = encode_impl(b, (const short *)b->d_an_pcm.p, packets ? b->d_packets.p : nullptr, packets ? nullptr : b->d_an_feat.p, LPCN_AN_NB_FEATURES, n_packets, st);
    if (rc) return rc;
    if (packets)
        HIP_TRY(hipMemcpyAsync(packets, b->d_packets, nbytes, hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(hipMemcpy2DAsync(features, (size_t)feat_stride * sizeof(float), b->d_an_feat, LPCN_AN_NB_FEATURES * sizeof(float),
                                 LPCN_AN_NB_FEATURES * sizeof(float), (size_t)b->active * n_packets * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_get_encoder_vq_mem(lpcn_batch_dev *b, int s, float *out18)
{
    return stream_rec(b, s, b->d_enc_vq_mem, LPCN_NB_BANDS, out18, nullptr, lpcn_batch_dev_encoder_enable);
}
extern "C" int lpcn_batch_dev_set_encoder_vq_mem(lpcn_batch_dev *b, int s, const float *in18)
{
    return stream_rec(b, s, b->d_enc_vq_mem, LPCN_NB_BANDS, nullptr, in18, lpcn_batch_dev_encoder_enable);
}
