// The 1.6 kb/s encoder on the device: lpcnet_encode (src/lpcnet_enc.c:882-893; 640 PCM samples -> one 8-byte packet) and
// lpcnet_compute_features (:895-909; -> four 36-float feature vectors) for every stream and packet of a batch, bit for bit like the
// reference's generic-C float build.  compute_frame_features is the same code in the single-frame and the four-frame path, so the first
// two launches of a chunk are the analysis kernels unchanged, on 4 * n_packets frames (analysis_kernels.hip.h).  Then:
//   encode_pitch_kernel    one workgroup per stream, serial over the chunk's packets: process_superframe (:599-701) -- weights over eight
//                          half-frames, eight Viterbi steps (the step the analysis uses), backward pass, the weighted regression, voiced /
//                          corr_id / main_pitch / modulation; or, for compute_features, the unquantised [18], [19].  The ONLY writer of the
//                          analysis state.
//   encode_vq_end_kernel   one wavefront per (stream, packet): c0_id and quantize_3stage_mbest (:131-240) of frame 3
//   encode_vq_mid_kernel   one wavefront per (stream, packet): quantize_diff (:284-317) of frame 1 with sign, double_interp_search
//                          (:389-409), the nine bit fields -> 8 bytes
// vq_mem entering packet p is the quantised frame 3 of packet p - 1, which the vq_end kernel produces without reading vq_mem: every
// (stream, packet) of a chunk is independent in both VQ kernels (packet 0 takes the stored vq_mem), and only the pitch kernel is serial.
// The searches put one codebook entry on a lane's accumulator, dimensions serial in the reference's order, d = d + (x - c)*(x - c) with
// three roundings (-ffp-contract=off); a workgroup stages the transposed codebook ([dimension][entry], lanes read four consecutive
// entries as one 128-bit word) once per stage for all its items.  The quantised features of frames 0..2, their LPC and the pitch
// features of the quantised path (:686-690, :720-723) are not part of a packet and are not computed.
#pragma once
#include "analysis_kernels.hip.h"
#include "encode_plan.h"

namespace lpcn {

constexpr int ENC_NB1 = LPCN_NB_BANDS - 1;     // NB_BANDS_1: the 17 coefficients of the three-stage VQ
constexpr int ENC_CB = 1024;                   // entries of a stage codebook, and of one quarter of ceps_codebook_diff4
constexpr int ENC_SURV = 5;                    // SURVIVORS
constexpr int ENC_VQ_WAVES = LPCN_ENC_VQ_WAVES;
constexpr int ENC_VQ_THREADS = 64 * ENC_VQ_WAVES;
constexpr int ENC_END_IPW = LPCN_ENC_END_IPW;  // (stream, packet) items per wavefront, at most (encode_plan.h: lpcn_encode_ipw)
constexpr int ENC_MID_IPW = LPCN_ENC_MID_IPW;
constexpr int ENC_PK = 4;                      // ints per packet of the scratch record: [0] pitch | modulation | corr_id (11 bits), [1] c0_id + 64, [2] vq_end (30 bits)

// (int)v as the reference's x86 build converts (cvttsd2si): out of range and NaN give INT_MIN
__device__ __forceinline__ int enc_int(const double v) { return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (int)0x80000000; }
__device__ __forceinline__ int enc_imax(const int a, const int b) { return a > b ? a : b; }
__device__ __forceinline__ int enc_imin(const int a, const int b) { return a < b ? a : b; }

// log(a), a finite and positive, for main_pitch (src/lpcnet_enc.c:671): the correctly rounded log of lpcnet_log10.h on the mantissa plus
// k ln 2 in two parts, within one ULP of the host libm's (glibc: < 0.52 ULP).  main_pitch = floor(.5 + 30.29..*log(a)) can differ from
// the reference's only when that product lies within about one double ULP of a rounding boundary: ~2^-48 per packet, a day of 8192
// streams sees 2e10 packets.  The 63 thresholds of the monotone map as a generated table would carry the same exposure against the
// libm of the host that generated them.
__device__ __forceinline__ double enc_log(const double a)
{
    uint64_t bits;
    memcpy(&bits, &a, 8);
    const int k = (int)((bits >> 52) & 0x7ff) - 1023;
    bits = (bits & 0x000fffffffffffffull) | (0x3ffull << 52);
    double x;
    memcpy(&x, &bits, 8);
    return (double)k * LPCN_LOG_LN2_HI + (lpcn_log_unit(x) + (double)k * LPCN_LOG_LN2_LO);
}

// process_superframe for every packet of the chunk, and the state the next chunk starts from.  QUANT: lpcnet_encode (quantize = 1) -> the
// packet's pitch fields; else lpcnet_compute_features -> feat[..][18], [19] and vq_mem = the unquantised frame 3 of the last packet.
template <bool QUANT>
__global__ __launch_bounds__(AN_PITCH_THREADS) void encode_pitch_kernel(int n_packets, const short *pcm, size_t pcm_stream_stride, lpcn_analysis_state *states,
                                                                        const float *resid, const float *xc_in, const float *fw_in, float *feat, int feat_stride,
                                                                        size_t feat_stream_stride, float *vq_mem, float *qf3 /*[stream][n_packets+1][18]*/,
                                                                        int *pk /*[stream][n_packets][ENC_PK]*/)
{
    __shared__ float pmp[AN_PATHS];
    __shared__ float xcw[8][LPCN_PITCH_MAX_PERIOD];
    __shared__ short prevs[8][AN_PATHS];      // pitch_prev[8][]
    __shared__ float red_v[AN_PITCH_THREADS / 64];
    __shared__ int red_i[AN_PITCH_THREADS / 64];
    __shared__ float amb[LPCN_AN_OVERLAP];
    const int i = threadIdx.x;
    const int stream = blockIdx.x;
    const int n_frames = 4 * n_packets;
    lpcn_analysis_state *st = &states[stream];
    const float *r = resid + (size_t)stream * n_frames * LPCN_FRAME_SIZE;
    const size_t base = (size_t)stream * pcm_stream_stride;
    if (i < AN_PATHS) pmp[i] = st->pitch_max_path[i];
    float pmpa = st->pitch_max_path_all;
    int best_i = st->best_i;
    if (QUANT && i < LPCN_NB_BANDS) qf3[(size_t)stream * (n_packets + 1) * LPCN_NB_BANDS + i] = vq_mem[(size_t)stream * LPCN_NB_BANDS + i];
    __syncthreads();
    for (int p = 0; p < n_packets; ++p) {
        const size_t half0 = ((size_t)stream * n_frames + 4 * p) * 2;      // the packet's first half-frame in xc_in / fw_in
        // weights normalised by 8 / (1e-15f + w0 + .. + w7) (:617-618)
        float fsum = 1e-15f;
#pragma unroll
        for (int h = 0; h < 8; ++h) fsum = fsum + fw_in[half0 + h];
        const float scale = 8.f / fsum;
        for (int h = 0; h < 8; ++h)
            an_viterbi_step(i, xc_in[(half0 + h) * LPCN_PITCH_MAX_PERIOD + i], fw_in[half0 + h] * scale, xcw[h], prevs[h], pmp, red_v, red_i, pmpa, best_i);
        if (i == 0) {
            // backward pass (:647-655)
            int best[8];
            float w[8];
            int b = best_i;
            float frame_corr = 0.f;
#pragma unroll
            for (int h = 7; h >= 0; --h) {
                w[h] = fw_in[half0 + h] * scale;
                best[h] = LPCN_PITCH_MAX_PERIOD - b;
                frame_corr = frame_corr + w[h] * xcw[h][b];
                b = prevs[h][b];
            }
            frame_corr = frame_corr / 8.f;
            if (!QUANT) {
                // :691-693
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float *fo = feat + (size_t)stream * feat_stream_stride + (size_t)(4 * p + k) * feat_stride;
                    fo[LPCN_NB_BANDS] = .01f * (float)(enc_imax(66, enc_imin(510, best[2 * k] + best[2 * k + 1])) - 200);
                    fo[LPCN_NB_BANDS + 1] = frame_corr - .5f;
                }
            } else {
                if (frame_corr < 0.f) frame_corr = 0.f;
                // the weighted linear regression of the pitch contour (:661-684): float sums, sub = 2..9
                float sw = 0.f, sx = 0.f, sxx = 0.f, sxy = 0.f, sy = 0.f;
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const float fs = (float)(h + 2), fb = (float)best[h];
                    sw = sw + w[h];
                    sx = sx + w[h] * fs;
                    sxx = sxx + (w[h] * fs) * fs;
                    sxy = sxy + (w[h] * fs) * fb;
                    sy = sy + w[h] * fb;
                }
                const bool voiced = (double)frame_corr >= .3;
                float best_a = (sw * sxy - sx * sy) / (sw * sxx - sx * sx);
                int corr_id;
                if (voiced) {
                    const float mean_pitch = sy / sw;
                    const float max_a = mean_pitch / 32.f, neg = -max_a;
                    const float lo = LPCN_MAX16(neg, best_a);
                    best_a = max_a < lo ? max_a : lo;                       // MIN16(max_a, MAX16(-max_a, best_a))
                    corr_id = enc_int(floor((double)((frame_corr - .3f) / .175f)));
                } else {
                    best_a = 0.f;
                    corr_id = enc_int(floor((double)(frame_corr / .075f)));
                }
                const float best_b = (sy - best_a * sx) / sw;
                const float center_pitch = best_b + 5.5f * best_a;
                const float cp32 = center_pitch / 32.f;
                // (for an argument that is not finite and positive the reference's log gives -inf / NaN / +inf, and its conversion INT_MIN)
                int main_pitch = (cp32 > 0.f && cp32 < HUGE_VALF) ? enc_int(floor(.5 + (21. * 1.442695041) * enc_log((double)cp32))) : (int)0x80000000;
                main_pitch = enc_imax(0, enc_imin(63, main_pitch));
                int modulation = enc_int(floor(.5 + (double)((112.f * best_a) / center_pitch)));
                modulation = enc_imax(-3, enc_imin(3, modulation));
                pk[((size_t)stream * n_packets + p) * ENC_PK] = (main_pitch << 5) | ((voiced ? modulation + 4 : 0) << 2) | (corr_id & 3);
            }
        }
        __syncthreads();
    }
    if (!QUANT && i < LPCN_NB_BANDS)       // :725 with the unquantised frame 3 (written by the spectrum kernel)
        vq_mem[(size_t)stream * LPCN_NB_BANDS + i] = feat[(size_t)stream * feat_stream_stride + (size_t)(n_frames - 1) * feat_stride + i];
    an_store_state(i, n_frames, pcm, 0, base, r, st, pmp, amb, pmpa, best_i);
}

// LDS written by some lanes of a wavefront, read by others of the same wavefront
__device__ __forceinline__ void enc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// n floats (a multiple of 4) from global memory to LDS, by the whole workgroup
__device__ __forceinline__ void enc_stage(float *lds, const float *g, const int n)
{
    for (int k = threadIdx.x * 4; k < n; k += ENC_VQ_THREADS * 4) *(float4 *)(lds + k) = *(const float4 *)(g + k);
}

// lexicographic minimum of (d, idx) over the wavefront, in every lane
__device__ __forceinline__ void enc_wave_argmin(float &d, int &idx)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float od = __shfl_xor(d, off);
        const int oi = __shfl_xor(idx, off);
        if (od < d || (od == d && oi < idx)) { d = od; idx = oi; }
    }
}

// vq_quantize_mbest (src/lpcnet_enc.c:53-78) over a staged 1024 x 17 codebook: the five lexicographically smallest (distance, index)
// pairs, ascending, in every lane.  Lane l owns entries 256 kk + 4 l + e (kk, e = 0..3), so ascending (kk, e) is ascending index.
__device__ __forceinline__ void enc_search5(const float *cbt, const float *x, const int lane, float (&od)[ENC_SURV], int (&oi)[ENC_SURV])
{
    float d[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) d[c] = 0.f;
#pragma unroll 1
    for (int j = 0; j < ENC_NB1; ++j) {
        const float xj = x[j];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float4 c4 = *(const float4 *)(cbt + j * ENC_CB + kk * 256 + 4 * lane);
            float t;
            t = xj - c4.x; d[4 * kk + 0] = d[4 * kk + 0] + t * t;
            t = xj - c4.y; d[4 * kk + 1] = d[4 * kk + 1] + t * t;
            t = xj - c4.z; d[4 * kk + 2] = d[4 * kk + 2] + t * t;
            t = xj - c4.w; d[4 * kk + 3] = d[4 * kk + 3] + t * t;
        }
    }
#pragma unroll
    for (int r = 0; r < ENC_SURV; ++r) {
        float bd = d[0];
        int bc = 0;
#pragma unroll
        for (int c = 1; c < 16; ++c) if (d[c] < bd) { bd = d[c]; bc = c; }
        int bidx = (bc >> 2) * 256 + 4 * lane + (bc & 3);
        enc_wave_argmin(bd, bidx);
        od[r] = bd;
        oi[r] = bidx;
#pragma unroll
        for (int c = 0; c < 16; ++c) if ((c >> 2) * 256 + 4 * lane + (c & 3) == bidx) d[c] = INFINITY;      // taken
    }
}

// One survivor's search result merged into the global list (src/lpcnet_enc.c:155-176, :185-212), literally, by one lane on LDS arrays:
// a single forward pass with strict <, guarded by curr_dist[0] < glob_dist[4].  idx: ENC_SURV rows of `width` ints; the new rows are
// {head[0 .. width-2], curr_index[m]}.
__device__ __forceinline__ void enc_merge(const int k, const float *curr_dist, const int *curr_index, float *glob_dist, int *idx, const int width, const int *head)
{
    if (k == 0) {
        for (int m = 0; m < ENC_SURV; ++m) {
            for (int c = 0; c < width - 1; ++c) idx[m * width + c] = head[c];
            idx[m * width + width - 1] = curr_index[m];
            glob_dist[m] = curr_dist[m];
        }
    } else if (curr_dist[0] < glob_dist[ENC_SURV - 1]) {
        int m = 0;
        for (int pos = 0; pos < ENC_SURV; ++pos) {
            if (curr_dist[m] < glob_dist[pos]) {
                for (int j = ENC_SURV - 1; j >= pos + 1; --j) {
                    glob_dist[j] = glob_dist[j - 1];
                    for (int c = 0; c < width; ++c) idx[j * width + c] = idx[(j - 1) * width + c];
                }
                glob_dist[pos] = curr_dist[m];
                for (int c = 0; c < width - 1; ++c) idx[pos * width + c] = head[c];
                idx[pos * width + width - 1] = curr_index[m];
                m++;
            }
        }
    }
}

// c0_id and quantize_3stage_mbest on frame 3 of every (stream, packet) (src/lpcnet_enc.c:703-708): -> pk[1], pk[2], the quantised
// features[3][0..17] in qf3[stream][packet + 1], and in vq_mem for the chunk's last packet (:725)
__global__ __launch_bounds__(ENC_VQ_THREADS) void encode_vq_end_kernel(EncodeTables T, int n_packets, int n_items, int ipw, const float *feat /*[item][4][36]*/,
                                                                       float *qf3, int *pk, float *vq_mem)
{
    __shared__ __attribute__((aligned(16))) float cbt[ENC_NB1 * ENC_CB];
    __shared__ float xs[ENC_VQ_WAVES][ENC_END_IPW][20];
    __shared__ int idx1[ENC_VQ_WAVES][ENC_END_IPW][ENC_SURV];
    __shared__ float gd[ENC_VQ_WAVES][ENC_END_IPW][ENC_SURV];
    __shared__ int idx2[ENC_VQ_WAVES][ENC_END_IPW][ENC_SURV * 2];
    __shared__ int idx3[ENC_VQ_WAVES][ENC_END_IPW][ENC_SURV * 3];
    __shared__ float diff[ENC_VQ_WAVES][20];
    __shared__ float curd[ENC_VQ_WAVES][ENC_SURV];
    __shared__ int curi[ENC_VQ_WAVES][ENC_SURV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float od[ENC_SURV];
    int oi[ENC_SURV];
    // item of slot m; slots past the end repeat the last item and write nothing
    auto item_of = [&](const int m) { return (int)(((size_t)blockIdx.x * ipw + m) * ENC_VQ_WAVES + wv); };

    enc_stage(cbt, T.cb1_t, ENC_NB1 * ENC_CB);
    for (int m = 0; m < ipw; ++m) {
        const int item = enc_imin(item_of(m), n_items - 1);
        if (lane < ENC_NB1) xs[wv][m][lane] = feat[((size_t)item * 4 + 3) * LPCN_AN_NB_FEATURES + 1 + lane];
    }
    __syncthreads();
    for (int m = 0; m < ipw; ++m) {
        enc_search5(cbt, xs[wv][m], lane, od, oi);
        if (lane == 0) {
#pragma unroll
            for (int s = 0; s < ENC_SURV; ++s) idx1[wv][m][s] = oi[s];
        }
    }
    __syncthreads();
    enc_stage(cbt, T.cb2_t, ENC_NB1 * ENC_CB);
    __syncthreads();
#pragma unroll 1
    for (int m = 0; m < ipw; ++m) {
#pragma unroll 1
        for (int k = 0; k < ENC_SURV; ++k) {
            if (lane < ENC_NB1) diff[wv][lane] = xs[wv][m][lane] - T.cb1[idx1[wv][m][k] * ENC_NB1 + lane];
            enc_wave_sync();
            enc_search5(cbt, diff[wv], lane, od, oi);
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < ENC_SURV; ++s) { curd[wv][s] = od[s]; curi[wv][s] = oi[s]; }
                enc_merge(k, curd[wv], curi[wv], gd[wv][m], idx2[wv][m], 2, &idx1[wv][m][k]);
            }
            enc_wave_sync();
        }
    }
    __syncthreads();
    enc_stage(cbt, T.cb3_t, ENC_NB1 * ENC_CB);
    __syncthreads();
#pragma unroll 1
    for (int m = 0; m < ipw; ++m) {
#pragma unroll 1
        for (int k = 0; k < ENC_SURV; ++k) {
            if (lane < ENC_NB1) {
                float v = xs[wv][m][lane] - T.cb1[idx2[wv][m][2 * k] * ENC_NB1 + lane];
                v = v - T.cb2[idx2[wv][m][2 * k + 1] * ENC_NB1 + lane];
                diff[wv][lane] = v;
            }
            enc_wave_sync();
            enc_search5(cbt, diff[wv], lane, od, oi);
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < ENC_SURV; ++s) { curd[wv][s] = od[s]; curi[wv][s] = oi[s]; }
                enc_merge(k, curd[wv], curi[wv], gd[wv][m], idx3[wv][m], 3, &idx2[wv][m][2 * k]);
            }
            enc_wave_sync();
        }
        const int item = item_of(m);
        if (item < n_items) {
            const int stream = item / n_packets, p = item % n_packets;
            float *q = qf3 + ((size_t)stream * (n_packets + 1) + p + 1) * LPCN_NB_BANDS;
            const int e0 = idx3[wv][m][0], e1 = idx3[wv][m][1], e2 = idx3[wv][m][2];
            if (lane < ENC_NB1) {
                float v = T.cb1[e0 * ENC_NB1 + lane] + T.cb2[e1 * ENC_NB1 + lane];
                v = v + T.cb3[e2 * ENC_NB1 + lane];
                q[1 + lane] = v;
                if (p == n_packets - 1) vq_mem[(size_t)stream * LPCN_NB_BANDS + 1 + lane] = v;
            } else if (lane == ENC_NB1) {
                const float f = feat[((size_t)item * 4 + 3) * LPCN_AN_NB_FEATURES];
                int c0_id = enc_int(floor(.5 + (double)(f * 4.f)));
                c0_id = enc_imax(-64, enc_imin(63, c0_id));
                const float v = (float)c0_id / 4.f;
                q[0] = v;
                if (p == n_packets - 1) vq_mem[(size_t)stream * LPCN_NB_BANDS] = v;
                pk[(size_t)item * ENC_PK + 1] = c0_id + 64;
                pk[(size_t)item * ENC_PK + 2] = (e0 << 20) | (e1 << 10) | e2;
            }
        }
    }
}

// quantize_diff(features[1], vq_mem, features[3], ceps_codebook_diff4, 12, 1), double_interp_search and the packet
// (src/lpcnet_enc.c:709-711, :726-741).  find_nearest_multi (:243-281): entry i against target variant i & 3 -- a lane's four consecutive
// entries are the four variants --, all positive-sign entries before all negative ones, strict <.
__global__ __launch_bounds__(ENC_VQ_THREADS) void encode_vq_mid_kernel(EncodeTables T, int n_packets, int n_items, int ipw, const float *feat /*[item][4][36]*/,
                                                                       const float *qf3, const int *pk, unsigned char *packets, int packets_per_stream)
{
    __shared__ __attribute__((aligned(16))) float cq[LPCN_NB_BANDS * ENC_CB];
    __shared__ __attribute__((aligned(16))) float tg[ENC_VQ_WAVES][ENC_MID_IPW][LPCN_NB_BANDS][4];      // target[variant] per band; after the search: the interpolation terms
    __shared__ float rec_d[ENC_VQ_WAVES][ENC_MID_IPW][2];
    __shared__ int rec_i[ENC_VQ_WAVES][ENC_MID_IPW][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    auto item_of = [&](const int m) { return (int)(((size_t)blockIdx.x * ipw + m) * ENC_VQ_WAVES + wv); };

    for (int m = 0; m < ipw; ++m) {
        const int item = enc_imin(item_of(m), n_items - 1);
        const int stream = item / n_packets, p = item % n_packets;
        if (lane < LPCN_NB_BANDS) {
            const float left = qf3[((size_t)stream * (n_packets + 1) + p) * LPCN_NB_BANDS + lane];
            const float right = qf3[((size_t)stream * (n_packets + 1) + p + 1) * LPCN_NB_BANDS + lane];
            const float x = feat[((size_t)item * 4 + 1) * LPCN_AN_NB_FEATURES + lane];
            const float mid = .5f * (left + right);
            float4 t;
            t.x = x - mid; t.y = x - mid; t.z = x - left; t.w = x - right;
            *(float4 *)tg[wv][m][lane] = t;
        }
        if (lane == 0) { rec_d[wv][m][0] = 1e15f; rec_d[wv][m][1] = 1e15f; rec_i[wv][m][0] = 0; rec_i[wv][m][1] = 0; }
    }
    for (int q = 0; q < 4; ++q) {
        __syncthreads();
        enc_stage(cq, T.cbd_t + (size_t)q * LPCN_NB_BANDS * ENC_CB, LPCN_NB_BANDS * ENC_CB);
        __syncthreads();
        for (int m = 0; m < ipw; ++m) {
            float dp[16], dn[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) { dp[c] = 0.f; dn[c] = 0.f; }
            for (int j = 0; j < LPCN_NB_BANDS; ++j) {
                const float4 t = *(const float4 *)tg[wv][m][j];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const float4 c4 = *(const float4 *)(cq + j * ENC_CB + kk * 256 + 4 * lane);
                    float a;
                    a = t.x - c4.x; dp[4 * kk + 0] = dp[4 * kk + 0] + a * a;
                    a = t.y - c4.y; dp[4 * kk + 1] = dp[4 * kk + 1] + a * a;
                    a = t.z - c4.z; dp[4 * kk + 2] = dp[4 * kk + 2] + a * a;
                    a = t.w - c4.w; dp[4 * kk + 3] = dp[4 * kk + 3] + a * a;
                    a = t.x + c4.x; dn[4 * kk + 0] = dn[4 * kk + 0] + a * a;
                    a = t.y + c4.y; dn[4 * kk + 1] = dn[4 * kk + 1] + a * a;
                    a = t.z + c4.z; dn[4 * kk + 2] = dn[4 * kk + 2] + a * a;
                    a = t.w + c4.w; dn[4 * kk + 3] = dn[4 * kk + 3] + a * a;
                }
            }
            float bp = dp[0], bn = dn[0];
            int cp = 0, cn = 0;
#pragma unroll
            for (int c = 1; c < 16; ++c) {
                if (dp[c] < bp) { bp = dp[c]; cp = c; }
                if (dn[c] < bn) { bn = dn[c]; cn = c; }
            }
            int ip = q * ENC_CB + (cp >> 2) * 256 + 4 * lane + (cp & 3), in = q * ENC_CB + (cn >> 2) * 256 + 4 * lane + (cn & 3);
            enc_wave_argmin(bp, ip);
            enc_wave_argmin(bn, in);
            if (lane == 0) {      // earlier quarters hold the lower indices: strict <
                if (bp < rec_d[wv][m][0]) { rec_d[wv][m][0] = bp; rec_i[wv][m][0] = ip; }
                if (bn < rec_d[wv][m][1]) { rec_d[wv][m][1] = bn; rec_i[wv][m][1] = in; }
            }
        }
    }
    enc_wave_sync();
    for (int m = 0; m < ipw; ++m) {
        const int item = item_of(m);
        if (item >= n_items) continue;      // (wave-uniform)
        const int stream = item / n_packets, p = item % n_packets;
        const bool negative = rec_d[wv][m][1] < rec_d[wv][m][0];      // the negative pass continues from the positive pass's minimum
        const int id = negative ? rec_i[wv][m][1] : rec_i[wv][m][0];
        const int vq_mid = negative ? id + 4096 : id;
        float *terms = &tg[wv][0][0][0];       // [6][18] <= the 144 floats of this wavefront's targets, no longer needed
        enc_wave_sync();
        if (lane < LPCN_NB_BANDS) {
            const float left = qf3[((size_t)stream * (n_packets + 1) + p) * LPCN_NB_BANDS + lane];
            const float right = qf3[((size_t)stream * (n_packets + 1) + p + 1) * LPCN_NB_BANDS + lane];
            const int v = id & 3;
            const float pred = v < 2 ? .5f * (left + right) : (v == 2 ? left : right);
            const float s = negative ? -1.f : 1.f;
            const float q1 = pred + s * T.cb_diff4[(size_t)id * LPCN_NB_BANDS + lane];        // features[1], quantised (:309-311)
            const float x0 = feat[((size_t)item * 4 + 0) * LPCN_AN_NB_FEATURES + lane], x2 = feat[((size_t)item * 4 + 2) * LPCN_AN_NB_FEATURES + lane];
            // interp_search(features[0], mem, features[1]) and interp_search(features[2], features[1], features[3]) (:319-340)
            float e;
            e = x0 - .5f * (left + q1);  terms[0 * LPCN_NB_BANDS + lane] = e * e;
            e = x0 - left;               terms[1 * LPCN_NB_BANDS + lane] = e * e;
            e = x0 - q1;                 terms[2 * LPCN_NB_BANDS + lane] = e * e;
            e = x2 - .5f * (q1 + right); terms[3 * LPCN_NB_BANDS + lane] = e * e;
            e = x2 - q1;                 terms[4 * LPCN_NB_BANDS + lane] = e * e;
            e = x2 - right;              terms[5 * LPCN_NB_BANDS + lane] = e * e;
        }
        enc_wave_sync();
        float dist = 0.f;
        if (lane < 6) for (int k = 0; k < LPCN_NB_BANDS; ++k) dist = dist + terms[lane * LPCN_NB_BANDS + k];
        float dd[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) dd[k] = __shfl(dist, k);
        if (lane == 0) {
            // double_interp_search (:389-409): id 7 is forbidden
            int best_id = 0;
            float min_dist = 1e15f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const float d = dd[a] + dd[3 + b];
                    if (d < min_dist && 3 * a + b != 7) { min_dist = d; best_id = 3 * a + b; }
                }
            }
            const int interp_id = best_id - (best_id >= 7 ? 1 : 0);
            // bits_pack, MSB first: 7 + (6 + 3 + 2) + (10 + 10 + 10) + 13 + 3
            const int *k = pk + (size_t)item * ENC_PK;
            const unsigned long long word = ((unsigned long long)(k[1] & 127) << 57) | ((unsigned long long)(k[0] & 2047) << 46) |
                                            ((unsigned long long)(k[2] & 0x3fffffff) << 16) | ((unsigned long long)vq_mid << 3) | (unsigned long long)interp_id;
            unsigned char *out = packets + ((size_t)stream * packets_per_stream + p) * 8;
#pragma unroll
            for (int b = 0; b < 8; ++b) out[b] = (unsigned char)(word >> (56 - 8 * b));
        }
    }
}

}  // namespace lpcn

// the launches of one chunk of n_packets packets (4 * n_packets <= the analysis scratch's frames).  d_packets != NULL: lpcnet_encode, five
// launches, cepstrum / LPC into the scratch rows d_feat (stride 36); else lpcnet_compute_features, three launches, d_feat is the caller's.
int lpcn_launch_encode_kernels(const LpcnFrameModel &M, const lpcn::EncodeTables &T, hipStream_t st, int n, int n_packets, const short *d_pcm,
                                             size_t pcm_stream_stride, lpcn_analysis_state *d_state, float *d_feat, int feat_stride, size_t feat_stream_stride,
                                             float *d_resid, float *d_xc, float *d_fw, float *d_vq_mem, float *d_qf3, int *d_pk, unsigned char *d_packets,
                                             int packets_per_stream, char *err, size_t errlen)
{
    const int n_frames = 4 * n_packets;
    const size_t fitems = (size_t)n * n_frames, items = (size_t)n * n_packets;
    hipLaunchKernelGGL(lpcn::analysis_spectrum_kernel, dim3((unsigned)((fitems + lpcn::AN_WAVES - 1) / lpcn::AN_WAVES)), dim3(64 * lpcn::AN_WAVES), 0, st,
                       M, n, n_frames, (const void *)d_pcm, 0, pcm_stream_stride, (const lpcn_analysis_state *)d_state, d_feat, feat_stride, feat_stream_stride, d_resid);
    hipLaunchKernelGGL(lpcn::analysis_xcorr_kernel, dim3((unsigned)(fitems * 2)), dim3(lpcn::AN_XC_THREADS), 0, st,
                       n_frames, (const lpcn_analysis_state *)d_state, (const float *)d_resid, d_xc, d_fw);
    if (!d_packets) {
        hipLaunchKernelGGL(lpcn::encode_pitch_kernel<false>, dim3(n), dim3(lpcn::AN_PITCH_THREADS), 0, st, n_packets, d_pcm, pcm_stream_stride, d_state,
                           (const float *)d_resid, (const float *)d_xc, (const float *)d_fw, d_feat, feat_stride, feat_stream_stride, d_vq_mem, d_qf3, d_pk);
    } else {
        hipLaunchKernelGGL(lpcn::encode_pitch_kernel<true>, dim3(n), dim3(lpcn::AN_PITCH_THREADS), 0, st, n_packets, d_pcm, pcm_stream_stride, d_state,
                           (const float *)d_resid, (const float *)d_xc, (const float *)d_fw, d_feat, feat_stride, feat_stream_stride, d_vq_mem, d_qf3, d_pk);
        const int ipw_end = lpcn_encode_ipw(items, lpcn::ENC_END_IPW), ipw_mid = lpcn_encode_ipw(items, lpcn::ENC_MID_IPW);
        const size_t per_end = (size_t)lpcn::ENC_VQ_WAVES * ipw_end, per_mid = (size_t)lpcn::ENC_VQ_WAVES * ipw_mid;
        hipLaunchKernelGGL(lpcn::encode_vq_end_kernel, dim3((unsigned)((items + per_end - 1) / per_end)), dim3(lpcn::ENC_VQ_THREADS), 0, st,
                           T, n_packets, (int)items, ipw_end, (const float *)d_feat, d_qf3, d_pk, d_vq_mem);
        hipLaunchKernelGGL(lpcn::encode_vq_mid_kernel, dim3((unsigned)((items + per_mid - 1) / per_mid)), dim3(lpcn::ENC_VQ_THREADS), 0, st,
                           T, n_packets, (int)items, ipw_mid, (const float *)d_feat, (const float *)d_qf3, (const int *)d_pk, d_packets, packets_per_stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(err, errlen, "encode kernels: %s", hipGetErrorString(e)); return LPCN_E_HIP; }
    return 0;
}
