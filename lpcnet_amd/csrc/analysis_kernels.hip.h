// Feature analysis on the device: lpcnet_compute_single_frame_features (src/lpcnet_enc.c:911-933) for every stream and frame of a
// batch -- 160 PCM samples in, 36 floats out: [0..17] cepstrum, [18] pitch, [19] pitch correlation, [20..35] LPC -- bit for bit like the
// reference's generic-C float build.  Every sum keeps the reference's order, products and sums are rounded separately
// (-ffp-contract=off); double precision only where the reference has it (log10, the sqrt(2./18) product, the 10^x of the LPC path, the
// ener1 recurrence).  Three kernels per chunk of frames:
//   analysis_spectrum_kernel  one wavefront per (stream, frame): pre-emphasis, window, FFT, band energies, log10, DCT -> cepstrum;
//                             lpc_from_cepstrum -> LPC; the LPC residual before its one-tap filter -> resid
//   analysis_xcorr_kernel     one workgroup per (stream, frame, half-frame): 256-lag cross-correlation, the ener1 recurrence,
//                             normalisation, 3x interpolation -> xc, frame_weight
//   analysis_pitch_kernel     one workgroup per stream, serial over frames and half-frames: the Viterbi step of process_single_frame,
//                             the backward pass -> [18], [19]; the ONLY writer of the per-stream state
// The first two read the state and the call's PCM only, so every (stream, frame) of a chunk is independent: a frame depends on earlier
// frames through input samples and through the previous frame's residual (`pitch_filt`), which the second kernel picks up from resid.
// The first two kernels, the pitch search's half-frame step (an_viterbi_step) and the state hand-over (an_store_state) also serve the
// four-frame encoder (encode_kernels.hip.h): compute_frame_features is one function for both paths in the reference.
#pragma once
#include "lpcnet_log10.h"
#include "spectral.hip.h"

namespace lpcn {

constexpr int AN_WAVES = 4;             // wavefronts (= frames) per workgroup of the spectrum kernel
constexpr int AN_XC_THREADS = 320;      // cross-correlation: 256 lag lanes + one wavefront whose lane 0 runs the energy recurrence
constexpr int AN_PITCH_THREADS = 256;
constexpr int AN_HIST = LPCN_PITCH_MAX_PERIOD + LPCN_FRAME_SIZE;      // live part of exc_buf in single-frame analysis (416 of 576)
constexpr int AN_PATHS = LPCN_PITCH_MAX_PERIOD - LPCN_PITCH_MIN_PERIOD;

__device__ __forceinline__ float an_pcm(const void *pcm, const int is_float, const size_t i)
{
    return is_float ? ((const float *)pcm)[i] : (float)((const short *)pcm)[i];
}
// pre-emphasised sample g of the chunk (src/lpcnet_enc.c:872-880; g >= -160: negative = the state's analysis_mem): the filter memory is
// -0.85f * the previous INPUT sample, so no sample depends on another's result
__device__ __forceinline__ float an_preemph(const void *pcm, const int is_float, const size_t base, const int g, const lpcn_analysis_state *st)
{
    if (g < 0) return st->analysis_mem[LPCN_AN_OVERLAP + g];
    const float x = an_pcm(pcm, is_float, base + g);
    const float mem = g == 0 ? st->mem_preemph : -(0.85f * an_pcm(pcm, is_float, base + g - 1));
    return x + mem;
}

__global__ __launch_bounds__(64 * AN_WAVES) void analysis_spectrum_kernel(LpcnFrameModel M, int n_streams, int n_frames, const void *pcm, int is_float,
                                                                          size_t pcm_stream_stride, const lpcn_analysis_state *states, float *feat,
                                                                          int feat_stride, size_t feat_stream_stride, float *resid /*[stream][n_frames*160]*/)
{
    __shared__ cpx fbuf[AN_WAVES][320];
    __shared__ float ybuf[AN_WAVES][320];       // pre-emphasised samples -160 .. 159 of the frame
    __shared__ float exb[AN_WAVES][LPCN_NB_BANDS];
    __shared__ float lyb[AN_WAVES][LPCN_NB_BANDS];
    __shared__ float cepb[AN_WAVES][LPCN_NB_BANDS];
    __shared__ float xrb[AN_WAVES][164];
    __shared__ float lpcb[AN_WAVES][LPCN_LPC_ORDER];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t item = (size_t)blockIdx.x * AN_WAVES + wv;
    const bool valid = item < (size_t)n_streams * n_frames;
    const int stream = valid ? (int)(item / n_frames) : 0, t = valid ? (int)(item % n_frames) : 0;
    const lpcn_analysis_state *st = &states[stream];
    const size_t base = (size_t)stream * pcm_stream_stride;
    cpx *F = fbuf[wv];
    float *y = ybuf[wv], *ex = exb[wv], *ly = lyb[wv], *cep = cepb[wv];
    float *fo = feat + (size_t)stream * feat_stream_stride + (size_t)t * feat_stride;

    // the window's 320 samples: analysis_mem | frame (src/lpcnet_enc.c:488-493), windowed (src/freq.c:322-328), scaled by 1/320 into
    // digit-reversed order with a zero imaginary part (src/freq.c:242-254, src/kiss_fft.c:579-584)
    for (int k = lane; k < 320; k += 64) {
        const float v = an_preemph(pcm, is_float, base, t * LPCN_FRAME_SIZE - LPCN_AN_OVERLAP + k, st);
        y[k] = v;
        const float w = v * lpcn_half_window[k < 160 ? k : 319 - k];
        cpx z; z.r = 0.0031250000f * w; z.i = 0.0031250000f * 0.f;
        F[M.tab_bitrev[k]] = z;
    }
    __syncthreads();
    fft320_passes(F, (const cpx *)M.tab_tw, lane);
    // band energies (src/freq.c:131-154): sum[b] takes band b-1's frac*tmp terms, then band b's (1-frac)*tmp terms, j ascending
    if (lane < LPCN_NB_BANDS) {
        float sum = 0.f;
        if (lane > 0) {
            const int lo = lpcn_eband5ms[lane - 1] * 4, size = (lpcn_eband5ms[lane] - lpcn_eband5ms[lane - 1]) * 4;
            for (int j = 0; j < size; ++j) {
                const float frac = (float)j / (float)size;
                const cpx X = F[lo + j];
                float tmp = X.r * X.r;
                tmp = tmp + X.i * X.i;
                sum = sum + frac * tmp;
            }
        }
        if (lane < LPCN_NB_BANDS - 1) {
            const int lo = lpcn_eband5ms[lane] * 4, size = (lpcn_eband5ms[lane + 1] - lpcn_eband5ms[lane]) * 4;
            for (int j = 0; j < size; ++j) {
                const float frac = (float)j / (float)size;
                const cpx X = F[lo + j];
                float tmp = X.r * X.r;
                tmp = tmp + X.i * X.i;
                sum = sum + (1.f - frac) * tmp;
            }
        }
        if (lane == 0 || lane == LPCN_NB_BANDS - 1) sum = sum * 2.f;
        // log10 of a double argument, rounded to float (src/lpcnet_enc.c:513): lpcnet_log10.h, not the device math library
        ly[lane] = lpcn_log10f_of_double(1e-2 + (double)sum);
    }
    __syncthreads();
    // floor follower (src/lpcnet_enc.c:510-518): 18 serial steps
    if (lane == 0) {
        float logMax = -2.f, follow = -2.f;
        for (int i = 0; i < LPCN_NB_BANDS; ++i) {
            float v = ly[i];
            const float f25 = follow - 2.5f, m8 = logMax - 8.f;
            const float inner = LPCN_MAX16(f25, v);
            v = LPCN_MAX16(m8, inner);
            logMax = LPCN_MAX16(logMax, v);
            follow = LPCN_MAX16(f25, v);
            ex[i] = v;
        }
    }
    __syncthreads();
    // DCT (src/freq.c:218-228): float sum, product with sqrt(2./18) in double; c0 - 4 (src/lpcnet_enc.c:520)
    if (lane < LPCN_NB_BANDS) {
        float sum = 0.f;
        for (int j = 0; j < LPCN_NB_BANDS; ++j) sum = sum + ex[j] * M.tab_idct[j * LPCN_NB_BANDS + lane];
        float c = (float)((double)sum * sqrt(2. / LPCN_NB_BANDS));
        if (lane == 0) c = c - 4.f;
        cep[lane] = c;
        if (valid) fo[lane] = c;
    }
    __syncthreads();
    // LPC from the cepstrum (src/lpcnet_enc.c:521-522; no lpc_weighting in the analysis)
    float lpc[LPCN_LPC_ORDER];
    lpc_from_cepstrum_wave(M, cep, F, ex, xrb[wv], lane, true, lpc);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < LPCN_LPC_ORDER; ++k) { lpcb[wv][k] = lpc[k]; if (valid) fo[LPCN_NB_BANDS + 2 + k] = lpc[k]; }
    }
    __syncthreads();
    // LPC residual of the input delayed by 80 samples (src/lpcnet_enc.c:523-532), before the one-tap filter of :533: an FIR over y
    if (valid) {
        float *r = resid + ((size_t)stream * n_frames + t) * LPCN_FRAME_SIZE;
        for (int i = lane; i < LPCN_FRAME_SIZE; i += 64) {
            const float *a = y + LPCN_AN_OVERLAP - LPCN_AN_TRAINING_OFFSET + i;      // aligned_in[i]
            float sum = a[0];
#pragma unroll
            for (int j = 0; j < LPCN_LPC_ORDER; ++j) sum = sum + lpcb[wv][j] * a[-1 - j];
            r[i] = sum;
        }
    }
}

// excitation sample p of the chunk (p >= -256; negative = the state's exc_buf): exc = sum + .7f * previous sum (src/lpcnet_enc.c:533-534)
__device__ __forceinline__ float an_exc(const float *resid, const int p, const lpcn_analysis_state *st)
{
    if (p < 0) return st->exc_buf[AN_HIST + p];
    const float prev = p == 0 ? st->pitch_filt : resid[p - 1];
    return resid[p] + .7f * prev;
}

__global__ __launch_bounds__(AN_XC_THREADS) void analysis_xcorr_kernel(int n_frames, const lpcn_analysis_state *states, const float *resid,
                                                                       float *xc_out /*[stream][frame][2][256]*/, float *fw_out /*[stream][frame][2]*/)
{
    __shared__ float w[336];        // exc_buf[off .. off + 336): y = w, x = w + 256
    __shared__ float enr[LPCN_PITCH_MAX_PERIOD];
    __shared__ float xcs[LPCN_PITCH_MAX_PERIOD];
    const int tid = threadIdx.x;
    const size_t item = blockIdx.x >> 1;                    // (stream, frame)
    const int sub = blockIdx.x & 1;
    const int stream = (int)(item / n_frames), t = (int)(item % n_frames);
    const lpcn_analysis_state *st = &states[stream];
    const float *r = resid + (size_t)stream * n_frames * LPCN_FRAME_SIZE;
    const int p0 = t * LPCN_FRAME_SIZE - LPCN_PITCH_MAX_PERIOD + sub * (LPCN_FRAME_SIZE / 2);
    for (int k = tid; k < 336; k += AN_XC_THREADS) w[k] = an_exc(r, p0 + k, st);
    __syncthreads();
    float xs = 0.f;
    if (tid < LPCN_PITCH_MAX_PERIOD) {
        // celt_pitch_xcorr (src/pitch.c:43-83): one accumulator per lag, j ascending
        const float *x = w + LPCN_PITCH_MAX_PERIOD, *yy = w + tid;
#pragma unroll 8
        for (int j = 0; j < LPCN_FRAME_SIZE / 2; ++j) xs = xs + x[j] * yy[j];
    } else if (tid == LPCN_PITCH_MAX_PERIOD) {
        // ener0 (float), ener1 (a double running sum of float squares), ener = 1 + ener0 + ener1 (src/lpcnet_enc.c:541-551)
        const float *x = w + LPCN_PITCH_MAX_PERIOD;
        float ener0 = 0.f, e1 = 0.f;
        for (int j = 0; j < LPCN_FRAME_SIZE / 2; ++j) ener0 = ener0 + x[j] * x[j];
        for (int j = 0; j < LPCN_FRAME_SIZE / 2 - 1; ++j) e1 = e1 + w[j] * w[j];
        double ener1 = (double)e1;
        const float one_ener0 = 1.f + ener0;
#pragma unroll 4
        for (int i = 0; i < LPCN_PITCH_MAX_PERIOD; ++i) {
            const float a = w[i + LPCN_FRAME_SIZE / 2 - 1], b = w[i];
            ener1 = ener1 + (double)(a * a);
            enr[i] = (float)((double)one_ener0 + ener1);
            ener1 = ener1 - (double)(b * b);
        }
        fw_out[item * 2 + sub] = ener0;
    }
    __syncthreads();
    if (tid < LPCN_PITCH_MAX_PERIOD) xcs[tid] = (2.f * xs) / enr[tid];
    __syncthreads();
    if (tid < LPCN_PITCH_MAX_PERIOD) {
        // 3x upsampling, keep the max (src/lpcnet_enc.c:552-567): lags 4..251
        float v = xcs[tid];
        if (tid >= 4 && tid < LPCN_PITCH_MAX_PERIOD - 4) {
            const float interp[7] = {0.026184f, -0.098339f, 0.369938f, 0.837891f, -0.184969f, 0.070242f, -0.020947f};
            float val1 = 0.f, val2 = 0.f;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                val1 = val1 + xcs[tid - 3 + j] * interp[j];
                val2 = val2 + xcs[tid + 3 - j] * interp[j];
            }
            const float m12 = LPCN_MAX16(val1, val2);
            v = LPCN_MAX16(v, m12);
        }
        xc_out[(item * 2 + sub) * LPCN_PITCH_MAX_PERIOD + tid] = v;
    }
}

// One half-frame of the pitch search, the same in process_single_frame (src/lpcnet_enc.c:828-852) and process_superframe (:622-646):
// the *= .8f pass on the half-frame's cross-correlation (lane i holds lag i, `v`), one Viterbi step over the 224 pitch candidates with
// weight `fw`, renormalisation.  Leaves the modified cross-correlation in xcw[256], the predecessors in prevs[224], the new path
// scores in pmp[224] and (max_path_all, best_i) in pmpa / best_i.  Called by all AN_PITCH_THREADS lanes of the workgroup.
__device__ __forceinline__ void an_viterbi_step(const int i, float v, const float fw, float *xcw, short *prevs, float *pmp, float *red_v, int *red_i,
                                                float &pmpa, int &best_i)
{
    xcw[i] = v;
    __syncthreads();
    // the *= .8f pass reads only entries above the one it writes ((255 + i)/2 > i for i < 192): parallel
    if (i < LPCN_PITCH_MAX_PERIOD - 2 * LPCN_PITCH_MIN_PERIOD) {
        const float a = xcw[(LPCN_PITCH_MAX_PERIOD + i) / 2], b = xcw[(LPCN_PITCH_MAX_PERIOD + i + 2) / 2];
        const float c = xcw[(LPCN_PITCH_MAX_PERIOD + i - 1) / 2];
        const float ab = LPCN_MAX16(a, b);
        const float xc_half = LPCN_MAX16(ab, c);
        if (v < xc_half * 1.1f) v = v * .8f;
    }
    __syncthreads();
    xcw[i] = v;
    // 9 neighbours from -4 upwards, strict >
    float nv = -1e15f;
    if (i < AN_PATHS) {
        float max_prev = pmpa - 6.f;
        int pp = best_i;
#pragma unroll
        for (int j = -4; j <= 4; ++j) {
            if (i + j >= 0 && i + j < AN_PATHS) {
                const int aj = j < 0 ? -j : j;
                const float cand = pmp[i + j] - (.02f * (float)aj) * (float)aj;
                if (cand > max_prev) { max_prev = cand; pp = i + j; }
            }
        }
        prevs[i] = (short)pp;
        nv = max_prev + fw * v;
    }
    // argmax, the lowest index winning ties, starting from (-1e15f, 0)
    float bv = nv;
    int bi = i < AN_PATHS ? i : 0x7fffffff;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int oi = __shfl_xor(bi, d);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((i & 63) == 0) { red_v[i >> 6] = bv; red_i[i >> 6] = bi; }
    __syncthreads();      // (also: every lane has read its pmp neighbours)
    bv = red_v[0]; bi = red_i[0];
#pragma unroll
    for (int k = 1; k < AN_PITCH_THREADS / 64; ++k) {
        const float ov = red_v[k];
        const int oi = red_i[k];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (!(bv > -1e15f)) { bv = -1e15f; bi = 0; }
    if (i < AN_PATHS) pmp[i] = nv - bv;        // renormalise
    pmpa = bv;
    best_i = bi;
    __syncthreads();
}

// The state after T frames of the chunk (what compute_frame_features leaves behind, plus the path scores): everything is read into
// registers before anything is written.  amb: LPCN_AN_OVERLAP floats of LDS.
__device__ __forceinline__ void an_store_state(const int i, const int T, const void *pcm, const int is_float, const size_t base, const float *r,
                                               lpcn_analysis_state *st, const float *pmp, float *amb, const float pmpa, const int best_i)
{
    float e0 = 0.f, e1 = 0.f, am = 0.f;
    e0 = an_exc(r, T * LPCN_FRAME_SIZE - AN_HIST + i, st);
    if (i + AN_PITCH_THREADS < AN_HIST) e1 = an_exc(r, T * LPCN_FRAME_SIZE - AN_HIST + i + AN_PITCH_THREADS, st);
    if (i < LPCN_AN_OVERLAP) am = an_preemph(pcm, is_float, base, (T - 1) * LPCN_FRAME_SIZE + i, st);
    const float last_x = an_pcm(pcm, is_float, base + (size_t)T * LPCN_FRAME_SIZE - 1);
    const float last_sum = r[T * LPCN_FRAME_SIZE - 1];
    if (i < LPCN_AN_OVERLAP) amb[i] = am;
    __syncthreads();
    st->exc_buf[i] = e0;
    if (i + AN_PITCH_THREADS < AN_HIST) st->exc_buf[i + AN_PITCH_THREADS] = e1;
    if (i < LPCN_AN_OVERLAP) st->analysis_mem[i] = am;
    if (i < LPCN_LPC_ORDER) st->pitch_mem[i] = amb[LPCN_AN_OVERLAP - LPCN_AN_TRAINING_OFFSET - 1 - i];
    if (i < AN_PATHS) st->pitch_max_path[i] = pmp[i];
    if (i == 0) {
        st->mem_preemph = -(0.85f * last_x);
        st->pitch_filt = last_sum;
        st->pitch_max_path_all = pmpa;
        st->best_i = best_i;
    }
}

// process_single_frame (src/lpcnet_enc.c:814-870) for every frame of the chunk, and the state the next chunk starts from
__global__ __launch_bounds__(AN_PITCH_THREADS) void analysis_pitch_kernel(int n_frames, const void *pcm, int is_float, size_t pcm_stream_stride,
                                                                          lpcn_analysis_state *states, const float *resid, const float *xc_in,
                                                                          const float *fw_in, float *feat, int feat_stride, size_t feat_stream_stride)
{
    __shared__ float pmp[AN_PATHS];
    __shared__ float xcw[2][LPCN_PITCH_MAX_PERIOD];
    __shared__ short prevs[2][AN_PATHS];
    __shared__ float red_v[AN_PITCH_THREADS / 64];
    __shared__ int red_i[AN_PITCH_THREADS / 64];
    const int i = threadIdx.x;
    const int stream = blockIdx.x;
    lpcn_analysis_state *st = &states[stream];
    const float *r = resid + (size_t)stream * n_frames * LPCN_FRAME_SIZE;
    const size_t base = (size_t)stream * pcm_stream_stride;
    if (i < AN_PATHS) pmp[i] = st->pitch_max_path[i];
    float pmpa = st->pitch_max_path_all;
    int best_i = st->best_i;
    __syncthreads();
    for (int t = 0; t < n_frames; ++t) {
        const size_t item = (size_t)stream * n_frames + t;
        // weights normalised by 2 / (1e-15f + w0 + w1) (:822-824)
        float fsum = 1e-15f;
        fsum = fsum + fw_in[item * 2];
        fsum = fsum + fw_in[item * 2 + 1];
        const float scale = 2.f / fsum;
        const float fw0 = fw_in[item * 2] * scale, fw1 = fw_in[item * 2 + 1] * scale;
        for (int sub = 0; sub < 2; ++sub)
            an_viterbi_step(i, xc_in[(item * 2 + sub) * LPCN_PITCH_MAX_PERIOD + i], sub ? fw1 : fw0, xcw[sub], prevs[sub], pmp, red_v, red_i, pmpa, best_i);
        // backward pass (:858-866)
        if (i == 0) {
            int b = best_i;
            const int best3 = LPCN_PITCH_MAX_PERIOD - b;
            float frame_corr = 0.f + fw1 * xcw[1][b];
            b = prevs[1][b];
            const int best2 = LPCN_PITCH_MAX_PERIOD - b;
            frame_corr = frame_corr + fw0 * xcw[0][b];
            frame_corr = frame_corr / 2.f;
            int period = best2 + best3;
            period = period < 510 ? period : 510;
            period = period > 66 ? period : 66;
            float *fo = feat + (size_t)stream * feat_stream_stride + (size_t)t * feat_stride;
            fo[LPCN_NB_BANDS] = .01f * (float)(period - 200);
            fo[LPCN_NB_BANDS + 1] = frame_corr - .5f;
        }
        __syncthreads();
    }
    __shared__ float amb[LPCN_AN_OVERLAP];
    an_store_state(i, n_frames, pcm, is_float, base, r, st, pmp, amb, pmpa, best_i);
}

}  // namespace lpcn

// the three launches of one chunk (n_frames <= the scratch buffers' capacity)
int lpcn_launch_analysis_kernels(const LpcnFrameModel &M, hipStream_t st, int n, int n_frames, const void *d_pcm, int is_float,
                                               size_t pcm_stream_stride, lpcn_analysis_state *d_state, float *d_feat, int feat_stride,
                                               size_t feat_stream_stride, float *d_resid, float *d_xc, float *d_fw, char *err, size_t errlen)
{
    const size_t items = (size_t)n * n_frames;
    hipLaunchKernelGGL(lpcn::analysis_spectrum_kernel, dim3((unsigned)((items + lpcn::AN_WAVES - 1) / lpcn::AN_WAVES)), dim3(64 * lpcn::AN_WAVES), 0, st,
                       M, n, n_frames, d_pcm, is_float, pcm_stream_stride, (const lpcn_analysis_state *)d_state, d_feat, feat_stride, feat_stream_stride, d_resid);
    hipLaunchKernelGGL(lpcn::analysis_xcorr_kernel, dim3((unsigned)(items * 2)), dim3(lpcn::AN_XC_THREADS), 0, st,
                       n_frames, (const lpcn_analysis_state *)d_state, (const float *)d_resid, d_xc, d_fw);
    hipLaunchKernelGGL(lpcn::analysis_pitch_kernel, dim3(n), dim3(lpcn::AN_PITCH_THREADS), 0, st,
                       n_frames, d_pcm, is_float, pcm_stream_stride, d_state, (const float *)d_resid, (const float *)d_xc, (const float *)d_fw,
                       d_feat, feat_stride, feat_stream_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(err, errlen, "analysis kernels: %s", hipGetErrorString(e)); return LPCN_E_HIP; }
    return 0;
}
