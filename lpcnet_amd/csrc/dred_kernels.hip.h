// The DRED decoder on the device: DRED_rdovae_decode_all (src/dred_rdovae.c:38-52) for every stream of a batch, bit for bit like the reference's
// generic-C float build.  dred_rdovae_dec_init_states (src/dred_rdovae_dec.c:37-47) turns the initial state into the three GRU states; then
// dred_rdovae_decode_qframe (:50-98) runs per latent dense 1 -> GRU 2 -> dense 3 -> GRU 4 -> dense 5 -> GRU 6 -> dense 7 -> dense 8, appends every
// output to one buffer and applies dec_final to the whole buffer: 80 floats, four feature frames.
//
// One launch decodes every stream's whole chain.  A workgroup carries S streams: their activations lie side by side in LDS,
// cell [j][S], so the S values of one input j are one broadcast read.  A lane owns an output row and A of the S streams: it loads each weight of
// the row once and applies it to A accumulators, one separately ordered add chain per stream -- the order of every sum is the reference's
// (_lpcnet_compute_dense src/nnet.c:122-135 from the bias over the columns ascending; compute_gruB :326-372 with bias + 0.f, the 8x4 block list in
// list order, the recurrent sum ascending; products and sums rounded separately, -ffp-contract=off).  The GRUs hold most of the weights and take
// A = S: every recurrent weight is read once per workgroup and latent.  The dense layers have few rows (dec_final: 80), so their streams are dealt
// over lanes instead (A < S): their matrices are small and stay in L2.  The GRU states are their segments of the concatenated buffer: nothing of
// the chain goes to global memory but the features.
#pragma once
#include "kernel_params.h"
#include "lpcnet_math.h"

namespace lpcn {

constexpr int DRED_THREADS = 1024;
constexpr int DRED_REC = 4;            // per-stream record {count, first, take, first packed row}: first < 0 = the plain layout

// floats of dynamic LDS a workgroup of S streams needs: the concatenated buffer, the input vector, the GRUs' two scratch arrays
__host__ __device__ inline int dred_lds_floats(const DredNet &P, int S)
{
    const int in = P.latent_dim > P.state_dim ? P.latent_dim : P.state_dim;
    return S * (P.total + in + 6 * P.max_gru);
}

template <int A>
__device__ __forceinline__ void dred_load(float (&v)[A], const float *p)
{
    if constexpr (A == 8) {
        const float4 a = ((const float4 *)p)[0], b = ((const float4 *)p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if constexpr (A == 4) {
        const float4 a = *(const float4 *)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (A == 2) {
        const float2 a = *(const float2 *)p;
        v[0] = a.x; v[1] = a.y;
    } else {
        v[0] = p[0];
    }
}

// _lpcnet_compute_dense (src/nnet.c:122-135), tanh.  x [n_in][S] in LDS.  Item = (row, group of A streams); out [n_out][S] in LDS
template <int S, int A>
__device__ __forceinline__ void dred_dense(const int n_in, const int n_out, const float *W, const float *B, const float *x, float *out, const float *tansig)
{
    const int items = n_out * (S / A);
    for (int it = threadIdx.x; it < items; it += DRED_THREADS) {
        const int row = it % n_out, a0 = (it / n_out) * A;
        float acc[A];
        const float b = B[row];
#pragma unroll
        for (int a = 0; a < A; ++a) acc[a] = b;
        const float *w = W + row;
        const float *xp = x + a0;
#pragma unroll 4
        for (int j = 0; j < n_in; ++j) {
            const float wv = w[(size_t)j * n_out];
            float xv[A];
            dred_load<A>(xv, xp + j * S);
#pragma unroll
            for (int a = 0; a < A; ++a) acc[a] = acc[a] + wv * xv[a];
        }
#pragma unroll
        for (int a = 0; a < A; ++a) out[row * S + a0 + a] = lpcn_tanh(acc[a], tansig);
    }
}

// compute_gruB with a zero condition (src/nnet.c:326-372, float build: sparse_sgemv_accum8x4 src/vec.h:347-403, sgemv_accum src/nnet.c:73-86), the
// arithmetic of plc_gru (plc_kernels.hip.h) on S streams: lane = row, all S streams.  x [n_in][S] and hs [N][S] (the state; replaced for the streams
// with live[a] set) in LDS; zrh / recur [3 N][S] LDS scratch.
template <int S>
__device__ __forceinline__ void dred_gru(const int N, const float *W, const int *start, const int *pos, const float *Rw, const float *bias,
                                         const float *x, float *hs, float *zrh, float *recur, const float *tansig, const int *live)
{
    const int rows = 3 * N;
    for (int row = threadIdx.x; row < rows; row += DRED_THREADS) {
        float z[S];
        const float b0 = bias[row] + 0.f;
#pragma unroll
        for (int a = 0; a < S; ++a) z[a] = b0;
        const int grp = row >> 3, r = row & 7;
        for (int blk = start[grp]; blk < start[grp + 1]; ++blk) {
            const float *w = W + (size_t)blk * 32 + r;
            const float *xp = x + pos[blk] * S;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float wv = w[8 * c];
                float xv[S];
                dred_load<S>(xv, xp + c * S);
#pragma unroll
                for (int a = 0; a < S; ++a) z[a] = z[a] + wv * xv[a];
            }
        }
#pragma unroll
        for (int a = 0; a < S; ++a) zrh[row * S + a] = z[a];
        float rc[S];
        const float b1 = bias[rows + row];
#pragma unroll
        for (int a = 0; a < S; ++a) rc[a] = b1;
        const float *R = Rw + row;
#pragma unroll 4
        for (int j = 0; j < N; ++j) {
            const float wv = R[(size_t)j * rows];
            float hv[S];
            dred_load<S>(hv, hs + j * S);
#pragma unroll
            for (int a = 0; a < S; ++a) rc[a] = rc[a] + wv * hv[a];
        }
#pragma unroll
        for (int a = 0; a < S; ++a) recur[row * S + a] = rc[a];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * N * S; i += DRED_THREADS) zrh[i] = lpcn_sigmoid(zrh[i] + recur[i], tansig);
    __syncthreads();
    // cell e = unit * S + stream: a lane reads and writes only its own cells of the state
    for (int e = threadIdx.x; e < N * S; e += DRED_THREADS) {
        float hh = zrh[2 * N * S + e] + recur[2 * N * S + e] * zrh[N * S + e];
        hh = lpcn_tanh(hh, tansig);
        const float z = zrh[e];
        const float hn = z * hs[e] + (1.f - z) * hh;
        if (live[e % S]) hs[e] = hn;
    }
    __syncthreads();
}

// one step of the decoder's block (kernel_params.h: DredStep): the whole workgroup takes the same branch
template <int S>
__device__ __forceinline__ void dred_step(const DredStep *q, float *buf, const float *xin, float *zrh, float *recur, const float *tansig, const int *live)
{
    constexpr int AD = S >= 8 ? 2 : 1;      // streams per lane in the dense layers: up to 256 rows x S / AD groups fill the workgroup
    const float *x = q->x < 0 ? xin : buf + S * q->x;
    if (q->gru) {
        dred_gru<S>(q->n_out, q->w, q->start, q->pos, q->rec, q->b, x, buf + S * q->out, zrh, recur, tansig, live);
    } else {
        dred_dense<S, AD>(q->n_in, q->n_out, q->w, q->b, x, buf + S * q->out, tansig);
        __syncthreads();
    }
}

// Workgroup w decodes streams [w S, w S + S) of the n active ones.  rec [n][DRED_REC] = {count, first, take, first packed row}; state [n][state_dim],
// latents [n][max_latents][latent_dim].  first < 0: features [n][4 max_latents][20], rows below 4 count written.  Else `features` is the packed array
// and decoded row r of the stream, first <= r < first + take, goes to packed row (first packed row) + first + take - 1 - r: the oldest frame first.
// A stream whose count is below its workgroup's largest neither writes nor advances once its own latents are through.
template <int S>
__global__ __launch_bounds__(DRED_THREADS) void dred_decode_kernel(const DredNet *P, int n, int max_latents, const int *rec, const float *state,
                                                                    const float *latents, float *features)
{
    extern __shared__ float4 dred_lds[];
    __shared__ int cnt[S], live[S];
    const int total = P->total, latent_dim = P->latent_dim, state_dim = P->state_dim;
    const float *tansig = P->tansig;
    float *buf = (float *)dred_lds;
    float *xin = buf + S * total;
    float *zrh = xin + S * (latent_dim > state_dim ? latent_dim : state_dim);
    float *recur = zrh + S * 3 * P->max_gru;
    const int s0 = blockIdx.x * S, t = threadIdx.x;
    if (t < S) { cnt[t] = s0 + t < n ? rec[(size_t)(s0 + t) * DRED_REC] : 0; live[t] = 1; }
    __syncthreads();
    int maxc = 0;
#pragma unroll
    for (int a = 0; a < S; ++a) maxc = cnt[a] > maxc ? cnt[a] : maxc;
    if (maxc == 0) return;                  // (the whole workgroup)
    for (int e = t; e < S * state_dim; e += DRED_THREADS) {
        const int j = e / S, a = e % S;
        xin[e] = cnt[a] > 0 ? state[(size_t)(s0 + a) * state_dim + j] : 0.f;
    }
    __syncthreads();
    // dred_rdovae_dec_init_states (src/dred_rdovae_dec.c:37-47): the GRU states are the GRUs' segments of the buffer
#pragma unroll 1
    for (int k = 0; k < 3; ++k) dred_step<S>(&P->init[k], buf, xin, zrh, recur, tansig, live);
    for (int l = 0; l < maxc; ++l) {
        if (t < S) live[t] = l < cnt[t];
        for (int e = t; e < S * latent_dim; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            xin[e] = l < cnt[a] ? latents[((size_t)(s0 + a) * max_latents + l) * latent_dim + j] : 0.f;
        }
        __syncthreads();
        // dred_rdovae_decode_qframe (src/dred_rdovae_dec.c:50-98): dense 1, GRU 2, dense 3, GRU 4, dense 5, GRU 6, dense 7, dense 8
#pragma unroll 1
        for (int k = 0; k < 8; ++k) dred_step<S>(&P->step[k], buf, xin, zrh, recur, tansig, live);
        // dec_final over the whole buffer, linear: one lane per (output, stream); straight to the output
        for (int it = t; it < LPCN_DRED_OUT * S; it += DRED_THREADS) {
            const int i = it % LPCN_DRED_OUT, a = it / LPCN_DRED_OUT;
            float acc = P->final_b[i];
            const float *w = P->final_w + i;
            const float *xp = buf + a;
#pragma unroll 8
            for (int j = 0; j < total; ++j) acc = acc + w[(size_t)j * LPCN_DRED_OUT] * xp[j * S];
            if (live[a]) {
                const int *q = rec + (size_t)(s0 + a) * DRED_REC;
                const int first = q[1], take = q[2], r = LPCN_DRED_FRAMES * l + i / LPCN_NB_FEAT;
                if (first < 0) features[((size_t)(s0 + a) * LPCN_DRED_FRAMES * max_latents + r) * LPCN_NB_FEAT + i % LPCN_NB_FEAT] = acc;
                else if (r >= first && r < first + take) features[((size_t)q[3] + (first + take - 1 - r)) * LPCN_NB_FEAT + i % LPCN_NB_FEAT] = acc;
            }
        }
        __syncthreads();
    }
}

}  // namespace lpcn
