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
//
// An int8 (DOT_PROD) blob's decoder is the same walk, bit for bit like the reference's generic-C int8 build: that build's dense layers run on float
// weights too, so only the three GRUs differ (gru_b_i8, frame_nets.hip.h).  One body, two kernels: dred_decode_kernel<S> for a float
// block, dred_decode_i8_kernel<S> for an int8 one.
#pragma once
#include "frame_nets.hip.h"      // dense, gru_b, gru_b_i8: the layers, shared with the PLC predictor
#include <type_traits>

namespace lpcn {

constexpr int DRED_THREADS = 1024;
constexpr int DRED_REC = 4;            // per-stream record {count, first, take, first packed row}: first < 0 = the plain layout

// the widest input of a block's three GRUs (steps 1, 3, 5 of either half): the quantised input cells of an int8 block
template <typename Step>
__host__ __device__ inline int dred_gru_in(const Step *step)
{
    const int a = step[1].n_in, b = step[3].n_in, c = step[5].n_in;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// floats of dynamic LDS a workgroup of S streams needs: the concatenated buffer, the input vector, the GRUs' two scratch arrays -- and for an int8
// block the GRUs' quantised input and old state, four int8 per dword
template <typename W>
__host__ __device__ inline int dred_lds_floats(const DredNetT<W> &P, int S)
{
    const int in = P.latent_dim > P.state_dim ? P.latent_dim : P.state_dim;
    const int q = std::is_same<W, float>::value ? 0 : (dred_gru_in(P.step) + P.max_gru) / 4;
    return S * (P.total + in + 6 * P.max_gru + q);
}

// one step of the decoder's block (kernel_params.h: DredStepT): the whole workgroup takes the same branch.  xq: an int8 block's quantised cells (the
// widest GRU input's, then the widest GRU's), not read by a float block
template <int S, typename W>
__device__ __forceinline__ void dred_step(const DredStepT<W> *q, float *buf, const float *xin, float *zrh, float *recur, int *xq, int gru_in, const float *tansig,
                                          const int *live)
{
    constexpr int AD = S >= 8 ? 2 : 1;      // streams per lane in the dense layers: up to 256 rows x S / AD groups fill the workgroup
    const float *x = q->x < 0 ? xin : buf + S * q->x;
    if (q->gru) {
        const GruLayer<W> g{q->n_in, q->n_out, q->gw, q->rec, q->b, q->start, q->pos};
        if constexpr (std::is_same<W, float>::value) gru_b<S, DRED_THREADS, true>(g, x, buf + S * q->out, zrh, recur, tansig, live);
        else gru_b_i8<S, DRED_THREADS, true>(g, x, buf + S * q->out, zrh, recur, xq, xq + S * (gru_in >> 2), tansig, live);
    } else {
        float *out = buf + S * q->out;
        dense<S, AD, DRED_THREADS, 4>(q->n_in, q->n_out, q->w, q->b, x, [&](int row, int a0, const float (&acc)[AD]) {
#pragma unroll
            for (int a = 0; a < AD; ++a) out[row * S + a0 + a] = lpcn_tanh(acc[a], tansig);
        });
        __syncthreads();
    }
}

// Workgroup w decodes streams [w S, w S + S) of the n active ones.  rec [n][DRED_REC] = {count, first, take, first packed row}; state [n][state_dim],
// latents [n][max_latents][latent_dim].  first < 0: features [n][4 max_latents][20], rows below 4 count written.  Else `features` is the packed array
// and decoded row r of the stream, first <= r < first + take, goes to packed row (first packed row) + first + take - 1 - r: the oldest frame first.
// A stream whose count is below its workgroup's largest neither writes nor advances once its own latents are through.
// The body of both flavours: W = float a float blob's kernel, W = int an int8 blob's, which differ in the GRUs alone (dred_step).
template <int S, typename W>
__device__ __forceinline__ void dred_decode_body(const DredNetT<W> *P, int n, int max_latents, const int *rec, const float *state, const float *latents,
                                                 float *features)
{
    extern __shared__ float4 dred_lds[];
    __shared__ int cnt[S], live[S];
    const int total = P->total, latent_dim = P->latent_dim, state_dim = P->state_dim;
    const float *tansig = P->tansig;
    float *buf = (float *)dred_lds;
    float *xin = buf + S * total;
    float *zrh = xin + S * (latent_dim > state_dim ? latent_dim : state_dim);
    float *recur = zrh + S * 3 * P->max_gru;
    int *xq = nullptr, gru_in = 0;
    if constexpr (!std::is_same<W, float>::value) { xq = (int *)(recur + S * 3 * P->max_gru); gru_in = dred_gru_in(P->step); }
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
    for (int k = 0; k < 3; ++k) dred_step<S, W>(&P->init[k], buf, xin, zrh, recur, xq, gru_in, tansig, live);
    for (int l = 0; l < maxc; ++l) {
        if (t < S) live[t] = l < cnt[t];
        for (int e = t; e < S * latent_dim; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            xin[e] = l < cnt[a] ? latents[((size_t)(s0 + a) * max_latents + l) * latent_dim + j] : 0.f;
        }
        __syncthreads();
        // dred_rdovae_decode_qframe (src/dred_rdovae_dec.c:50-98): dense 1, GRU 2, dense 3, GRU 4, dense 5, GRU 6, dense 7, dense 8
#pragma unroll 1
        for (int k = 0; k < 8; ++k) dred_step<S, W>(&P->step[k], buf, xin, zrh, recur, xq, gru_in, tansig, live);
        // dec_final over the whole buffer, linear: one lane per (output, stream); straight to the output
        dense<S, 1, DRED_THREADS, 8>(total, LPCN_DRED_OUT, P->final_w, P->final_b, buf, [&](int i, int a, const float (&sum)[1]) {
            const float acc = sum[0];
            if (live[a]) {
                const int *q = rec + (size_t)(s0 + a) * DRED_REC;
                const int first = q[1], take = q[2], r = LPCN_DRED_FRAMES * l + i / LPCN_NB_FEAT;
                if (first < 0) features[((size_t)(s0 + a) * LPCN_DRED_FRAMES * max_latents + r) * LPCN_NB_FEAT + i % LPCN_NB_FEAT] = acc;
                else if (r >= first && r < first + take) features[((size_t)q[3] + (first + take - 1 - r)) * LPCN_NB_FEAT + i % LPCN_NB_FEAT] = acc;
            }
        });
        __syncthreads();
    }
}

template <int S>
__global__ __launch_bounds__(DRED_THREADS) void dred_decode_kernel(const DredNet *P, int n, int max_latents, const int *rec, const float *state,
                                                                    const float *latents, float *features)
{
    dred_decode_body<S, float>(P, n, max_latents, rec, state, latents, features);
}
// ... and an int8 (DOT_PROD) blob's: the dense layers float, the GRUs compute_gruB of the reference's generic-C int8 build (gru_b_i8)
template <int S>
__global__ __launch_bounds__(DRED_THREADS) void dred_decode_i8_kernel(const DredNetQ *P, int n, int max_latents, const int *rec, const float *state,
                                                                       const float *latents, float *features)
{
    dred_decode_body<S, int>(P, n, max_latents, rec, state, latents, features);
}

// ---- the decoder as a per-stream state (DRED_rdovae_dec_init_states / DRED_rdovae_decode_qframe on an RDOVAEDecState).  A stream's
// record in dstate [n][rec_floats] is the three GRU states in the reference's member order at their own widths (dense2_state, dense4_state,
// dense6_state; src/dred_rdovae_dec.h:35-39), padded to whole 16 bytes.  One body serves both calls, with the walk, the LDS layout and the order of
// every sum of dred_decode_body: the GRU segments of the buffer are computed from `state` (init) or loaded from the records (step), `count` latents
// run from `start`, and the segments go back to the records of the streams that did anything.
constexpr int DRED_SREC = 8;           // per-stream record of a call {flag, start, count, first, take, first packed row, -, -}: flag = `which` of an init

// the floats of a stream's record before the padding, and with it
template <typename W>
__host__ __device__ inline int dred_state_floats(const DredNetT<W> &P) { return P.step[1].n_out + P.step[3].n_out + P.step[5].n_out; }
template <typename W>
__host__ __device__ inline int dred_state_rec_floats(const DredNetT<W> &P) { return (dred_state_floats(P) + 3) & ~3; }

// Workgroup w serves streams [w S, w S + S) of the n active ones.  rec [n][DRED_SREC], or nullptr: every stream takes part, with latents u_start ..
// u_start + u_count - 1 (the uniform form: nothing of the launch depends on the host).  init: state [n][state_dim] -> the records of the flagged
// streams.  Else: latents start .. start + count - 1 of latents [n][max_latents][latent_dim] from the record, feature rows 4 start .. 4 (start + count)
// - 1 as dred_decode_body lays them out (first < 0: plain; else the packed array, first / take in the stream's own row numbers), the record back.
// A stream that does nothing (flag or count 0) neither writes a row nor touches its record; a workgroup of such streams returns at once.
template <int S, typename W>
__device__ __forceinline__ void dred_stream_body(const DredNetT<W> *P, int n, int max_latents, int init, const int *rec, int u_start, int u_count,
                                                 const float *state, const float *latents, float *features, float *dstate, int rec_floats)
{
    extern __shared__ float4 dred_lds[];
    __shared__ int cnt[S], live[S];
    const int total = P->total, latent_dim = P->latent_dim, state_dim = P->state_dim;
    const float *tansig = P->tansig;
    float *buf = (float *)dred_lds;
    float *xin = buf + S * total;
    float *zrh = xin + S * (latent_dim > state_dim ? latent_dim : state_dim);
    float *recur = zrh + S * 3 * P->max_gru;
    int *xq = nullptr, gru_in = 0;
    if constexpr (!std::is_same<W, float>::value) { xq = (int *)(recur + S * 3 * P->max_gru); gru_in = dred_gru_in(P->step); }
    const int s0 = blockIdx.x * S, t = threadIdx.x;
    if (t < S) {
        int c = 0;
        if (s0 + t < n) {
            const int *q = rec ? rec + (size_t)(s0 + t) * DRED_SREC : nullptr;
            c = init ? (q ? q[0] != 0 : 1) : (q ? q[2] : u_count);      // (an init "runs" one step of nothing: cnt says who takes part)
        }
        cnt[t] = c; live[t] = 1;
    }
    const auto beg = [&](int a) { return rec ? rec[(size_t)(s0 + a) * DRED_SREC + 1] : u_start; };      // (of a stream that takes part)
    __syncthreads();
    int maxc = 0;
#pragma unroll
    for (int a = 0; a < S; ++a) maxc = cnt[a] > maxc ? cnt[a] : maxc;
    if (maxc == 0) return;                  // (the whole workgroup)
    if (init) {
        for (int e = t; e < S * state_dim; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            xin[e] = cnt[a] > 0 ? state[(size_t)(s0 + a) * state_dim + j] : 0.f;
        }
        __syncthreads();
        // dred_rdovae_dec_init_states (src/dred_rdovae_dec.c:37-47): the GRU states are the GRUs' segments of the buffer
#pragma unroll 1
        for (int k = 0; k < 3; ++k) dred_step<S, W>(&P->init[k], buf, xin, zrh, recur, xq, gru_in, tansig, live);
        maxc = 0;
    } else {
        for (int g = 0, at = 0; g < 3; ++g) {
            const int w = P->step[2 * g + 1].n_out;
            float *seg = buf + S * P->step[2 * g + 1].out;
            for (int e = t; e < S * w; e += DRED_THREADS) {
                const int j = e / S, a = e % S;
                seg[e] = cnt[a] > 0 ? dstate[(size_t)(s0 + a) * rec_floats + at + j] : 0.f;
            }
            at += w;
        }
        __syncthreads();
    }
    for (int l = 0; l < maxc; ++l) {
        if (t < S) live[t] = l < cnt[t];
        for (int e = t; e < S * latent_dim; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            xin[e] = l < cnt[a] ? latents[((size_t)(s0 + a) * max_latents + beg(a) + l) * latent_dim + j] : 0.f;
        }
        __syncthreads();
        // dred_rdovae_decode_qframe (src/dred_rdovae_dec.c:50-98): dense 1, GRU 2, dense 3, GRU 4, dense 5, GRU 6, dense 7, dense 8
#pragma unroll 1
        for (int k = 0; k < 8; ++k) dred_step<S, W>(&P->step[k], buf, xin, zrh, recur, xq, gru_in, tansig, live);
        // dec_final over the whole buffer, linear: one lane per (output, stream); straight to the output
        dense<S, 1, DRED_THREADS, 8>(total, LPCN_DRED_OUT, P->final_w, P->final_b, buf, [&](int i, int a, const float (&sum)[1]) {
            const float acc = sum[0];
            if (live[a]) {
                const int r = LPCN_DRED_FRAMES * (beg(a) + l) + i / LPCN_NB_FEAT;
                int first = -1, take = 0, row = 0;
                if (rec) { const int *q = rec + (size_t)(s0 + a) * DRED_SREC; first = q[3]; take = q[4]; row = q[5]; }
                if (first < 0) features[((size_t)(s0 + a) * LPCN_DRED_FRAMES * max_latents + r) * LPCN_NB_FEAT + i % LPCN_NB_FEAT] = acc;
                else if (r >= first && r < first + take) features[((size_t)row + (first + take - 1 - r)) * LPCN_NB_FEAT + i % LPCN_NB_FEAT] = acc;
            }
        });
        __syncthreads();
    }
    // the GRU states after every stream's own last latent (the live mask kept a finished stream's still) back to the records
    for (int g = 0, at = 0; g < 3; ++g) {
        const int w = P->step[2 * g + 1].n_out;
        const float *seg = buf + S * P->step[2 * g + 1].out;
        for (int e = t; e < S * w; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            if (cnt[a] > 0) dstate[(size_t)(s0 + a) * rec_floats + at + j] = seg[e];
        }
        at += w;
    }
}

// I8: an int8 (DOT_PROD) blob's block (the second parameter keeps these apart from the one-shot kernels' names)
template <int S, bool I8>
__global__ __launch_bounds__(DRED_THREADS) void dred_stream_kernel(const DredNetT<std::conditional_t<I8, int, float>> *P, int n, int max_latents, int init,
                                                                    const int *rec, int u_start, int u_count, const float *state, const float *latents,
                                                                    float *features, float *dstate, int rec_floats)
{
    dred_stream_body<S, std::conditional_t<I8, int, float>>(P, n, max_latents, init, rec, u_start, u_count, state, latents, features, dstate, rec_floats);
}

}  // namespace lpcn
