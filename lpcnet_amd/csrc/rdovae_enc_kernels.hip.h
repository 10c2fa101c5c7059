// The DRED encoder on the device: DRED_rdovae_encode_dframe (src/dred_rdovae.c:102-105; dred_rdovae_encode_dframe, src/dred_rdovae_enc.c:38-95) for
// every stream of a batch, bit for bit like the reference's generic-C float build.  Per double frame (two 20-float feature frames, 40 inputs):
// dense 1 -> GRU 2 -> dense 3 -> GRU 4 -> dense 5 -> GRU 6 -> dense 7 -> dense 8, every output appended to one buffer; the latents are the conv1d
// bits_dense over the last `taps` buffers, linear (compute_conv1d, src/nnet.c:452-470: from the bias over the window ascending, the oldest tap first);
// the initial state is gdense2(gdense1(buffer)), both tanh.
//
// One launch encodes every active stream's double frames of a call.  The stack is the decoder's: a workgroup carries S streams whose
// activations lie side by side in LDS, and dred_step (dred_kernels.hip.h) walks the DredStep records over dense and gru_b of frame_nets.hip.h.  A
// stream's state comes from its record in global memory at the start and goes back at the end: the three GRU states are their segments of the buffer;
// the conv memory -- the taps - 1 earlier buffers -- stays in the record, a ring of taps - 1 slots that the window's sum reads from global memory (it is
// read once per double frame and lies in L2), so the LDS holds one buffer per stream whatever the taps.  A lane of the window's sum owns one (output,
// stream): one add chain of taps x total terms, the longest of a double frame.
//
// An int8 (DOT_PROD) blob's encoder is the same walk, bit for bit like the reference's generic-C int8 build: its dense layers, its conv1d and its state
// are float, only the three GRUs differ (gru_b_i8, frame_nets.hip.h).  One body, two kernels: rdovae_enc_kernel<S> for a float block,
// rdovae_enc_i8_kernel<S> for an int8 one.
#pragma once
#include "dred_kernels.hip.h"      // dred_step: the walk over DredStep records, shared with the decoder

namespace lpcn {

constexpr int RDOVAE_ENC_IN = LPCN_DRED_ENC_IN;

// floats of one stream's record: the GRU states, the ring, its head
template <typename W>
__host__ __device__ inline int rdovae_enc_rec_floats(const DredEncNetT<W> &P) { return P.gru_floats + (P.taps - 1) * P.total + 1; }
// floats of dynamic LDS a workgroup of S streams needs: the buffer with gdense1's output behind it, the input vector, the GRUs' two scratch arrays --
// and for an int8 block the GRUs' quantised input and old state, four int8 per dword
template <typename W>
__host__ __device__ inline int rdovae_enc_lds_floats(const DredEncNetT<W> &P, int S)
{
    const int q = std::is_same<W, float>::value ? 0 : (dred_gru_in(P.step) + P.max_gru) / 4;
    return S * (P.total + P.gd1 + RDOVAE_ENC_IN + 6 * P.max_gru + q);
}

// Workgroup w encodes streams [w S, w S + S) of the n active ones.  count [n] double frames per stream, or NULL: `uniform` for every one.  features
// [n][2 max_dframes][stride], the first 20 floats of a row read; state [n][rdovae_enc_rec_floats]; latents [n][max_dframes][latent_dim], initial
// [n][max_dframes][state_dim], rows below a stream's count written.  A stream whose count is below its workgroup's largest neither writes nor advances
// once its own double frames are through; one with count 0 is not touched at all.
// The body of both flavours: W = float a float blob's kernel, W = int an int8 blob's, which differ in the GRUs alone (dred_step).
template <int S, typename W>
__device__ __forceinline__ void rdovae_enc_body(const DredEncNetT<W> *P, int n, int max_dframes, const int *count, int uniform, const float *features,
                                                int stride, float *state, float *latents, float *initial)
{
    extern __shared__ float4 rdovae_enc_lds[];
    __shared__ int cnt[S], live[S], head[S];
    // (the block's fields are read where they are used, not kept: the layers' loops need the scalar registers)
    const int total = P->total;
    const float *tansig = P->tansig;
    float *buf = (float *)rdovae_enc_lds;
    float *xin = buf + S * (total + P->gd1);
    float *zrh = xin + S * RDOVAE_ENC_IN;
    float *recur = zrh + S * 3 * P->max_gru;
    int *xq = nullptr, gru_in = 0;
    if constexpr (!std::is_same<W, float>::value) { xq = (int *)(recur + S * 3 * P->max_gru); gru_in = dred_gru_in(P->step); }
    const int s0 = blockIdx.x * S, t = threadIdx.x;
    if (t < S) {
        const int c = s0 + t < n ? (count ? count[s0 + t] : uniform) : 0, rec = rdovae_enc_rec_floats(*P);
        cnt[t] = c; live[t] = 1;
        head[t] = c > 0 ? ((const int *)(state + (size_t)(s0 + t) * rec))[rec - 1] : 0;
    }
    __syncthreads();
    int maxc = 0;
#pragma unroll
    for (int a = 0; a < S; ++a) maxc = cnt[a] > maxc ? cnt[a] : maxc;
    if (maxc == 0) return;                  // (the whole workgroup)
    // the GRU states into their segments of the buffer
    for (int g = 0, at = 0; g < 3; at += P->gru_n[g], ++g) {
        const int N = P->gru_n[g], off = P->gru_off[g], rec = rdovae_enc_rec_floats(*P);
        for (int e = t; e < S * N; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            buf[(off + j) * S + a] = cnt[a] > 0 ? state[(size_t)(s0 + a) * rec + at + j] : 0.f;
        }
    }
    for (int l = 0; l < maxc; ++l) {
        if (t < S) live[t] = l < cnt[t];
        for (int e = t; e < S * RDOVAE_ENC_IN; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            xin[e] = l < cnt[a] ? features[((size_t)(s0 + a) * 2 * max_dframes + 2 * l + j / LPCN_NB_FEAT) * stride + j % LPCN_NB_FEAT] : 0.f;
        }
        __syncthreads();
        // dred_rdovae_encode_dframe (src/dred_rdovae_enc.c:52-84): dense 1, GRU 2, dense 3, GRU 4, dense 5, GRU 6, dense 7, dense 8 -- and gdense1
        // behind the buffer (:91), which the window's sum does not read
#pragma unroll 1
        for (int k = 0; k < 9; ++k) dred_step<S, W>(&P->step[k], buf, xin, zrh, recur, xq, gru_in, tansig, live);
        // bits_dense over the window (:87), linear: one lane per (output, stream), the earlier buffers from the stream's ring, this one from LDS
        {
            const int latent_dim = P->latent_dim, taps = P->taps;
            for (int it = t; it < latent_dim * S; it += DRED_THREADS) {
                const int row = it % latent_dim, a = it / latent_dim;
                if (!live[a]) continue;
                float acc = P->bits_b[row];
                const float *w = P->bits_w + row;
                const float *mem = state + (size_t)(s0 + a) * rdovae_enc_rec_floats(*P) + P->gru_floats;
                for (int i = 0; i < taps - 1; ++i) {
                    int slot = head[a] + i;
                    slot = slot >= taps - 1 ? slot - (taps - 1) : slot;
                    const float *m = mem + (size_t)slot * total;
#pragma unroll 8
                    for (int j = 0; j < total; ++j) acc = acc + w[(size_t)j * latent_dim] * m[j];
                    w += (size_t)total * latent_dim;
                }
#pragma unroll 8
                for (int j = 0; j < total; ++j) acc = acc + w[(size_t)j * latent_dim] * buf[j * S + a];
                latents[((size_t)(s0 + a) * max_dframes + l) * latent_dim + row] = acc;
            }
        }
        // gdense2 straight to the output (:93)
        {
            const int state_dim = P->state_dim;
            dense<S, 1, DRED_THREADS, 4>(P->gd1, state_dim, P->g2_w, P->g2_b, buf + S * total, [&](int i, int a, const float (&sum)[1]) {
                if (live[a]) initial[((size_t)(s0 + a) * max_dframes + l) * state_dim + i] = lpcn_tanh(sum[0], tansig);
            });
        }
        __syncthreads();                    // (every lane's window sum has read the ring)
        // compute_conv1d's shift of its memory (src/nnet.c:468-469): this buffer replaces the oldest tap, and the head moves on
        if (P->taps > 1) {
            const int rec = rdovae_enc_rec_floats(*P), gruf = P->gru_floats, last = P->taps - 2;
            for (int e = t; e < S * total; e += DRED_THREADS) {
                const int j = e / S, a = e % S;
                if (live[a]) state[(size_t)(s0 + a) * rec + gruf + (size_t)head[a] * total + j] = buf[e];
            }
            __syncthreads();
            if (t < S && live[t]) head[t] = head[t] >= last ? 0 : head[t] + 1;
        }
    }
    __syncthreads();
    for (int g = 0, at = 0; g < 3; at += P->gru_n[g], ++g) {
        const int N = P->gru_n[g], off = P->gru_off[g], rec = rdovae_enc_rec_floats(*P);
        for (int e = t; e < S * N; e += DRED_THREADS) {
            const int j = e / S, a = e % S;
            if (cnt[a] > 0) state[(size_t)(s0 + a) * rec + at + j] = buf[(off + j) * S + a];
        }
    }
    if (t < S && cnt[t] > 0) { const int rec = rdovae_enc_rec_floats(*P); ((int *)(state + (size_t)(s0 + t) * rec))[rec - 1] = head[t]; }
}

template <int S>
__global__ __launch_bounds__(DRED_THREADS) void rdovae_enc_kernel(const DredEncNet *P, int n, int max_dframes, const int *count, int uniform,
                                                                   const float *features, int stride, float *state, float *latents, float *initial)
{
    rdovae_enc_body<S, float>(P, n, max_dframes, count, uniform, features, stride, state, latents, initial);
}
// ... and an int8 (DOT_PROD) blob's: the dense layers and the state record float, the GRUs compute_gruB of the reference's generic-C int8 build
template <int S>
__global__ __launch_bounds__(DRED_THREADS) void rdovae_enc_i8_kernel(const DredEncNetQ *P, int n, int max_dframes, const int *count, int uniform,
                                                                      const float *features, int stride, float *state, float *latents, float *initial)
{
    rdovae_enc_body<S, int>(P, n, max_dframes, count, uniform, features, stride, state, latents, initial);
}

}  // namespace lpcn
