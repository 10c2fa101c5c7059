// The DRED decoder's FAST flavour (lpcnet_batch_dred_set_fast): the same network as dred_decode_kernel in the arithmetic of the
// reference's AVX2+FMA float build, with the streams of a workgroup on the column index of an fp32 MFMA.
//
// Arithmetic.  Every sum is ONE fma chain from its bias in ascending input order, as sgemv_accum16 (src/vec_avx.h:618-643) and sparse_sgemv_accum8x4
// (:865-903) compute it: a dense row from bias[i] over j ascending; a GRU's input part from bias[i] over the row group's blocks in list order, four
// columns each; its recurrent part from bias[3 N + i] over j ascending; dec_final from its bias over the layers' outputs in the order they are
// produced.  v_mfma_f32_32x32x2_f32 and v_mfma_f32_16x16x4_f32 are exactly that chain (D = fma(a1, b1, fma(a0, b0, C)) ..., one rounding per step),
// so no sum is ever split over k, and a stream's bits are the same in both.
// The activations are exp / rcp based (tanh x = 1 - 2 / (1 + e^2x), sigmoid x = 1 / (1 + e^-x) on v_exp_f32 / v_rcp_f32), the GRU update is
// h' = fma(z, h, (1 - z) tanh(fma(rec_h, r, in_h))).
//
// Layout.  A workgroup carries T streams through their whole latent chain: T = 32 on the 32x32x2 MFMA (one per step of two inputs), T = 16 on the
// 16x16x4 MFMA (two per step of four inputs: a wave's 32 rows are two row tiles).  A layer is W[rows x K] . X[K x T]: a wave owns 32 rows, reads its
// A operand straight from the blob's [k][rows] arrays (128 bytes per k; the sparse GRU input matrices from the union-packed image of
// dred_fast_pack.h) and its B operand from LDS, where the activations lie as [k][T].  LDS holds the three GRU states and ONE activation buffer: a
// layer computes into accumulators, the workgroup meets at a barrier behind the last reader of what the layer overwrites, then it writes.  The
// concatenated buffer of the PARITY kernel does not exist: dec_final's 80 x T accumulators live in three waves of their own, which advance them over
// a layer's output while the layer waves compute the next layer.  A GRU wave owns the z, r and h rows of 32 units, input and recurrent part, and
// closes the update in registers.
//
// A stream's column never meets another's: its bits do not depend on which streams share its tile, on their counts or on the active prefix.
#pragma once
#include "kernel_params.h"
#include "dred_kernels.hip.h"      // DRED_REC

namespace lpcn {

constexpr int DRED_FAST_LAYER_WAVES = LPCN_DRED_MAX_UNITS / 32;         // one 32-row tile each: the widest layer has 256 rows (per gate)
constexpr int DRED_FAST_FINAL_WAVES = (LPCN_DRED_OUT + 31) / 32;
constexpr int DRED_FAST_THREADS = 64 * (DRED_FAST_LAYER_WAVES + DRED_FAST_FINAL_WAVES + 1);     // (twelve waves, three per SIMD; the twelfth only helps to copy
                                                                                                 // the latents in and meets the barriers)

using dred_f32x16 = __attribute__((ext_vector_type(16))) float;
using dred_f32x4 = __attribute__((ext_vector_type(4))) float;
using dred_gfloat = __attribute__((address_space(1))) float;
using dred_gchar = __attribute__((address_space(1))) char;

__device__ __forceinline__ float dred_fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504f * x)); }
__device__ __forceinline__ float dred_fast_tanh(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(2.88539008f * x)); }

// a wave-uniform pointer, said so to the compiler: the loads through it take a scalar base and a 32-bit lane offset instead of a 64-bit address per lane
template <typename P>
__device__ __forceinline__ P *dred_fast_uniform(P *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (P *)((unsigned long long)hi << 32 | lo);
}

// floats of dynamic LDS, every buffer in whole tiles of 32 rows, so that a partial tile is written and read like a whole one (its rows past the layer's
// last are never an input): the three GRU states, the activation buffer (the widest of the latent, the initial state and the dense layers), [k][T]
__host__ __device__ inline int dred_fast_pad(int rows) { return (rows + 31) & ~31; }
__host__ __device__ inline int dred_fast_act_rows(const DredNet &P)
{
    int m = P.latent_dim > P.state_dim ? P.latent_dim : P.state_dim;
    for (int k = 0; k < 8; ++k) if (!P.step[k].gru && P.step[k].n_out > m) m = P.step[k].n_out;
    return m;
}
__host__ __device__ inline int dred_fast_lds_floats(const DredNet &P, int T)
{
    return T * (dred_fast_pad(P.step[1].n_out) + dred_fast_pad(P.step[3].n_out) + dred_fast_pad(P.step[5].n_out) + dred_fast_pad(dred_fast_act_rows(P)));
}

// A wave's 32 rows x T streams of accumulators and the MFMA that advances them by one step of KS = 64 / T inputs.  Lane l holds column l % T of B and
// input KS s + l / T of step s; of A it holds that input's weight of row l % T of every row tile (NJ: one tile of 32 rows at T = 32, two of 16 at
// T = 16).  An element e < NE of the lane is row (e & 3) + RUN (e >> 2) + 4 (l / T) of the 32, column l % T: runs of four consecutive rows
template <int T> struct DredFastAcc;
template <> struct DredFastAcc<32> {
    static constexpr int NJ = 1, NE = 16, RUN = 8;
    dred_f32x16 v;
    __device__ __forceinline__ float get(int e) const { return v[e]; }
    __device__ __forceinline__ void set(int e, float x) { v[e] = x; }
    __device__ __forceinline__ void mma(const float (&a)[1], float b) { v = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b, v, 0, 0, 0); }
};
template <> struct DredFastAcc<16> {
    static constexpr int NJ = 2, NE = 8, RUN = 16;
    dred_f32x4 v[2];
    __device__ __forceinline__ float get(int e) const { return v[e >> 2][e & 3]; }
    __device__ __forceinline__ void set(int e, float x) { v[e >> 2][e & 3] = x; }
    __device__ __forceinline__ void mma(const float (&a)[2], float b)
    {
        v[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b, v[0], 0, 0, 0);
        v[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b, v[1], 0, 0, 0);
    }
};

// bias + W . X over K inputs, KS = 64 / T per step, as one k-ordered fma chain per (row, stream) that starts from the bias.  w: the matrix
// (wave-uniform: a load takes it as its scalar base), wstep floats from step to step; woff[j]: the lane's weight of step 0 in row tile j, wlo[j]: the
// same in the step's first input (both inside the matrix: a row that does not exist is clamped to one that does, and its results are not used).
// xcol: the lane's column of X, xrow(s): the row of X the step's first input stands in (wave-uniform), xmax: the last row.  acc: the chain so far, or
// none (first): then bias[bidx[j]], the lane's rows', enter through the pipe as well -- from -0 everywhere, fma(bias, 1, -0) = bias in the first
// input's lanes and fma(-0, 1, bias) = bias in the others', bit for bit -- which takes them in A's layout, one load per lane and row tile.  Whole
// batches of U steps run with their weights loaded a batch ahead; the rest of the chain runs four steps at a time, and nothing is predicated there either:
// past K a load goes to a clamped address and B is zero, so the chain adds fma(w, 0, acc) = acc there
template <int T, int U, typename XR>
__device__ __forceinline__ DredFastAcc<T> dred_fast_chain(bool first, DredFastAcc<T> acc, const float *bias, const unsigned (&bidx)[DredFastAcc<T>::NJ], const float *w,
                                                          const unsigned (&woff)[DredFastAcc<T>::NJ], const unsigned (&wlo)[DredFastAcc<T>::NJ], int wstep, int K,
                                                          const float *xcol, int xmax, XR xrow)
{
    constexpr int KS = 64 / T, NJ = DredFastAcc<T>::NJ;
    const int kq = (threadIdx.x & 63) / T, ns = (K + KS - 1) / KS, whole = K / KS / U * U;      // (steps in whole batches: every input below K)
    const dred_gchar *wg = (const dred_gchar *)dred_fast_uniform(w);        // (global, not flat: the loads do not share a counter with the LDS reads)
    const float *xh = xcol + kq * T;
    float a[U][NJ], an[U][NJ];
    auto load = [&](float (&d)[U][NJ], int s0) {
        const dred_gchar *wp = wg + (size_t)s0 * wstep * 4;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            unsigned off = 4 * woff[j];     // (opaque: base + lane offset stays a scalar base and a 32-bit offset, not a hoisted 64-bit address per lane)
            asm volatile("" : "+v"(off));
#pragma unroll
            for (int u = 0; u < U; ++u) d[u][j] = *(const dred_gfloat *)(wp + (off + (unsigned)u * (unsigned)wstep * 4u));      // (one scalar base for the batch)
        }
    };
    if (whole) load(a, 0);
    if (first) {
        float b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = kq ? -0.f : *(const dred_gfloat *)((const dred_gchar *)dred_fast_uniform(bias) + 4 * bidx[j]);
#pragma unroll
        for (int e = 0; e < DredFastAcc<T>::NE; ++e) acc.set(e, -0.f);
        acc.mma(b, 1.f);
    }
    for (int s0 = 0; s0 < whole; s0 += U) {
        if (s0 + U < whole) load(an, s0 + U);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.mma(a[u], xh[xrow(s0 + u) * T]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) a[u][j] = an[u][j];
    }
    // (the rest in batches of four: sixteen clamped steps at once would hold sixteen scalar offsets and positions)
#pragma unroll 1
    for (int s0 = whole; s0 < ns; s0 += 4) {
        float ta[4][NJ], tb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = min(s0 + u, ns - 1);
            const bool ok = s0 + u < ns && KS * s + kq < K;
#pragma unroll
            for (int j = 0; j < NJ; ++j) ta[u][j] = *(const dred_gfloat *)(wg + ((unsigned)s * (unsigned)wstep * 4u + 4 * (ok ? woff[j] : wlo[j])));      // (the one scalar base)
            const float v = xcol[min(xrow(s) + kq, xmax) * T];
            tb[u] = ok ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc.mma(ta[u], tb[u]);
    }
    return acc;
}

// a dense matrix [K][stride] from row i0: rows below n_rows exist.  bias: [n_rows], the chain's start (then acc is not read); or none: acc goes on
template <int T, int U>
__device__ __forceinline__ DredFastAcc<T> dred_fast_dense(const float *bias, DredFastAcc<T> acc, const float *w, int stride, int i0, int n_rows, int K, const float *x)
{
    constexpr int KS = 64 / T, NJ = DredFastAcc<T>::NJ;
    int tk = threadIdx.x;                   // (opaque: the lane's offsets are formed per chain, not held in registers across the loops)
    asm volatile("" : "+v"(tk));
    const int lane = tk & 63, kq = lane / T;
    unsigned r[NJ], woff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { r[j] = min(i0 + T * j + lane % T, n_rows - 1); woff[j] = kq * stride + r[j]; }
    return dred_fast_chain<T, U>(bias != nullptr, acc, bias, r, w, woff, r, KS * stride, K, x + lane % T, K - 1, [](int s) { return KS * s; });
}

// the accumulator's element e of this lane: row (e & 3) + RUN (e >> 2) + row0 of the wave's 32, column lane % T.  dred_fast_row0: 4 (lane / T), opaque
// to the compiler at every use, so that a tile's addresses are formed where they are used -- hoisted out of the layer and latent loops, the
// addresses of every buffer would be held in registers all along
template <int T>
__device__ __forceinline__ int dred_fast_row0()
{
    int r = 4 * ((threadIdx.x & 63) / T);
    asm volatile("" : "+v"(r));
    return r;
}
template <int T>
__device__ __forceinline__ int dred_fast_row(int e, int row0) { return (e & 3) + DredFastAcc<T>::RUN * (e >> 2) + row0; }

// Workgroup w decodes streams [w T, w T + T) of the n active ones; arguments as dred_decode_kernel's, plus the GRUs' packed input matrices.
// U: steps whose weights are in flight per wave
template <int T, int U>
__global__ __launch_bounds__(DRED_FAST_THREADS) void dred_fast_kernel(const DredNet *P, const DredFastImage *img, int n, int max_latents, const int *rec,
                                                                       const float *state, const float *latents, float *features)
{
    static_assert(T == 32 || T == 16, "32 streams on the 32x32x2 MFMA, 16 on the 16x16x4");
    using Acc = DredFastAcc<T>;
    constexpr int KS = 64 / T, NJ = Acc::NJ, NE = Acc::NE;
    extern __shared__ float4 dred_fast_lds[];
    __shared__ int cnt[T];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, col = lane % T;
    const int latent_dim = P->latent_dim, state_dim = P->state_dim;
    float *const h0 = (float *)dred_fast_lds, *const h1 = h0 + T * dred_fast_pad(P->step[1].n_out), *const h2 = h1 + T * dred_fast_pad(P->step[3].n_out);
    float *const act = h2 + T * dred_fast_pad(P->step[5].n_out);
    const auto h = [&](int g) { return g == 0 ? h0 : g == 1 ? h1 : h2; };
    const int s0 = blockIdx.x * T;
    if (t < T) cnt[t] = s0 + t < n ? rec[(size_t)(s0 + t) * DRED_REC] : 0;
    __syncthreads();
    int maxc = 0;
    for (int a = 0; a < T; ++a) maxc = cnt[a] > maxc ? cnt[a] : maxc;
    if (maxc == 0) return;                  // (the whole workgroup)
    const int my_cnt = cnt[col];
    const bool layer_wave = wave < DRED_FAST_LAYER_WAVES;
    const int ft = wave - DRED_FAST_LAYER_WAVES;                       // dec_final's tile of a final wave
    const bool final_wave = ft >= 0 && ft < DRED_FAST_FINAL_WAVES;
    const int i0 = 32 * wave;

    for (int e = t; e < T * state_dim; e += DRED_FAST_THREADS) {
        const int j = e / T, a = e % T;
        act[e] = cnt[a] > 0 ? state[(size_t)(s0 + a) * state_dim + j] : 0.f;
    }
    __syncthreads();
    // latent l of every stream into the activation buffer, by the whole workgroup
    const auto load_latent = [&](int l) {
        int tl = t;                         // (opaque: the addresses of a latent's loads are formed per latent, not held in registers)
        asm volatile("" : "+v"(tl));
        for (int e = tl; e < T * latent_dim; e += DRED_FAST_THREADS) {
            const int j = e / T, a = e % T;
            act[e] = l < cnt[a] ? latents[((size_t)(s0 + a) * max_latents + l) * latent_dim + j] : 0.f;
        }
        __syncthreads();
    };
    // The two roles run the latent loop apart, so that neither holds the other's addresses in registers.  They meet at the same barriers, and the
    // counts on the two sides are kept equal by hand: ONE after the GRU states are written, then per latent ONE in load_latent, TWO per layer (16 in
    // all) and ONE at the latent's end.  A barrier added or dropped on one side alone hangs the workgroup.
    {
        // dred_rdovae_decode_qframe (src/dred_rdovae_dec.c:50-98): dense 1, GRU 2, dense 3, GRU 4, dense 5, GRU 6, dense 7, dense 8.  Step k of the layer
        // waves: compute layer k, barrier (every reader of what it overwrites is through), write, barrier.  The final waves meet the same barriers
        // and in step k advance dec_final over layer k - 1's output, which layer k only reads or leaves alone
        if (layer_wave) {
    // dred_rdovae_dec_init_states (src/dred_rdovae_dec.c:37-47): the GRU states
#pragma unroll 1
    for (int g = 0; g < 3; ++g) {
        const DredStep *q = &P->init[g];
        if (i0 < q->n_out) {
            Acc acc = dred_fast_dense<T, U>(q->b, Acc{}, q->w, q->n_out, i0, q->n_out, q->n_in, act);
#pragma unroll
            for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) h(g)[(i0 + dred_fast_row<T>(e, r0)) * T + col] = dred_fast_tanh(acc.get(e));
        }
    }
    __syncthreads();                        // (1) the GRU states are written
#pragma unroll 1
            for (int l = 0; l < maxc; ++l) {
            load_latent(l);                 // (1 barrier)
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                int tk = threadIdx.x;       // (opaque: what a layer derives from the lane is formed per layer, not held in registers across the loops)
                asm volatile("" : "+v"(tk));
                const int lane = tk & 63, col = lane % T, kq = lane / T;
                const DredStep *q = &P->step[k];
                const int g = k >> 1;       // the GRU of step 1, 3, 5; the state a dense layer 2, 4, 6 reads is GRU g - 1's
                const int n_out = q->n_out;
                float *out = q->gru ? h(g) : act;
                const float *x = k == 0 || q->gru || k == 7 ? act : h(g - 1);
                Acc res = {};
                const bool mine = i0 < n_out;
                if (mine && !q->gru) {
                    res = dred_fast_dense<T, U>(q->b, res, q->w, n_out, i0, n_out, q->n_in, x);
#pragma unroll
                    for (int e = 0; e < NE; ++e) res.set(e, dred_fast_tanh(res.get(e)));
                } else if (mine) {
                    // units i0 .. i0 + 31: gate by gate, the input part over the tile's union blocks, the recurrent part over the state
                    const int N = n_out;
                    const DredFastGru im = img->gru[g];
                    const int *start = im.start + 3 * wave;
                    float *hg = out;
                    Acc z = {}, r = {};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        asm volatile("" ::: "memory");      // (one chain at a time: two chains' loads in flight together cost their registers)
                        const int b0 = start[c], nb = start[c + 1] - b0;
                        const int *pos = dred_fast_uniform(im.pos + b0);
                        unsigned bidx[NJ], woff[NJ], wlo[NJ];
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int i = T * j + col;      // the lane's row of row tile j among the wave's 32
                            bidx[j] = min(i0 + i, N - 1); woff[j] = 32 * kq + i; wlo[j] = i;
                        }
                        const Acc in = dred_fast_chain<T, U>(true, Acc{}, q->b + c * N, bidx, im.w + (size_t)b0 * 128, woff, wlo, 32 * KS, 4 * nb, act + col, q->n_in - 1,
                                                             [&](int s) { return pos[(KS * s) >> 2] + ((KS * s) & 3); });
                        asm volatile("" ::: "memory");
                        const Acc rc = dred_fast_dense<T, U>(q->b + 3 * N + c * N, Acc{}, q->rec + c * N, 3 * N, i0, N, N, hg);
#pragma unroll
                        for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) {
                            if (c == 0) z.set(e, dred_fast_sigmoid(in.get(e) + rc.get(e)));
                            else if (c == 1) r.set(e, dred_fast_sigmoid(in.get(e) + rc.get(e)));
                            else {
                                const float old = hg[(i0 + dred_fast_row<T>(e, r0)) * T + col];
                                res.set(e, __builtin_fmaf(z.get(e), old, (1.f - z.get(e)) * dred_fast_tanh(__builtin_fmaf(rc.get(e), r.get(e), in.get(e)))));
                            }
                        }
                    }
                }
                __syncthreads();            // (2 k + 1) every reader of what layer k overwrites is through
                if (mine) {
#pragma unroll
                    for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) out[(i0 + dred_fast_row<T>(e, r0)) * T + col] = res.get(e);
                }
                __syncthreads();            // (2 k + 2) layer k's output is written
            }
            __syncthreads();                // (1) dec_final has read the last layer's output: the next latent may overwrite it
            }
        } else {
            __syncthreads();                // (1) the GRU states are written
#pragma unroll 1
            for (int l = 0; l < maxc; ++l) {
            load_latent(l);                 // (1 barrier)
            Acc facc = {};
            int off = 0;                    // of layer k among dec_final's inputs
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                __syncthreads();            // (2 k + 1)
                __syncthreads();            // (2 k + 2) layer k's output is written
                const DredStep *q = &P->step[k];
                if (final_wave) facc = dred_fast_dense<T, U>(k ? nullptr : P->final_b, facc, P->final_w + (size_t)off * LPCN_DRED_OUT, LPCN_DRED_OUT, 32 * ft, LPCN_DRED_OUT, q->n_out, q->gru ? h(k >> 1) : act);
                off += q->n_out;
            }
            if (final_wave && l < my_cnt) {
                // the lane's outputs are runs of four, and a run lies in one 20-float row: one address per run
                const int fcol = col;
                const int *q = rec + (size_t)(s0 + fcol) * DRED_REC;
                const int first = q[1], take = q[2], i00 = 32 * ft + dred_fast_row0<T>();
#pragma unroll
                for (int run = 0; run < NE / 4; ++run) {
                    const int i = i00 + Acc::RUN * run, r = LPCN_DRED_FRAMES * l + i / LPCN_NB_FEAT;
                    const bool ok = i < LPCN_DRED_OUT && (first < 0 || (r >= first && r < first + take));
                    const size_t row = first < 0 ? (size_t)(s0 + fcol) * LPCN_DRED_FRAMES * max_latents + r : (size_t)q[3] + (first + take - 1 - r);
                    if (ok) {
                        float *dst = features + row * LPCN_NB_FEAT + i % LPCN_NB_FEAT;
#pragma unroll
                        for (int e = 0; e < 4; ++e) dst[e] = facc.get(4 * run + e);
                    }
                }
            }
            __syncthreads();                // (1) the latent's end
            }
        }
    }
}

// ---- the decoder as a per-stream state in FAST arithmetic (dred_stream_kernel of dred_kernels.hip.h is the PARITY one): the tiles,
// the roles, the chains and the barrier discipline of dred_fast_kernel, with the three LDS state buffers filled from and drained to the streams'
// records.  Arguments as dred_stream_kernel's.  A record holds a layer's own width: the pad rows of a partial 32-row tile are zero on the way in and
// stay here on the way out.  What dred_fast_kernel leaves to chance -- a stream whose latents are through goes on advancing its column -- matters
// here: a GRU's new state is written for the columns whose own latents still run and for no other.
template <int T, int U>
__global__ __launch_bounds__(DRED_FAST_THREADS) void dred_stream_fast_kernel(const DredNet *P, const DredFastImage *img, int n, int max_latents, int init,
                                                                              const int *rec, int u_start, int u_count, const float *state,
                                                                              const float *latents, float *features, float *dstate, int rec_floats)
{
    static_assert(T == 32 || T == 16, "32 streams on the 32x32x2 MFMA, 16 on the 16x16x4");
    using Acc = DredFastAcc<T>;
    constexpr int KS = 64 / T, NJ = Acc::NJ, NE = Acc::NE;
    extern __shared__ float4 dred_fast_lds[];
    __shared__ int cnt[T], beg[T];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, col = lane % T;
    const int latent_dim = P->latent_dim, state_dim = P->state_dim;
    float *const h0 = (float *)dred_fast_lds, *const h1 = h0 + T * dred_fast_pad(P->step[1].n_out), *const h2 = h1 + T * dred_fast_pad(P->step[3].n_out);
    float *const act = h2 + T * dred_fast_pad(P->step[5].n_out);
    const auto h = [&](int g) { return g == 0 ? h0 : g == 1 ? h1 : h2; };
    const int s0 = blockIdx.x * T;
    if (t < T) {
        int c = 0, b = 0;
        if (s0 + t < n) {
            const int *q = rec ? rec + (size_t)(s0 + t) * DRED_SREC : nullptr;
            c = init ? (q ? q[0] != 0 : 1) : (q ? q[2] : u_count);
            b = q ? q[1] : u_start;
        }
        cnt[t] = c; beg[t] = b;
    }
    __syncthreads();
    int maxc = 0;
    for (int a = 0; a < T; ++a) maxc = cnt[a] > maxc ? cnt[a] : maxc;
    if (maxc == 0) return;                  // (the whole workgroup)
    const bool layer_wave = wave < DRED_FAST_LAYER_WAVES;
    const int ft = wave - DRED_FAST_LAYER_WAVES;                       // dec_final's tile of a final wave
    const bool final_wave = ft >= 0 && ft < DRED_FAST_FINAL_WAVES;
    const int i0 = 32 * wave;
    // the records of the streams that took part, from the state buffers: a layer's own rows
    const auto store_records = [&]() {
        for (int g = 0, at = 0; g < 3; ++g) {
            const int w = P->step[2 * g + 1].n_out;
            for (int e = t; e < T * w; e += DRED_FAST_THREADS) {
                const int j = e / T, a = e % T;
                if (cnt[a] > 0) dstate[(size_t)(s0 + a) * rec_floats + at + j] = h(g)[e];
            }
            at += w;
        }
    };

    if (init) {
        for (int e = t; e < T * state_dim; e += DRED_FAST_THREADS) {
            const int j = e / T, a = e % T;
            act[e] = cnt[a] > 0 ? state[(size_t)(s0 + a) * state_dim + j] : 0.f;
        }
        __syncthreads();
        // dred_rdovae_dec_init_states (src/dred_rdovae_dec.c:37-47): the GRU states
        if (layer_wave) {
#pragma unroll 1
            for (int g = 0; g < 3; ++g) {
                const DredStep *q = &P->init[g];
                if (i0 < q->n_out) {
                    Acc acc = dred_fast_dense<T, U>(q->b, Acc{}, q->w, q->n_out, i0, q->n_out, q->n_in, act);
#pragma unroll
                    for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) h(g)[(i0 + dred_fast_row<T>(e, r0)) * T + col] = dred_fast_tanh(acc.get(e));
                }
            }
        }
        __syncthreads();
        store_records();
        return;
    }
    for (int g = 0, at = 0; g < 3; ++g) {
        const int w = P->step[2 * g + 1].n_out;
        for (int e = t; e < T * dred_fast_pad(w); e += DRED_FAST_THREADS) {
            const int j = e / T, a = e % T;
            h(g)[e] = j < w && cnt[a] > 0 ? dstate[(size_t)(s0 + a) * rec_floats + at + j] : 0.f;
        }
        at += w;
    }
    __syncthreads();                        // the GRU states are in LDS
    // latent l of every stream's range into the activation buffer, by the whole workgroup
    const auto load_latent = [&](int l) {
        int tl = t;                         // (opaque: the addresses of a latent's loads are formed per latent, not held in registers)
        asm volatile("" : "+v"(tl));
        for (int e = tl; e < T * latent_dim; e += DRED_FAST_THREADS) {
            const int j = e / T, a = e % T;
            act[e] = l < cnt[a] ? latents[((size_t)(s0 + a) * max_latents + beg[a] + l) * latent_dim + j] : 0.f;
        }
        __syncthreads();
    };
    // The two roles run the latent loop apart, as in dred_fast_kernel, and meet at the same barriers: per latent ONE in load_latent, TWO per layer (16
    // in all) and ONE at the latent's end.  A barrier added or dropped on one side alone hangs the workgroup.
    if (layer_wave) {
#pragma unroll 1
        for (int l = 0; l < maxc; ++l) {
            load_latent(l);                 // (1 barrier)
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                int tk = threadIdx.x;       // (opaque: what a layer derives from the lane is formed per layer, not held in registers across the loops)
                asm volatile("" : "+v"(tk));
                const int lane = tk & 63, col = lane % T, kq = lane / T;
                const DredStep *q = &P->step[k];
                const int g = k >> 1;       // the GRU of step 1, 3, 5; the state a dense layer 2, 4, 6 reads is GRU g - 1's
                const int n_out = q->n_out;
                float *out = q->gru ? h(g) : act;
                const float *x = k == 0 || q->gru || k == 7 ? act : h(g - 1);
                Acc res = {};
                const bool mine = i0 < n_out;
                if (mine && !q->gru) {
                    res = dred_fast_dense<T, U>(q->b, res, q->w, n_out, i0, n_out, q->n_in, x);
#pragma unroll
                    for (int e = 0; e < NE; ++e) res.set(e, dred_fast_tanh(res.get(e)));
                } else if (mine) {
                    // units i0 .. i0 + 31: gate by gate, the input part over the tile's union blocks, the recurrent part over the state
                    const int N = n_out;
                    const DredFastGru im = img->gru[g];
                    const int *start = im.start + 3 * wave;
                    float *hg = out;
                    Acc z = {}, r = {};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        asm volatile("" ::: "memory");      // (one chain at a time: two chains' loads in flight together cost their registers)
                        const int b0 = start[c], nb = start[c + 1] - b0;
                        const int *pos = dred_fast_uniform(im.pos + b0);
                        unsigned bidx[NJ], woff[NJ], wlo[NJ];
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int i = T * j + col;      // the lane's row of row tile j among the wave's 32
                            bidx[j] = min(i0 + i, N - 1); woff[j] = 32 * kq + i; wlo[j] = i;
                        }
                        const Acc in = dred_fast_chain<T, U>(true, Acc{}, q->b + c * N, bidx, im.w + (size_t)b0 * 128, woff, wlo, 32 * KS, 4 * nb, act + col, q->n_in - 1,
                                                             [&](int s) { return pos[(KS * s) >> 2] + ((KS * s) & 3); });
                        asm volatile("" ::: "memory");
                        const Acc rc = dred_fast_dense<T, U>(q->b + 3 * N + c * N, Acc{}, q->rec + c * N, 3 * N, i0, N, N, hg);
#pragma unroll
                        for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) {
                            if (c == 0) z.set(e, dred_fast_sigmoid(in.get(e) + rc.get(e)));
                            else if (c == 1) r.set(e, dred_fast_sigmoid(in.get(e) + rc.get(e)));
                            else {
                                const float old = hg[(i0 + dred_fast_row<T>(e, r0)) * T + col];
                                res.set(e, __builtin_fmaf(z.get(e), old, (1.f - z.get(e)) * dred_fast_tanh(__builtin_fmaf(rc.get(e), r.get(e), in.get(e)))));
                            }
                        }
                    }
                }
                __syncthreads();            // (2 k + 1) every reader of what layer k overwrites is through
                if (mine && (!q->gru || l < cnt[col])) {      // (a stream whose own latents are through keeps its state)
#pragma unroll
                    for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) out[(i0 + dred_fast_row<T>(e, r0)) * T + col] = res.get(e);
                }
                __syncthreads();            // (2 k + 2) layer k's output is written
            }
            __syncthreads();                // (1) dec_final has read the last layer's output: the next latent may overwrite it
        }
    } else {
        const int my_cnt = cnt[col], my_beg = beg[col];
#pragma unroll 1
        for (int l = 0; l < maxc; ++l) {
            load_latent(l);                 // (1 barrier)
            Acc facc = {};
            int off = 0;                    // of layer k among dec_final's inputs
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                __syncthreads();            // (2 k + 1)
                __syncthreads();            // (2 k + 2) layer k's output is written
                const DredStep *q = &P->step[k];
                if (final_wave) facc = dred_fast_dense<T, U>(k ? nullptr : P->final_b, facc, P->final_w + (size_t)off * LPCN_DRED_OUT, LPCN_DRED_OUT, 32 * ft, LPCN_DRED_OUT, q->n_out, q->gru ? h(k >> 1) : act);
                off += q->n_out;
            }
            if (final_wave && l < my_cnt) {
                // the lane's outputs are runs of four, and a run lies in one 20-float row: one address per run
                int first = -1, take = 0, prow = 0;
                if (rec) { const int *q = rec + (size_t)(s0 + col) * DRED_SREC; first = q[3]; take = q[4]; prow = q[5]; }
                const int i00 = 32 * ft + dred_fast_row0<T>();
#pragma unroll
                for (int run = 0; run < NE / 4; ++run) {
                    const int i = i00 + Acc::RUN * run, r = LPCN_DRED_FRAMES * (my_beg + l) + i / LPCN_NB_FEAT;
                    const bool ok = i < LPCN_DRED_OUT && (first < 0 || (r >= first && r < first + take));
                    const size_t row = first < 0 ? (size_t)(s0 + col) * LPCN_DRED_FRAMES * max_latents + r : (size_t)prow + (first + take - 1 - r);
                    if (ok) {
                        float *dst = features + row * LPCN_NB_FEAT + i % LPCN_NB_FEAT;
#pragma unroll
                        for (int e = 0; e < 4; ++e) dst[e] = facc.get(4 * run + e);
                    }
                }
            }
            __syncthreads();                // (1) the latent's end
        }
    }
    store_records();                        // (behind the last latent's closing barrier)
}

}  // namespace lpcn
