// The layers the frame-rate float networks are built from -- the PLC predictor (plc_kernels.hip.h) and the DRED decoder (dred_kernels.hip.h) -- bit for
// bit like the reference's generic-C float build.  A workgroup of THREADS lanes carries S streams whose activations lie side by side in LDS, cell [j][S],
// so the S values of one input j are one broadcast read.  A lane owns an output row and A of the S streams: it loads each weight of the row once and
// applies it to A accumulators, one separately ordered add chain per stream.  The order of every sum is the reference's; products and sums are rounded
// separately (-ffp-contract=off).
#pragma once
#include "kernel_params.h"
#include "lpcnet_math.h"
#include "quant_i8.hip.h"

namespace lpcn {

// A consecutive floats of LDS, in the widest load their alignment allows (the cells of A streams start at a multiple of A)
template <int A>
__device__ __forceinline__ void lds_load(float (&v)[A], const float *p)
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

// The sum of _lpcnet_compute_dense (src/nnet.c:122-135): from the bias over the columns ascending, W [n_in][n_out].  x [n_in][S] in LDS.  Item = (row,
// group of A streams); store(row, a0, acc) takes an item's A sums, those of streams a0 .. a0 + A - 1: it applies the layer's activation and puts the results
// where the caller wants them.  No barrier.
template <int S, int A, int THREADS, int UNROLL, typename Store>
__device__ __forceinline__ void dense(const int n_in, const int n_out, const float *W, const float *B, const float *x, Store store)
{
    const int items = n_out * (S / A);
    for (int it = threadIdx.x; it < items; it += THREADS) {
        const int row = S == A ? it : it % n_out, a0 = S == A ? 0 : (it / n_out) * A;      // (one group: no division)
        float acc[A];
        const float b = B[row];
#pragma unroll
        for (int a = 0; a < A; ++a) acc[a] = b;
        const float *w = W + row;
        const float *xp = x + a0;
#pragma unroll UNROLL
        for (int j = 0; j < n_in; ++j) {
            const float wv = w[(size_t)j * n_out];
            float xv[A];
            lds_load<A>(xv, xp + j * S);
#pragma unroll
            for (int a = 0; a < A; ++a) acc[a] = acc[a] + wv * xv[a];
        }
        store(row, a0, acc);
    }
}

// The gate passes of compute_gruB (src/nnet.c:362-371) over the two parts' sums zrh / recur [3 n][S]: z and r by the table sigmoid, h by the table tanh
// of in + rec * r, the new state z * h_old + (1 - z) * h into hs (LIVE: for the streams with live[a] set only).  Ends with a barrier.
template <int S, int THREADS, bool LIVE>
__device__ __forceinline__ void gru_gates(const int N, float *hs, float *zrh, const float *recur, const float *tansig, const int *live)
{
    for (int i = threadIdx.x; i < 2 * N * S; i += THREADS) zrh[i] = lpcn_sigmoid(zrh[i] + recur[i], tansig);
    __syncthreads();
    // cell e = unit * S + stream: a lane reads and writes only its own cells of the state
    for (int e = threadIdx.x; e < N * S; e += THREADS) {
        float hh = zrh[2 * N * S + e] + recur[2 * N * S + e] * zrh[N * S + e];
        hh = lpcn_tanh(hh, tansig);
        const float z = zrh[e];
        const float hn = z * hs[e] + (1.f - z) * hh;
        if constexpr (LIVE) { if (live[e % S]) hs[e] = hn; }
        else hs[e] = hn;
    }
    __syncthreads();
}

// compute_gruB with a zero condition (src/nnet.c:326-372, float build: sparse_sgemv_accum8x4 src/vec.h:347-403, sgemv_accum src/nnet.c:73-86): bias + 0.f,
// the 8x4 blocks in list order, the recurrent sum ascending.  Lane = row, all S streams.  x [n_in][S] and hs [n][S] in LDS: the state, replaced in place
// (LIVE: for the streams with live[a] set only); zrh / recur [3 n][S] LDS scratch.
template <int S, int THREADS, bool LIVE>
__device__ __forceinline__ void gru_b(const GruLayer<float> &g, const float *x, float *hs, float *zrh, float *recur, const float *tansig, const int *live)
{
    const int N = g.n, rows = 3 * N;
    for (int row = threadIdx.x; row < rows; row += THREADS) {
        float z[S];
        const float b0 = g.bias[row] + 0.f;
#pragma unroll
        for (int a = 0; a < S; ++a) z[a] = b0;
        const int grp = row >> 3, r = row & 7;
        for (int blk = g.start[grp]; blk < g.start[grp + 1]; ++blk) {
            const float *w = g.w + (size_t)blk * 32 + r;
            const float *xp = x + g.pos[blk] * S;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float wv = w[8 * c];
                float xv[S];
                lds_load<S>(xv, xp + c * S);
#pragma unroll
                for (int a = 0; a < S; ++a) z[a] = z[a] + wv * xv[a];
            }
        }
#pragma unroll
        for (int a = 0; a < S; ++a) zrh[row * S + a] = z[a];
        float rc[S];
        const float b1 = g.bias[rows + row];
#pragma unroll
        for (int a = 0; a < S; ++a) rc[a] = b1;
        const float *R = g.rec + row;
#pragma unroll 4
        for (int j = 0; j < N; ++j) {
            const float wv = R[(size_t)j * rows];
            float hv[S];
            lds_load<S>(hv, hs + j * S);
#pragma unroll
            for (int a = 0; a < S; ++a) rc[a] = rc[a] + wv * hv[a];
        }
#pragma unroll
        for (int a = 0; a < S; ++a) recur[row * S + a] = rc[a];
    }
    __syncthreads();
    gru_gates<S, THREADS, LIVE>(N, hs, zrh, recur, tansig, live);
}

// A consecutive dwords of LDS: lds_load's widths for packed int8 cells
template <int A>
__device__ __forceinline__ void lds_load(int (&v)[A], const int *p)
{
    if constexpr (A == 8) {
        const int4 a = ((const int4 *)p)[0], b = ((const int4 *)p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if constexpr (A == 4) {
        const int4 a = *(const int4 *)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (A == 2) {
        const int2 a = *(const int2 *)p;
        v[0] = a.x; v[1] = a.y;
    } else {
        v[0] = p[0];
    }
}

// n floats per stream, cell [j][S], to packed int8, four per dword, cell [j / 4][S]: (signed char)(int)floor(.5 + 127 x) (quant_s8).  n a multiple of 4.
// No barrier.
template <int S, int THREADS>
__device__ __forceinline__ void quant_cells(const int n, const float *x, int *q)
{
    for (int e = threadIdx.x; e < (n >> 2) * S; e += THREADS) {
        const float *p = x + (e / S) * 4 * S + e % S;
        q[e] = quant_s8(p[0]) | quant_s8(p[S]) << 8 | quant_s8(p[2 * S]) << 16 | quant_s8(p[3 * S]) << 24;
    }
}

// compute_gruB of the reference's generic-C int8 (DOT_PROD) build (src/nnet.c:326-372 over sparse_sgemv_accum8x4 / sgemv_accum8x4, src/vec.h:274-339,
// USE_SU_BIAS undefined): per row out = bias (+ 0.f: the input part's zero condition), out *= 128*127, per 8x4 block -- the input part's in list
// order, the recurrent part's N / 4 column blocks ascending -- the exact integer sum of four int8 products added with one rounded float add, then
// out *= 1/128/127.  The layer's input and the old state are quantised once, at the start of the call, into xq [n_in / 4][S] and sq [n / 4][S] (LDS,
// packed int8).  Lane = row, all S streams: a weight dword is loaded once and applied to the S dwords of its block, one broadcast read.  The gate
// passes, the scratch and `live` are gru_b's.
template <int S, int THREADS, bool LIVE>
__device__ __forceinline__ void gru_b_i8(const GruLayer<int> &g, const float *x, float *hs, float *zrh, float *recur, int *xq, int *sq, const float *tansig,
                                         const int *live)
{
    const int N = g.n, rows = 3 * N, nblk = N >> 2;
    quant_cells<S, THREADS>(g.n_in, x, xq);
    quant_cells<S, THREADS>(N, hs, sq);
    __syncthreads();
    for (int row = threadIdx.x; row < rows; row += THREADS) {
        float z[S];
        float b0 = g.bias[row] + 0.f;
        b0 = b0 * QS;
#pragma unroll
        for (int a = 0; a < S; ++a) z[a] = b0;
        const int grp = row >> 3, r = row & 7;
#pragma unroll 2
        for (int blk = g.start[grp]; blk < g.start[grp + 1]; ++blk) {
            const int wv = g.w[(size_t)blk * 8 + r];
            int xv[S];
            lds_load<S>(xv, xq + g.pos[blk] * S);
#pragma unroll
            for (int a = 0; a < S; ++a) z[a] = z[a] + (float)__builtin_amdgcn_sdot4(wv, xv[a], 0, false);
        }
#pragma unroll
        for (int a = 0; a < S; ++a) zrh[row * S + a] = z[a] * QS1;
        float rc[S];
        const float b1 = g.bias[rows + row] * QS;
#pragma unroll
        for (int a = 0; a < S; ++a) rc[a] = b1;
        const int *R = g.rec + row;
#pragma unroll 4
        for (int j = 0; j < nblk; ++j) {
            const int wv = R[(size_t)j * rows];
            int hv[S];
            lds_load<S>(hv, sq + j * S);
#pragma unroll
            for (int a = 0; a < S; ++a) rc[a] = rc[a] + (float)__builtin_amdgcn_sdot4(wv, hv[a], 0, false);
        }
#pragma unroll
        for (int a = 0; a < S; ++a) recur[row * S + a] = rc[a] * QS1;
    }
    __syncthreads();
    gru_gates<S, THREADS, LIVE>(N, hs, zrh, recur, tansig, live);
}

}  // namespace lpcn
