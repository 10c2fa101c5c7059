// Packet-loss concealment on the device: the data side of lpcnet_plc_update / lpcnet_plc_conceal in causal mode
// (src/lpcnet_plc.c:188-340) for every stream of a batch, bit for bit like the reference's generic-C build of the blob's flavour (float, or
// int8 DOT_PROD: only the PLC network's two GRUs differ, plc_pred_i8_kernel).  The control side
// -- which branch a stream takes in this step -- is a function of the loss flags and the FEC calls alone and lives on the host
// (plc_plan.cpp: plc_plan); each kernel here works on the streams the host listed for it:
//   plc_burg_kernel   DC removal (src/lpcnet_plc.c:196-205) and burg_cepstral_analysis (src/freq.c:156-199) of a received frame
//   plc_pred_kernel   compute_plc_pred (src/lpcnet_plc.c:135-146) with its input selection (get_fec_or_pred :148-168), the rotation and
//                     restoring of plc_copy (:215, :238, :305-306) and the attenuation of features[0] (:323-324)
//   plc_pred_i8_kernel  the same with the int8 GRUs of the DOT_PROD build (src/vec.h:274-339), for int8 blobs: one body (plc_pred_body), two flavours
//   plc_pred_s_kernel<S>, plc_pred_s_int8_kernel<S>  either flavour at S = 2, 4 or 8 records per workgroup, bit for bit like the two above
//   plc_mix_kernel    the PCM queue, the deferred feature queue, the cross-fade, lpcnet_reset_signal, DC restore
//   group_gather_kernel, group_scatter_kernel   everything a compacted group of streams takes in and gives back, in one launch each: the group
//                     runs through the ordinary frame and sample kernels
// Every sum keeps the reference's order; products and sums are rounded separately (-ffp-contract=off).
#pragma once
#include "spectral.hip.h"
#include "lpcnet_log10.h"
#include "frame_nets.hip.h"         // dense, gru_b: the float layers, shared with the DRED decoder
#include "quant_i8.hip.h"           // quant_s8, QS, QS1: the int8 arithmetic's quantisation and scales
#include "lpcnet_plc_tables_gen.h"
#include "plc_burg.h"
#include "plc_records.h"      // record sizes, flags and operation codes of the control lists (shared with the host planner)
#include <type_traits>

namespace lpcn {

constexpr int PLC_BURG_THREADS = 128;
constexpr int PLC_PRED_THREADS = 256;
constexpr int PLC_MIX_THREADS = 512;
#define LPCN_PLC_DC_CONST 0.003      // src/lpcnet_plc.c:183

// One workgroup per listed stream, wave h on half frame h.  pcm [n][160] is the call's frame: with the DC filter it is rewritten in place.
__global__ __launch_bounds__(PLC_BURG_THREADS) void plc_burg_kernel(LpcnFrameModel M, const int *map, int cnt, short *pcm, PlcData D, int remove_dc)
{
    __shared__ float xin[2][80];
    __shared__ double cauto[2][LPCN_BURG_ORDER + 1];
    __shared__ double work[2][LPCN_BURG_WORK];
    __shared__ float acoef[2][LPCN_BURG_ORDER];
    __shared__ float gres[2];
    __shared__ cpx fbuf[2][320];
    __shared__ float exb[2][LPCN_NB_BANDS], lyb[2][LPCN_NB_BANDS], cepb[2][LPCN_NB_BANDS];
    if ((int)blockIdx.x >= cnt) return;
    const int s = map[blockIdx.x];
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    short *p = pcm + (size_t)s * LPCN_FRAME_SIZE;
    if (remove_dc) {
        // src/lpcnet_plc.c:196-205: serial in double
        if (threadIdx.x == 0) {
            double dc_mem = D.dc[2 * s], syn_dc = D.dc[2 * s + 1];
            dc_mem += syn_dc;
            D.delta[s] = (int)syn_dc;
            short *lp = D.lp + (size_t)s * LPCN_FRAME_SIZE;
            for (int i = 0; i < LPCN_FRAME_SIZE; ++i) {
                const short l = (short)(int)floor(.5 + dc_mem);
                dc_mem += LPCN_PLC_DC_CONST * ((double)p[i] - dc_mem);
                lp[i] = l;
                p[i] = (short)((int)p[i] - (int)l);
            }
            D.dc[2 * s] = dc_mem;
            D.dc[2 * s + 1] = 0.0;
        }
        __syncthreads();
    }
    // compute_burg_cepstrum (src/freq.c:156-188) on half h
    const short *ph = p + h * 80;
    for (int i = lane; i < LPCN_BURG_LEN; i += 64) xin[h][i] = (float)ph[i + 1] - 0.85f * (float)ph[i];
    __syncthreads();
    if (lane <= LPCN_BURG_ORDER) cauto[h][lane] = lpcn_burg_inner(xin[h], xin[h] + lane, LPCN_BURG_LEN - lane);
    __syncthreads();
    if (lane == 0) {
        const float g = lpcn_burg_recursion(acoef[h], xin[h], cauto[h], work[h]);
        gres[h] = g / 50.f;                          // g /= len - 2*(order-1)
    }
    __syncthreads();
    cpx *F = fbuf[h];
    for (int k = lane; k < 320; k += 64) {
        float v = 0.f;
        if (k == 0) v = 1.f;
        else if (k <= LPCN_BURG_ORDER) v = (float)((double)(-acoef[h][k - 1]) * lpcn_plc_pow995[k - 1]);
        cpx z; z.r = 0.0031250000f * v; z.i = 0.0031250000f * 0.f;
        F[M.tab_bitrev[k]] = z;
    }
    __syncthreads();
    fft320_passes(F, (const cpx *)M.tab_tw, lane);
    // compute_band_energy_inverse (src/freq.c:60-84), scaling and log10 (:177-179)
    if (lane < LPCN_NB_BANDS) {
        float sum = 0.f;
        if (lane > 0) {
            const int lo = lpcn_eband5ms[lane - 1] * 4, size = (lpcn_eband5ms[lane] - lpcn_eband5ms[lane - 1]) * 4;
            for (int j = 0; j < size; ++j) {
                const float frac = (float)j / (float)size;
                const cpx X = F[lo + j];
                float tmp = X.r * X.r;
                tmp = tmp + X.i * X.i;
                tmp = (float)(1.0 / ((double)tmp + 1e-9));
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
                tmp = (float)(1.0 / ((double)tmp + 1e-9));
                sum = sum + (1.f - frac) * tmp;
            }
        }
        if (lane == 0 || lane == LPCN_NB_BANDS - 1) sum = sum * 2.f;
        const float inv_w3 = 1.f / ((320.f * 320.f) * 320.f);
        sum = (float)((double)sum * ((.45 * (double)gres[h]) * (double)inv_w3));
        lyb[h][lane] = lpcn_log10f_of_double(1e-2 + (double)sum);
    }
    __syncthreads();
    if (lane == 0) {
        float logMax = -2.f, follow = -2.f;
        for (int i = 0; i < LPCN_NB_BANDS; ++i) {
            float v = lyb[h][i];
            const float f25 = follow - 2.5f, m8 = logMax - 8.f;
            const float inner = LPCN_MAX16(f25, v);
            v = LPCN_MAX16(m8, inner);
            logMax = LPCN_MAX16(logMax, v);
            follow = LPCN_MAX16(f25, v);
            exb[h][i] = v;
        }
    }
    __syncthreads();
    if (lane < LPCN_NB_BANDS) {
        float sum = 0.f;
        for (int j = 0; j < LPCN_NB_BANDS; ++j) sum = sum + exb[h][j] * M.tab_idct[j * LPCN_NB_BANDS + lane];
        float c = (float)((double)sum * sqrt(2. / LPCN_NB_BANDS));
        if (lane == 0) c = c - 4.f;
        cepb[h][lane] = c;
    }
    __syncthreads();
    // burg_cepstral_analysis (src/freq.c:190-199): mean and difference of the halves
    if (h == 0 && lane < LPCN_NB_BANDS) {
        const float c0 = cepb[0][lane], c1 = cepb[1][lane];
        float *o = D.burg + (size_t)s * 2 * LPCN_NB_BANDS;
        o[lane] = (float)(.5 * (double)(c0 + c1));
        o[LPCN_NB_BANDS + lane] = c0 - c1;
    }
}

// ---- the int8 (DOT_PROD) PLC network: compute_plc_pred of the reference's generic-C int8 build.  The dense layers are float there too; the GRUs
// run sparse_sgemv_accum8x4 / sgemv_accum8x4 of src/vec.h:274-339 (USE_SU_BIAS undefined: they start from `bias`): per row out *= 128*127, then for
// each 8x4 block in list order the exact integer sum of four int8 products is added with ONE rounded float add, then out *= 1/128/127.  The inputs
// of a product are quantised once, (signed char)(int)floor(.5 + 127 x) (quant_s8, quant_i8.hip.h).
constexpr int PLC_Q_UNITS_PER_LANE = (LPCN_PLC_MAX_UNITS + PLC_PRED_THREADS - 1) / PLC_PRED_THREADS;

// compute_gruB on quantised inputs.  One lane per UNIT: it runs the unit's three gate rows (z, r, h: rows i, N + i, 2 N + i), so no pre-activation
// leaves the lane -- the input product row after row (each row group has its own block list), the recurrent product as three independent add chains
// on one LDS dword per block.  Units beyond the workgroup size take a second pass (t = 1).  xq [M / 4] and sq [N / 4]: the input and the old state as packed int8, four per dword; hs [N] the
// state (replaced); nq (may be null) receives the new state quantised, the next layer's input.  All in LDS.
__device__ __forceinline__ void plc_gru_i8(const GruLayer<int> &g, const int *xq, const int *sq, float *hs, unsigned char *nq, const float *tansig)
{
    const int N = g.n, rows = 3 * N, nblk = N >> 2;
    float hn[PLC_Q_UNITS_PER_LANE];
#pragma unroll
    for (int t = 0; t < PLC_Q_UNITS_PER_LANE; ++t) {
        const int i = threadIdx.x + t * PLC_PRED_THREADS;
        hn[t] = 0.f;
        if (i < N) {
            float zrh[3], rc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int row = k * N + i, grp = row >> 3, r = row & 7;
                float a = g.bias[row] + 0.f;
                a = a * QS;
                for (int blk = g.start[grp]; blk < g.start[grp + 1]; ++blk)
                    a = a + (float)__builtin_amdgcn_sdot4(g.w[(size_t)blk * 8 + r], xq[g.pos[blk]], 0, false);
                zrh[k] = a * QS1;
                rc[k] = g.bias[rows + row] * QS;
            }
            for (int j = 0; j < nblk; ++j) {
                const int x = sq[j];
                const int *w = g.rec + (size_t)j * rows + i;
                rc[0] = rc[0] + (float)__builtin_amdgcn_sdot4(w[0], x, 0, false);
                rc[1] = rc[1] + (float)__builtin_amdgcn_sdot4(w[N], x, 0, false);
                rc[2] = rc[2] + (float)__builtin_amdgcn_sdot4(w[2 * N], x, 0, false);
            }
            const float z = lpcn_sigmoid(zrh[0] + rc[0] * QS1, tansig);
            const float rg = lpcn_sigmoid(zrh[1] + rc[1] * QS1, tansig);
            float hh = zrh[2] + (rc[2] * QS1) * rg;
            hh = lpcn_tanh(hh, tansig);
            hn[t] = z * hs[i] + (1.f - z) * hh;
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PLC_Q_UNITS_PER_LANE; ++t) {
        const int i = threadIdx.x + t * PLC_PRED_THREADS;
        if (i < N) {
            hs[i] = hn[t];
            if (nq) nq[i] = (unsigned char)quant_s8(hn[t]);
        }
    }
    __syncthreads();
}

// What the two flavours of the predictor do differently: the LDS block (the 57 inputs, both GRU states as floats and the 20 outputs in either; then
// whatever the GRUs read and scratch), how a restored state value and a dense1 output are staged for the GRUs, and the two GRU calls.
struct PlcFloat {
    using Net = PlcNet;
    struct alignas(16) Lds {
        float in[LPCN_PLC_IN + 3];
        float d1[LPCN_PLC_MAX_UNITS], h1[LPCN_PLC_MAX_UNITS], h2[LPCN_PLC_MAX_UNITS];
        float zrh[3 * LPCN_PLC_MAX_UNITS], recur[3 * LPCN_PLC_MAX_UNITS];
        float out[LPCN_NB_FEAT];
    };
    static __device__ __forceinline__ void stage_state(Lds &, int, int, float) {}      // (the float state is all the GRUs read)
    static __device__ __forceinline__ void stage_dense1(Lds &L, int i, float v) { L.d1[i] = v; }
    static __device__ __forceinline__ void grus(const Net &P, Lds &L)
    {
        gru_b<1, PLC_PRED_THREADS, false>(P.gru[0], L.d1, L.h1, L.zrh, L.recur, P.tansig, nullptr);
        gru_b<1, PLC_PRED_THREADS, false>(P.gru[1], L.h1, L.h2, L.zrh, L.recur, P.tansig, nullptr);
    }
};
struct PlcInt8 {
    using Net = PlcNetQ;
    struct alignas(16) Lds {
        float h1[LPCN_PLC_MAX_UNITS], h2[LPCN_PLC_MAX_UNITS];
        int xq[LPCN_PLC_MAX_UNITS / 4], sq[2][LPCN_PLC_MAX_UNITS / 4];      // a layer's input, the two old states: packed int8
        float in[LPCN_PLC_IN + 3];
        float out[LPCN_NB_FEAT];
    };
    static __device__ __forceinline__ void stage_state(Lds &L, int layer, int i, float v) { ((unsigned char *)L.sq[layer])[i] = (unsigned char)quant_s8(v); }
    static __device__ __forceinline__ void stage_dense1(Lds &L, int i, float v) { ((unsigned char *)L.xq)[i] = (unsigned char)quant_s8(v); }      // (read as GRU 1's quantised input only)
    static __device__ __forceinline__ void grus(const Net &P, Lds &L)
    {
        plc_gru_i8(P.gru[0], L.xq, L.sq[0], L.h1, (unsigned char *)L.xq, P.tansig);
        plc_gru_i8(P.gru[1], L.xq, L.sq[1], L.h2, nullptr, P.tansig);
    }
};

// One workgroup per record.  flags: PLC_F_ROT rotate plc_copy and store plc_net in plc_copy[0]; restore k (1, 2): plc_net = plc_copy[k];
// PLC_F_COMPUTE run the network on the selected input; PLC_F_KEEP features = its output (FEC input: features = the FEC vector, the
// output is discarded); PLC_F_ATT features[0] = MAX16(-10, features[0] + a1 - a2).  PLC_F_RAW (the parity seam): the input is
// [burg36, an20, a1] as given and the output goes to raw_out [n][20].  The records, flags and per-stream data are the same for both flavours (the
// network state is float in both builds), and so is everything here but the GRUs.
template <typename F>
__device__ __forceinline__ void plc_pred_body(const typename F::Net &P, const int *ctl, int cnt, const PlcData &D, float *raw_out)
{
    __shared__ typename F::Lds L;
    if ((int)blockIdx.x >= cnt) return;
    const int *rec = ctl + (size_t)blockIdx.x * PLC_PRED_REC;
    const int s = rec[0], flags = rec[1], fec_row = rec[2];
    const float a1 = __int_as_float(rec[3]), a2 = __int_as_float(rec[4]);
    const int g1 = P.gru[0].n, g2 = P.gru[1].n, G = g1 + g2;
    float *net = D.net + (size_t)s * 4 * G;
    const int restore = (flags >> PLC_F_RESTORE_SHIFT) & 3, input = (flags >> PLC_F_INPUT_SHIFT) & 3;
    for (int t = threadIdx.x; t < G; t += blockDim.x) {
        float v0 = net[t];
        if (flags & PLC_F_ROT) {
            const float v1 = net[G + t], v2 = net[2 * G + t];
            net[G + t] = v0; net[2 * G + t] = v1; net[3 * G + t] = v2;
        }
        if (restore) { v0 = net[(restore + 1) * G + t]; net[t] = v0; }
        if (t < g1) { L.h1[t] = v0; F::stage_state(L, 0, t, v0); }
        else { L.h2[t - g1] = v0; F::stage_state(L, 1, t - g1, v0); }
    }
    if (!(flags & PLC_F_COMPUTE)) return;
    float *feat = D.feat + (size_t)s * LPCN_NB_FEAT;
    const float *fec = D.fec + ((size_t)s * LPCN_PLC_MAX_FEC + fec_row) * LPCN_NB_FEAT;
    if (threadIdx.x < LPCN_PLC_IN) {
        const int j = threadIdx.x;
        float v = 0.f;
        if (input >= PLC_IN_BURG && j < 2 * LPCN_NB_BANDS) v = D.burg[(size_t)s * 2 * LPCN_NB_BANDS + j];
        if (j >= 2 * LPCN_NB_BANDS && j < LPCN_PLC_IN - 1) {
            if (input == PLC_IN_FEC) v = fec[j - 2 * LPCN_NB_BANDS];
            if (input == PLC_IN_BURG_FEAT) v = D.an[(size_t)s * LPCN_AN_NB_FEATURES + j - 2 * LPCN_NB_BANDS];
        }
        if (j == LPCN_PLC_IN - 1) v = input == PLC_IN_FEC ? -1.f : input == PLC_IN_ZEROS ? 0.f : 1.f;
        if (flags & PLC_F_RAW) v = j < 2 * LPCN_NB_BANDS ? D.burg[(size_t)s * 2 * LPCN_NB_BANDS + j] : j < LPCN_PLC_IN - 1 ? D.an[(size_t)s * LPCN_AN_NB_FEATURES + j - 2 * LPCN_NB_BANDS] : a1;
        L.in[j] = v;
    }
    __syncthreads();
    // (dense1's 57 columns by three, 19 rounds and no remainder loop: by four, or rolled, the int8 step measures slower -- EXPERIMENTS.md)
    dense<1, 1, PLC_PRED_THREADS, 3>(LPCN_PLC_IN, P.d1, P.dense1_w, P.dense1_b, L.in, [&](int i, int, const float (&acc)[1]) { F::stage_dense1(L, i, lpcn_tanh(acc[0], P.tansig)); });
    __syncthreads();
    F::grus(P, L);
    dense<1, 1, PLC_PRED_THREADS, 4>(g2, LPCN_NB_FEAT, P.out_w, P.out_b, L.h2, [&](int i, int, const float (&sum)[1]) {
        float acc = sum[0];
        if (i == LPCN_NB_FEAT - 1) { const float v = acc + .1f; acc = .5f < v ? .5f : v; }      // MIN16(.5f, out[19]+.1f)
        L.out[i] = acc;
    });
    for (int t = threadIdx.x; t < G; t += blockDim.x) net[t] = t < g1 ? L.h1[t] : L.h2[t - g1];
    __syncthreads();
    if (threadIdx.x < LPCN_NB_FEAT) {
        const int i = threadIdx.x;
        float v = 0.f;
        bool write = false;
        if (input == PLC_IN_FEC) { v = fec[i]; write = true; }
        else if (flags & PLC_F_KEEP) { v = L.out[i]; write = true; }
        if (write && i == 0 && (flags & PLC_F_ATT)) {
            v = v + a1;
            v = v - a2;
            v = -10.f > v ? -10.f : v;
        }
        if (write) feat[i] = v;
        if ((flags & PLC_F_RAW) && raw_out) raw_out[(size_t)s * LPCN_NB_FEAT + i] = L.out[i];
    }
}

// the float network: both GRUs are gru_b (frame_nets.hip.h) ...
__global__ __launch_bounds__(PLC_PRED_THREADS) void plc_pred_kernel(PlcNet P, const int *ctl, int cnt, PlcData D, float *raw_out)
{
    plc_pred_body<PlcFloat>(P, ctl, cnt, D, raw_out);
}
// ... and an int8 blob's: plc_gru_i8
__global__ __launch_bounds__(PLC_PRED_THREADS) void plc_pred_i8_kernel(PlcNetQ P, const int *ctl, int cnt, PlcData D, float *raw_out)
{
    plc_pred_body<PlcInt8>(P, ctl, cnt, D, raw_out);
}

// ---- S = 2, 4 or 8 records per workgroup: workgroup w takes the records [w S, min(cnt, w S + S)), so a weight read through L2 serves S streams.  The same
// records, flags and arithmetic as plc_pred_body, stream by stream: each of the S streams keeps its own flags, so the rotation, the restore, the input
// selection and what becomes of the output are decided per stream; a stream without PLC_F_COMPUTE -- or a slot past the last record -- is not live in
// the layers, which leave its state alone (gru_b's LIVE mask), and has zeros where the layers read.  The activations lie [j][S] in dynamic LDS
// (plc_records.h: plc_pred_lds_bytes, sized by the blob's widths), so the S values of an input are one broadcast read of 4 S bytes that every lane of
// the wave makes at the same address: no bank conflict at any S.  The GRUs are the shared S-stream layers (frame_nets.hip.h): lane = gate row, all S
// streams; dense1 gives a lane S / 2 streams, so 128 rows fill the 256 lanes at every S, the output layer one (row, stream).
template <int S, typename W>
__device__ __forceinline__ void plc_pred_s_body(const PlcNetT<W> &P, const int *ctl, int cnt, const PlcData &D, float *raw_out)
{
    extern __shared__ float4 plc_pred_lds[];
    constexpr bool Q = !std::is_same<W, float>::value;
    constexpr int AD = S / 2;
    const int d1 = P.d1, g1 = P.gru[0].n, g2 = P.gru[1].n, G = g1 + g2, mg = plc_pred_max(g1, g2);
    float *in = (float *)plc_pred_lds;
    float *x1 = in + S * PLC_PRED_IN_PAD;
    float *h1 = x1 + S * d1, *h2 = h1 + S * g1;
    float *zrh = h2 + S * g2, *recur = zrh + S * 3 * mg;
    float *out = recur + S * 3 * mg;
    int *xq = (int *)(out + S * LPCN_NB_FEAT), *sq = xq + S * (plc_pred_max(d1, g1) >> 2);      // (an int8 blob's cells; else none)
    int *rec = Q ? sq + S * (mg >> 2) : xq;                                                       // [S][PLC_PRED_REC]: stream (-1: no record), flags, ...
    int *live = rec + S * PLC_PRED_REC;
    const int r0 = blockIdx.x * S, t = threadIdx.x;
    if (r0 >= cnt) return;
    if (t < S * PLC_PRED_REC) {
        const bool have = r0 + t / PLC_PRED_REC < cnt;
        rec[t] = have ? ctl[(size_t)r0 * PLC_PRED_REC + t] : t % PLC_PRED_REC == 0 ? -1 : 0;
    }
    __syncthreads();
    if (t < S) live[t] = rec[t * PLC_PRED_REC] >= 0 && (rec[t * PLC_PRED_REC + 1] & PLC_F_COMPUTE) ? 1 : 0;
    bool any = false;
#pragma unroll
    for (int a = 0; a < S; ++a) {
        const int s = rec[a * PLC_PRED_REC], flags = rec[a * PLC_PRED_REC + 1];
        const bool lv = s >= 0 && (flags & PLC_F_COMPUTE);
        any |= lv;
        float *net = D.net + (size_t)(s < 0 ? 0 : s) * 4 * G;
        const int restore = (flags >> PLC_F_RESTORE_SHIFT) & 3;
        for (int k = t; k < G; k += PLC_PRED_THREADS) {
            float v0 = 0.f;
            if (s >= 0) {
                v0 = net[k];
                if (flags & PLC_F_ROT) {
                    const float v1 = net[G + k], v2 = net[2 * G + k];
                    net[G + k] = v0; net[2 * G + k] = v1; net[3 * G + k] = v2;
                }
                if (restore) { v0 = net[(restore + 1) * G + k]; net[k] = v0; }
            }
            if (!lv) v0 = 0.f;
            if (k < g1) h1[k * S + a] = v0;
            else h2[(k - g1) * S + a] = v0;
        }
    }
    if (!any) return;                       // (the whole workgroup)
    for (int e = t; e < LPCN_PLC_IN * S; e += PLC_PRED_THREADS) {
        const int j = e / S, a = e % S;
        const int s = rec[a * PLC_PRED_REC], flags = rec[a * PLC_PRED_REC + 1];
        const int input = (flags >> PLC_F_INPUT_SHIFT) & 3;
        float v = 0.f;
        if (s >= 0 && (flags & PLC_F_COMPUTE)) {
            const float *fec = D.fec + ((size_t)s * LPCN_PLC_MAX_FEC + rec[a * PLC_PRED_REC + 2]) * LPCN_NB_FEAT;
            if (input >= PLC_IN_BURG && j < 2 * LPCN_NB_BANDS) v = D.burg[(size_t)s * 2 * LPCN_NB_BANDS + j];
            if (j >= 2 * LPCN_NB_BANDS && j < LPCN_PLC_IN - 1) {
                if (input == PLC_IN_FEC) v = fec[j - 2 * LPCN_NB_BANDS];
                if (input == PLC_IN_BURG_FEAT) v = D.an[(size_t)s * LPCN_AN_NB_FEATURES + j - 2 * LPCN_NB_BANDS];
            }
            if (j == LPCN_PLC_IN - 1) v = input == PLC_IN_FEC ? -1.f : input == PLC_IN_ZEROS ? 0.f : 1.f;
            if (flags & PLC_F_RAW) v = j < 2 * LPCN_NB_BANDS ? D.burg[(size_t)s * 2 * LPCN_NB_BANDS + j] : j < LPCN_PLC_IN - 1 ? D.an[(size_t)s * LPCN_AN_NB_FEATURES + j - 2 * LPCN_NB_BANDS] : __int_as_float(rec[a * PLC_PRED_REC + 3]);
        }
        in[e] = v;
    }
    __syncthreads();
    dense<S, AD, PLC_PRED_THREADS, 3>(LPCN_PLC_IN, d1, P.dense1_w, P.dense1_b, in, [&](int i, int a0, const float (&acc)[AD]) {
#pragma unroll
        for (int a = 0; a < AD; ++a) x1[i * S + a0 + a] = lpcn_tanh(acc[a], P.tansig);
    });
    __syncthreads();
    if constexpr (Q) {
        gru_b_i8<S, PLC_PRED_THREADS, true>(P.gru[0], x1, h1, zrh, recur, xq, sq, P.tansig, live);
        gru_b_i8<S, PLC_PRED_THREADS, true>(P.gru[1], h1, h2, zrh, recur, xq, sq, P.tansig, live);
    } else {
        gru_b<S, PLC_PRED_THREADS, true>(P.gru[0], x1, h1, zrh, recur, P.tansig, live);
        gru_b<S, PLC_PRED_THREADS, true>(P.gru[1], h1, h2, zrh, recur, P.tansig, live);
    }
    dense<S, 1, PLC_PRED_THREADS, 4>(g2, LPCN_NB_FEAT, P.out_w, P.out_b, h2, [&](int i, int a, const float (&sum)[1]) {
        float acc = sum[0];
        if (i == LPCN_NB_FEAT - 1) { const float v = acc + .1f; acc = .5f < v ? .5f : v; }      // MIN16(.5f, out[19]+.1f)
        out[i * S + a] = acc;
    });
#pragma unroll
    for (int a = 0; a < S; ++a) {
        if (!live[a]) continue;
        float *net = D.net + (size_t)rec[a * PLC_PRED_REC] * 4 * G;
        for (int k = t; k < G; k += PLC_PRED_THREADS) net[k] = k < g1 ? h1[k * S + a] : h2[(k - g1) * S + a];
    }
    __syncthreads();
    if (t < LPCN_NB_FEAT * S) {
        const int i = t / S, a = t % S;
        if (live[a]) {
            const int s = rec[a * PLC_PRED_REC], flags = rec[a * PLC_PRED_REC + 1];
            const int input = (flags >> PLC_F_INPUT_SHIFT) & 3;
            float v = 0.f;
            bool write = false;
            if (input == PLC_IN_FEC) { v = D.fec[((size_t)s * LPCN_PLC_MAX_FEC + rec[a * PLC_PRED_REC + 2]) * LPCN_NB_FEAT + i]; write = true; }
            else if (flags & PLC_F_KEEP) { v = out[i * S + a]; write = true; }
            if (write && i == 0 && (flags & PLC_F_ATT)) {
                v = v + __int_as_float(rec[a * PLC_PRED_REC + 3]);
                v = v - __int_as_float(rec[a * PLC_PRED_REC + 4]);
                v = -10.f > v ? -10.f : v;
            }
            if (write) D.feat[(size_t)s * LPCN_NB_FEAT + i] = v;
            if ((flags & PLC_F_RAW) && raw_out) raw_out[(size_t)s * LPCN_NB_FEAT + i] = out[i * S + a];
        }
    }
}

template <int S>
__global__ __launch_bounds__(PLC_PRED_THREADS) void plc_pred_s_kernel(PlcNet P, const int *ctl, int cnt, PlcData D, float *raw_out)
{
    plc_pred_s_body<S, float>(P, ctl, cnt, D, raw_out);
}
// ... and an int8 blob's, with gru_b_i8.  (Named _int8: every *_i8_kernel<int> of the engine is a DRED kernel to the DRED resource tests.)
template <int S>
__global__ __launch_bounds__(PLC_PRED_THREADS) void plc_pred_s_int8_kernel(PlcNetQ P, const int *ctl, int cnt, PlcData D, float *raw_out)
{
    plc_pred_s_body<S, int>(P, ctl, cnt, D, raw_out);
}

// Element-wise per-stream operations.  One workgroup per record {stream, a, b}; pcm [n][160] is the call's frame, gpcm the compacted
// PCM of the group that has just run (row a of it belongs to this record's stream).
__global__ __launch_bounds__(PLC_MIX_THREADS) void plc_mix_kernel(int op, const int *ctl, int cnt, short *pcm, const short *gpcm, PlcData D, lpcn_stream_state *states)
{
    if ((int)blockIdx.x >= cnt) return;
    const int *rec = ctl + (size_t)blockIdx.x * PLC_MIX_REC;
    const int s = rec[0], a = rec[1], b = rec[2];
    const int t = threadIdx.x;
    short *p = pcm + (size_t)s * LPCN_FRAME_SIZE;
    short *q = D.q + (size_t)s * LPCN_PLC_QUEUE;
    switch (op) {
    case PLC_MIX_QTAIL:           // RNN_COPY(st->pcm, &pcm[80], 80), src/lpcnet_plc.c:249
        if (t < 80) q[t] = p[80 + t];
        break;
    case PLC_MIX_QAPPEND:         // RNN_COPY(&st->pcm[st->pcm_fill], pcm, 160), :252
        if (t < LPCN_FRAME_SIZE) q[a + t] = p[t];
        break;
    case PLC_MIX_QPUSH: {         // st->pcm[400 + i] = pcm[i]; RNN_MOVE(st->pcm, &st->pcm[160], 400), :276-285
        short v = 0;
        if (t < LPCN_PLC_BUF_SIZE) v = t + LPCN_FRAME_SIZE < LPCN_PLC_BUF_SIZE ? q[t + LPCN_FRAME_SIZE] : p[t + LPCN_FRAME_SIZE - LPCN_PLC_BUF_SIZE];
        __syncthreads();
        if (t < LPCN_PLC_BUF_SIZE) q[t] = v;
        if (t < LPCN_FRAME_SIZE) q[LPCN_PLC_BUF_SIZE + t] = p[t];
        break;
    }
    case PLC_MIX_QSHIFT: {        // RNN_MOVE(st->pcm, &st->pcm[160], 400), :310
        short v = 0;
        if (t < LPCN_PLC_BUF_SIZE) v = q[t + LPCN_FRAME_SIZE];
        __syncthreads();
        if (t < LPCN_PLC_BUF_SIZE) q[t] = v;
        break;
    }
    case PLC_MIX_FAPPEND: {       // run_frame_network_deferred (src/lpcnet.c:122-133): a = fill before, b = 0 st->features, 1 the analysed features
        float *fb = D.fbuf + (size_t)s * LPCN_PLC_FBUF * LPCN_NB_FEAT;
        float v = 0.f;
        const bool full = a == LPCN_PLC_FBUF;
        if (full && t < (LPCN_PLC_FBUF - 1) * LPCN_NB_FEAT) v = fb[t + LPCN_NB_FEAT];
        __syncthreads();
        if (full && t < (LPCN_PLC_FBUF - 1) * LPCN_NB_FEAT) fb[t] = v;
        const int row = full ? LPCN_PLC_FBUF - 1 : a;
        if (t < LPCN_NB_FEAT) fb[row * LPCN_NB_FEAT + t] = b ? D.an[(size_t)s * LPCN_AN_NB_FEATURES + t] : D.feat[(size_t)s * LPCN_NB_FEAT + t];
        break;
    }
    case PLC_MIX_RESETSIG: {      // lpcnet_reset_signal (src/lpcnet.c:225-232)
        lpcn_stream_state *st = &states[s];
        for (int k = t; k < LPCN_N_A; k += blockDim.x) st->gru_a[k] = 0.f;
        if (t < LPCN_N_B) st->gru_b[t] = 0.f;
        if (t < LPCN_LPC_ORDER) st->last_sig[t] = 0.f;
        if (t == 0) { st->deemph_mem = 0.f; st->last_exc = lpcn_lin2ulaw(0.f); }
        break;
    }
    case PLC_MIX_DCRECV:          // pcm[i] += lp[i], :288-292
        if (t < LPCN_FRAME_SIZE) p[t] = (short)((int)p[t] + (int)D.lp[(size_t)s * LPCN_FRAME_SIZE + t]);
        break;
    case PLC_MIX_DCLOST:          // :334-339: serial in double
        if (t == 0) {
            double syn_dc = D.dc[2 * s + 1];
            const int dc = (int)floor(.5 + D.dc[2 * s]);
            for (int i = 0; i < LPCN_FRAME_SIZE; ++i) {
                syn_dc += LPCN_PLC_DC_CONST * ((double)p[i] - syn_dc);
                p[i] = (short)((int)p[i] + dc);
            }
            D.dc[2 * s + 1] = syn_dc;
        }
        break;
    case PLC_MIX_XFADE:           // :229-233
        if (t < 80) {
            const float w = lpcn_plc_fade[t];
            const int delta = D.delta[s];
            const float x0 = w * (float)p[t];
            const float x1 = (1.f - w) * (float)((int)gpcm[(size_t)a * LPCN_FRAME_SIZE + t] - delta);
            p[t] = (short)(int)floor(.5 + (double)x0 + (double)x1);
        }
        break;
    }
}

// lpcnet_plc_fec_add's RNN_MOVE on a full ring (src/lpcnet_plc.c:117-121): rows [keep, keep + rows) of one stream's ring move to the front
__global__ __launch_bounds__(256) void plc_fec_move_kernel(float *ring, int keep, int rows)
{
    const int total = rows * LPCN_NB_FEAT, shift = keep * LPCN_NB_FEAT;
    for (int base = 0; base < total; base += 256) {
        const int k = base + threadIdx.x;
        float v = 0.f;
        if (k < total) v = ring[k + shift];
        __syncthreads();
        if (k < total) ring[k] = v;
        __syncthreads();
    }
}

// A batched FEC feed (plc_plan.h: plc_fec_feed_plan): one workgroup per record {stream, first source row, a, ring row, move-from row, rows
// moved, b, ring row}.  `a` rows of the packed source go into the stream's ring; then, if the call compacts the ring, rows [from, from + rows)
// move to the front -- the rows just appended among them, so the move waits for them -- and `b` more rows follow.  The move overlaps itself
// and is staged through LDS whole.  Ring rows are 80 bytes from a 16-byte-aligned base, so the move goes in float4; the source is the caller's
// pointer with whatever alignment it has and a record copies a few rows of it, in single floats.
constexpr int PLC_FEED_THREADS = 256;
__global__ __launch_bounds__(PLC_FEED_THREADS) void plc_fec_feed_kernel(const int *recs, int cnt, const float *src, float *fec)
{
    __shared__ float4 stage[LPCN_PLC_MAX_FEC * LPCN_NB_FEAT / 4];
    if ((int)blockIdx.x >= cnt) return;
    const int *rec = recs + (size_t)blockIdx.x * PLC_FEED_REC;
    const int s = rec[0], a = rec[2], at_a = rec[3], from = rec[4], rows = rec[5], b = rec[6], at_b = rec[7];
    const int t = threadIdx.x;
    float *ring = fec + (size_t)s * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT;
    const float *v = src + (size_t)rec[1] * LPCN_NB_FEAT;
    for (int k = t; k < a * LPCN_NB_FEAT; k += PLC_FEED_THREADS) ring[at_a * LPCN_NB_FEAT + k] = v[k];
    if (rows > 0) {      // (the record's choice: the whole workgroup takes it)
        __syncthreads();
        const float4 *in4 = (const float4 *)(ring + from * LPCN_NB_FEAT);
        float4 *out4 = (float4 *)ring;
        for (int k = t; k < rows * (LPCN_NB_FEAT / 4); k += PLC_FEED_THREADS) stage[k] = in4[k];
        __syncthreads();
        for (int k = t; k < rows * (LPCN_NB_FEAT / 4); k += PLC_FEED_THREADS) out4[k] = stage[k];
        __syncthreads();
    }
    for (int k = t; k < b * LPCN_NB_FEAT; k += PLC_FEED_THREADS) ring[at_b * LPCN_NB_FEAT + k] = v[a * LPCN_NB_FEAT + k];      // (b > 0 after a move of no rows: keep == 100)
}

// A compacted group's rows in and out, one launch each way and one workgroup per stream of the group (engine_plc.hip: run_group).  Row i of the
// group's arrays belongs to stream map[i].  In: the state record, then what the group's kind needs -- the 20 features of a frame step, or the
// kept frame products (1152 + 48 + 16 floats) a tail group continues from -- and the N samples to impose.  Out: the N samples, the state
// unless the run was a trial, and the frame products where the group keeps them.  State records are 3592 bytes, so 8-byte aligned: they move
// in int2.  The engine's own rows (products, the group's features and PCM, the PCM queue) are 16-byte aligned and move in float4 / int4; a
// caller's features or PCM move that way only where the engine found pointer and stride aligned (feat_vec, pcm_vec), else one element at a time.
constexpr int PLC_GROUP_THREADS = 256;
static_assert(sizeof(lpcn_stream_state) % sizeof(int2) == 0, "state records move in int2");
template <typename V>
__device__ inline void group_copy(void *dst, const void *src, int count, int t)
{
    for (int k = t; k < count; k += PLC_GROUP_THREADS) ((V *)dst)[k] = ((const V *)src)[k];
}
__device__ inline void group_copy_pcm(short *dst, const short *src, int N, int vec, int t)
{
    const int n8 = vec ? N / 8 : 0;
    group_copy<int4>(dst, src, n8, t);
    for (int k = 8 * n8 + t; k < N; k += PLC_GROUP_THREADS) dst[k] = src[k];
}
__device__ inline void group_copy_products(float *da, float *db, float *dl, const float *sa, const float *sb, const float *sl, int t)
{
    group_copy<float4>(da, sa, LPCN_ROWS_A / 4, t);
    group_copy<float4>(db, sb, LPCN_ROWS_B / 4, t);
    group_copy<float4>(dl, sl, LPCN_LPC_ORDER / 4, t);
}
__global__ __launch_bounds__(PLC_GROUP_THREADS) void group_gather_kernel(GroupRows g)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= g.cnt) return;
    const size_t s = (size_t)g.map[i];
    group_copy<int2>(&g.gstates[i], &g.states[s], (int)(sizeof(lpcn_stream_state) / sizeof(int2)), t);
    if (g.feat) {
        const float *f = g.feat + s * g.feat_stride;
        float *d = g.gfeat + (size_t)i * LPCN_NB_FEAT;
        if (g.feat_vec) group_copy<float4>(d, f, LPCN_NB_FEAT / 4, t);
        else group_copy<float>(d, f, LPCN_NB_FEAT, t);
    }
    if (g.keep)
        group_copy_products(g.cond_a + (size_t)i * LPCN_ROWS_A, g.cond_b + (size_t)i * LPCN_ROWS_B, g.lpc + (size_t)i * LPCN_LPC_ORDER,
                            g.keep_a + s * LPCN_ROWS_A, g.keep_b + s * LPCN_ROWS_B, g.keep_lpc + s * LPCN_LPC_ORDER, t);
    if (g.pcm) group_copy_pcm(g.gpcm + (size_t)i * LPCN_FRAME_SIZE, g.pcm + s * g.pcm_stride, g.N, g.pcm_vec, t);
}
__global__ __launch_bounds__(PLC_GROUP_THREADS) void group_scatter_kernel(GroupRows g)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= g.cnt) return;
    const size_t s = (size_t)g.map[i];
    if (g.pcm) group_copy_pcm(g.pcm + s * g.pcm_stride, g.gpcm + (size_t)i * LPCN_FRAME_SIZE, g.N, g.pcm_vec, t);
    if (g.state_back) group_copy<int2>(&g.states[s], &g.gstates[i], (int)(sizeof(lpcn_stream_state) / sizeof(int2)), t);
    if (g.keep)
        group_copy_products(g.keep_a + s * LPCN_ROWS_A, g.keep_b + s * LPCN_ROWS_B, g.keep_lpc + s * LPCN_LPC_ORDER,
                            g.cond_a + (size_t)i * LPCN_ROWS_A, g.cond_b + (size_t)i * LPCN_ROWS_B, g.lpc + (size_t)i * LPCN_LPC_ORDER, t);
}

}  // namespace lpcn
