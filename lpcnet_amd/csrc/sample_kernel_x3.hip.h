// Persistent per-sample kernel, eight float streams per CU as two groups of four half a step apart, on TWELVE waves: three per SIMD (gfx950 / CDNA4).
//
// The schedule, the LDS layout, the leader, the hand-offs and every addition are those of sample_kernel_x2.hip.h (PARITY: src/vec.h:347-404,
// src/nnet.c:326-372,410-448,163-214, src/lpcnet.c:146-167,235-271; bit-identical to it and to the generic-C float build).  What differs is who does
// what.  With two waves per SIMD every interval of that kernel is a chain of latency-bound links on each wave, and only the partner wave can fill
// them; here a SIMD carries one chain wave and two row waves, in 168 VGPRs each:
//
//      waves 0..3    GRU-B's chain of one stream of group Q (grub_lds_loop_s4_v168.inc: the same loop in v128..v167) and its gates, then their P1
//                    segments of P
//      waves 4..11   the candidate heads of Q in the chains' shadow, the start-value pass ("P0") of P -- 2.25 rounds of 512 rows instead of 4.5 of
//                    256, two rounds in flight --, their P1 segments of P
//      LPCN_X3_HELPERS   four of the row waves, one per stream: stage 1 of that stream's tree (tree_stages.h) on the state its chain wave has stored
//      wave LPCN_X3_S2W   stage 2 of the four streams' trees in one packed pass, behind its P1 segments
//
// A lane holds 16 items (64 weight VGPRs) instead of 30, so a candidate slot of more than 16 items is cut: its head -- blocks 0..15, from
// bias + diag*h -- runs one sample ahead on a row wave and parks its partial sums in the rows' pre-activation cells, its tail goes on adding
// from those cells in P1 on ANOTHER wave (model_pack.c: lpcn_model_pack_x3).  That is the hand-off the eight-wave kernel uses between a head
// and the rest of its slot; no sum changes its order.  Every P1 segment therefore starts from the value its rows' cells hold.
//
// Scope: float blobs, PARITY arithmetic, dense GRU-B input matrix, a model that has the twelve-wave image.  Everything else runs on the other kernels.
#pragma once
#include "sample_kernel_x2.hip.h"

namespace lpcn {

#define LPCN_X3_TW 1            // the wave that draws the KISS99 thresholds: a chain wave on another SIMD than the leader's (waves w, w + 4, w + 8 share one: tools/ubench/hwid.hip)
#define LPCN_X3_HG 6            // head items a row wave runs before it polls the leader's indices for the start-value pass
#define LPCN_X3_S2W 11          // the wave that runs stage 2 of the four streams' trees in one pass: any but the leader's.  Row wave 9 / 11, chain wave 0 / 2 / 3: 177.8 / 180.6 / 176.8 / 176.9 / 172.7 M (round 13; the eight-wave form 175.6 M, this kernel with round 6's tree 163.0 M)
#define LPCN_X3_HELPERS 0xA865u  // nibble s: the HELPER wave of stream s, which runs stage 1 of that stream's tree -- row waves 5, 6, 8, 10: none on its stream's chain SIMD, none on the stage-2 wave's.  184.9 M against 180.2 M with stage 1 on the chain waves; {8,5,6,7}, each helper on its chain's SIMD: 180.5 M, a tie (round 14; the other maps in EXPERIMENTS.md)
#define LPCN_X3_S2_LEAD 2       // ... and how many of its P1 items from the end it polls the streams' prefixes and issues the loads of its rows (on wave 11, 1 / 2 / 4: 180.8 / 180.6 / 180.6 M, a tie; at least 1)

// The twelve-wave form's own LDS cells, behind everything LdsX2 lays out (no LdsX2 offset moves): per group one word per stream, the sequence number
// of the sample whose GRU-B state the stream's chain wave has stored.
struct LdsX3 {
    static constexpr int g_seq  = 0;                                // [4] i32
    static constexpr int G_SZ   = 16;
    static constexpr int total(int nb_b) { return LdsX2::total(nb_b) + 2 * G_SZ; }
};
// the helper wave of stream s / the stream a wave helps (-1: none)
constexpr int lpcn_x3_helper_wave(const int s) { return (int)((LPCN_X3_HELPERS >> (4 * s)) & 15u); }
__host__ __device__ constexpr int lpcn_x3_helper_stream(const int wave)
{
    for (int s = 0; s < 4; ++s) if ((int)((LPCN_X3_HELPERS >> (4 * s)) & 15u) == wave) return s;
    return -1;
}
constexpr bool lpcn_x3_helpers_ok()
{
    for (int s = 0; s < 4; ++s) {
        const int w = lpcn_x3_helper_wave(s);
        if (w < LPCN_X3_CHAIN_WAVES || w >= LPCN_X3_WAVES || w == LPCN_X3_LW || w == LPCN_X3_S2W) return false;
        for (int t = 0; t < s; ++t) if (lpcn_x3_helper_wave(t) == w) return false;
    }
    return true;
}
static_assert(lpcn_x3_helpers_ok(), "four distinct helper waves among the row waves, never the leader's or the stage-2 wave");

__global__ __launch_bounds__(LPCN_X3_THREADS, 1) void sample_kernel_x3(const LpcnSampleArgs *__restrict__ Ap)
{
    constexpr int NW = LPCN_X3_NW, WGT = LPCN_X3_THREADS, NSEG = LPCN_X3_SEGS;
    using L = LdsX2;
    constexpr int S = 4;
    constexpr int LW = LPCN_X3_LW, TW = LPCN_X3_TW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *const sm_pre_ur = (float *)(smem + L::pre_ur);
    float *const sm_inh = (float *)(smem + L::inh);
    const float *const sm_abias = (const float *)(smem + L::abias);
    const float *const sm_tansig = (const float *)(smem + L::tansig);
    const float *const sm_ulaw = (const float *)(smem + L::ulaw);
    const float *const sm_logit = (const float *)(smem + L::logit);
    const float *const sm_brec = (const float *)(smem + L::brec);
    const float *const sm_bbias = (const float *)(smem + L::bbias);
    const int *const sm_bstart = (const int *)(smem + L::bstart);

    const int tid0 = threadIdx.x;
    const int n_streams = Ap->n_streams, n_frames = Ap->n_frames, preload = Ap->preload, frame_len = Ap->frame_len;
    const int s0 = blockIdx.x * 2 * S;                      // first stream of this workgroup; group g holds streams s0 + 4 g + {0..3}
    auto stream_of = [&](int gs) __attribute__((always_inline)) { return (s0 + gs < n_streams) ? s0 + gs : n_streams - 1; };      // streams past the end: a clamped copy, never written back
    const int n_valid = (n_streams - s0 < 2 * S) ? n_streams - s0 : 2 * S;
    const size_t nf = (size_t)n_frames;
    auto *const states = as_global_rw(Ap->state);
    const LPCN_GLOBAL float *emb_nat_sig = as_global(Ap->emb_nat_sig), *emb_nat_pred = as_global(Ap->emb_nat_pred), *emb_nat_exc = as_global(Ap->emb_nat_exc);      // [256][1152]
    asm volatile("" : "+s"(emb_nat_sig), "+s"(emb_nat_pred), "+s"(emb_nat_exc));

    // ------------------------------------------------------------------ resident weights ----
    float4 w[NW];
    uint32_t offp[(NW + 1) / 2];
    int row_reg[1 + NSEG];          // segment 0: the head; 1..NSEG: the P1 segments
#define LPCN_ROW(k) (row_reg[k])
    {
        const int lane = tid0 & 63, wave = tid0 >> 6;
        const size_t base = (size_t)wave * NW * 64 + lane;
        const int lane_sel = (lane & 3) * 16;
        const auto *ab = as_global(Ap->a_blk);
        const auto *aw = (const LPCN_GLOBAL float *)as_global(Ap->a_w);
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const auto *v = aw + (base + (size_t)j * 64) * 4;
            w[j] = make_float4(v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int j = 0; j < NW; j += 2) {
            const int p0 = ab[base + (size_t)j * 64];
            const int p1 = (j + 1 < NW) ? ab[base + (size_t)(j + 1) * 64] : 0;
            offp[j >> 1] = (uint32_t)(L::ha_off(p0) + lane_sel) | ((uint32_t)(L::ha_off(p1) + lane_sel) << 16);
        }
        const auto *ar = as_global(Ap->a_row);
#pragma unroll
        for (int k = 0; k <= NSEG; ++k) row_reg[k] = ar[(wave * (1 + NSEG) + k) * 64 + lane];
    }
    // ends of this wave's P1 segments 1..NSEG (items [0, b4); an empty segment ends where it starts)
    int b1 = __builtin_amdgcn_readfirstlane(as_global(Ap->a_bound)[(tid0 >> 6) * (1 + NSEG) + 1]);
    int b2 = __builtin_amdgcn_readfirstlane(as_global(Ap->a_bound)[(tid0 >> 6) * (1 + NSEG) + 2]);
    int b3 = __builtin_amdgcn_readfirstlane(as_global(Ap->a_bound)[(tid0 >> 6) * (1 + NSEG) + 3]);
    int b4 = __builtin_amdgcn_readfirstlane(as_global(Ap->a_bound)[(tid0 >> 6) * (1 + NSEG) + 4]);
    const LPCN_GLOBAL float *fc_w_s = as_global(Ap->fc_w), *fc_b_s = as_global(Ap->fc_b), *fc_f_s = as_global(Ap->fc_f);
    asm volatile("" : "+s"(fc_w_s), "+s"(fc_b_s), "+s"(fc_f_s));
    const LPCN_GLOBAL float *cond_a_s = as_global(Ap->cond_a);
    asm volatile("" : "+s"(cond_a_s));
    const int hl = __builtin_amdgcn_readfirstlane(as_global(Ap->a_head)[tid0 >> 6]);      // items of this wave's head, at [NW - hl, NW)
    const bool p1_wave = __builtin_amdgcn_readfirstlane(b4 > 0 ? 1 : 0) != 0;      // wave-uniform: this wave has P1 items
    const bool early_wave = __builtin_amdgcn_readfirstlane(__ballot(row_reg[0] >= 0) != 0ull ? 1 : 0) != 0;      // wave-uniform: this wave computes a head (rows without blocks: bias + diag*h alone) one sample ahead

    // ------------------------------------------------------------------ LDS residents -------
    {
        const int tid = tid0;
        stage_tables<L>(smem, Ap, tid, NB * RB);
        stage_grub_weights(smem + L::bw, Ap, tid, true);
        for (int i = tid; i < 2 * S * NA; i += WGT) {
            const int gs = i / NA, n = i % NA, g = gs >> 2, s = gs & 3;
            const float hv0 = states[stream_of(gs)].gru_a[n];
            unsigned char *gb = smem + g * L::G_SZ;
            ((float *)(gb + L::g_hT))[n * S + s] = hv0;
            *(float *)(gb + L::g_hA + L::ha_off(n >> 2) + s * 16 + (n & 3) * 4) = hv0;
        }
        for (int i = tid; i < 2 * S * NB; i += WGT) {
            const int gs = i / NB, g = gs >> 2, s = gs & 3;
            ((float *)(smem + g * L::G_SZ + L::g_hB))[s * NB + i % NB] = states[stream_of(gs)].gru_b[i % NB];
        }
        if (tid < 2 * S) {
            const int g = tid >> 2, s = tid & 3;
            unsigned char *gb = smem + g * L::G_SZ;
            stage_leader_record({(float *)(gb + L::g_lead), (int *)(gb + L::g_idx), nullptr, nullptr}, s, &states[stream_of(tid)]);
        }
        if (tid < 2) { int *fl = (int *)(smem + tid * L::G_SZ + L::g_flag); fl[0] = 0; fl[1] = 0; }
        if (tid < 2 * S) ((int *)(smem + (tid >> 2) * L::G_SZ + L::g_pfx))[tid & 3] = 0;      // (no sample has sequence number 0)
        if (tid < 2 * S) ((int *)(smem + L::total(Ap->nb_b) + (tid >> 2) * LdsX3::G_SZ + LdsX3::g_seq))[tid & 3] = 0;
    }
    __syncthreads();

    // ---- leader state: wave LW, lane 16 s + j holds sample j of stream s's LPC history, one register per group
    const bool is_lw = (tid0 >> 6) == LW;                    // (wave-uniform)
    const bool is_tw_lane = tid0 >= 64 * TW && tid0 < 64 * TW + S;
#define LPCN_LROW ((tid0 & 63) >> 4)
#define LPCN_TAP (tid0 & 15)
    // "P" variables belong to the group that runs P1 / P2 in the current half-step, "Q" to the one that runs P3 / P4; they swap at its end.
    // The loop starts at h = -1 with P = group 1, Q = group 0.
    float histP = is_lw ? states[stream_of(S + LPCN_LROW)].last_sig[LPCN_TAP] : 0.f;
    float histQ = is_lw ? states[stream_of(LPCN_LROW)].last_sig[LPCN_TAP] : 0.f;
    bool liveP = false, liveQ = false;                       // per lane: leader lanes (their stream), threshold lanes
    int live_maskP = 0, live_maskQ = 0;                      // bit s: stream s of the group produces samples in its current frame
    int seqP = 0, seqQ = 0;                                  // samples opened so far, per group (identical in every wave)
    int smpP = 0, smpQ = 0, fP = 0, fQ = 0;                  // position of the group's NEXT P1 sample: sample within the frame, frame
    float lpc_tap = 0.f, prod_old = 0.f;                     // leader lanes: computed behind the tree of a group, used when its sample is finished

    const int T = n_frames * frame_len;                      // samples per stream in this launch
    const int x3_cells = __builtin_amdgcn_readfirstlane(L::total(Ap->nb_b));
#if LPCN_ENABLE_PROF
    // per-phase shader-clock accounting of workgroup 0 (profiling builds only): the slots and LPCN_X2_PROF of sample_kernel_x2.hip.h, waves 0..7
    unsigned long long *const prof = Ap->prof;
    unsigned long long pt[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
    const bool profiling = prof != nullptr && blockIdx.x == 0;
    if (profiling) tprev = __builtin_amdgcn_s_memtime();
#endif
    // ====================================================================== half-steps ======
    for (int h = -1; h <= 2 * T + 1; ++h) {
        const int p = h & 1, q = p ^ 1;
        unsigned char *const gp = smem + p * L::G_SZ, *const gq = smem + q * L::G_SZ;
        const bool p_active = h >= 0 && (h >> 1) < T;        // group P starts a sample in this half-step
        const bool p_prev = h >= 2;                          // group P's previous sample has been through its tree: the leader finishes it now
        const bool q_chain = h >= 1 && ((h - 1) >> 1) < T;   // group Q has a sample in GRU-B / the tree
        const bool q_heads = ((h + 1) >> 1) < T;             // group Q starts another sample in the next half-step: its candidate heads run now
        const bool new_frame = p_active && smpP == 0;
        const bool more = p_active && smpP != 0;             // P's new sample continues the frame of the one just finished
        float *const hT_p = (float *)(gp + L::g_hT);
        float *const hB_q = (float *)(gq + L::g_hB);
        int *const idx_p = (int *)(gp + L::g_idx);
        float *const lpc_p = (float *)(gp + L::g_lpc);
        short *const pcm_p = (short *)(gp + L::g_pcm);
        const LeaderCells cells_p = {(float *)(gp + L::g_lead), idx_p, (float *)(gp + L::g_thr), pcm_p};      // group P's leader cells (sample_common.hip.h)
        const uint32_t flag_p = lds_addr(gp + L::g_flag);
        unsigned char *const xq = smem + x3_cells + q * LdsX3::G_SZ;      // group Q's sequence words (LdsX3)

        // ------------------------------------------------ the leader finishes group P's previous sample --
        if (more) ++seqP;
        if (p_prev && is_lw) {
            __builtin_amdgcn_s_setprio(3);
            const int smp_done = smpP == 0 ? frame_len - 1 : smpP - 1;      // index of the finished sample in its frame
            int t_ = tid0;
            LPCN_REMAT_V(t_);                                // (lane-derived indices are rebuilt here: hoisted out of the loop they are spilled, and a scratch reload on the leader's path is ~0.5 k clk)
            const int lrow = (t_ & 63) >> 4, tap = t_ & 15;
            float pcm, deemph;
            int exc;
            draw_sample_walked(cells_p, (const int *)(gp + L::g_mask) + lrow, sm_ulaw, lrow, tap, liveP, smp_done, preload, histP, pcm, deemph, exc);
            // the next sample's indices first (wave LW publishes them through idx_p + flag_p): the row waves are waiting for them
            if (more) { open_sample<S>(cells_p, tid0, liveP, pcm, tap == 0 ? pcm * lpc_tap : prod_old, exc, false); lds_publish(flag_p, seqP); }
            __builtin_amdgcn_s_setprio(0);
            finish_sample(cells_p, lrow, tap, liveP, smp_done, preload, pcm, deemph);
        }
        if (more && is_tw_lane && liveP) { int t_ = tid0; LPCN_REMAT_V(t_); draw_thresholds(cells_p, sm_logit, t_ - 64 * TW); }

        // ------------------------------------------------ group P enters a new frame --------------------
        if (new_frame) {
            int tid = tid0;
            LPCN_REMAT_V(tid);                                // (lane-derived values are rebuilt here: hoisted out of the half-step loop they are spilled)
            const bool lw_ = (tid >> 6) == LW, twl_ = tid >= 64 * TW && tid < 64 * TW + S;
            __syncthreads();                                  // the leader's last sample of the previous frame
            if (fP > 0) {                                     // flush the finished frame's PCM (4 x 160 samples, coalesced)
                auto *out = as_global_rw(Ap->pcm);
                const size_t pstride = (size_t)Ap->pcm_stride;
                for (int i = tid; i < S * LPCN_FRAME_SIZE; i += WGT) {
                    const int s = i / LPCN_FRAME_SIZE, k = i % LPCN_FRAME_SIZE;
                    if (S * p + s < n_valid && k < frame_len) out[(size_t)(s0 + S * p + s) * pstride + (size_t)(fP - 1) * LPCN_FRAME_SIZE + k] = pcm_p[i];
                }
            }
            __syncthreads();                                  // (preload below overwrites the buffer)
            {
                const auto *cb = as_global(Ap->cond_b), *lp = as_global(Ap->lpc);
                float *const condb_p = (float *)(gp + L::g_condb);
                if (tid < S * RB) condb_p[tid] = cb[((size_t)stream_of(S * p + tid / RB) * nf + fP) * RB + tid % RB];
                if (tid >= 256 && tid < 256 + S * LPCN_LPC_ORDER) {
                    const int i = tid - 256;
                    lpc_p[i] = lp[((size_t)stream_of(S * p + i / LPCN_LPC_ORDER) * nf + fP) * LPCN_LPC_ORDER + i % LPCN_LPC_ORDER];
                }
                if (lw_ || twl_) {
                    const int lstream = stream_of(S * p + (lw_ ? (tid & 63) >> 4 : tid - 64 * TW));
                    liveP = stream_is_live(Ap, states, lstream, fP);
                }
                if (preload > 0 && tid < S) {
                    const auto *pin = as_global(Ap->pcm) + (size_t)stream_of(S * p + tid) * (size_t)Ap->pcm_stride + (size_t)fP * LPCN_FRAME_SIZE;
                    for (int i = 0; i < preload; ++i) pcm_p[tid * LPCN_FRAME_SIZE + i] = pin[i];
                }
            }
            __syncthreads();                                  // lpc_p visible to the leaders
            ++seqP;
            if (lw_) {
                open_sample<S>(cells_p, tid0, liveP, histP, histP * lpc_p[tid & 63], ((const int *)cells_p.lead)[((tid & 63) >> 4) * 8 + 2], true);
                lds_publish(flag_p, seqP);
            }
            if (twl_ && liveP) draw_thresholds(cells_p, sm_logit, tid - 64 * TW);
            __syncthreads();
            int lm = 0;
#pragma unroll
            for (int s = 0; s < S; ++s) lm |= (idx_p[S + s] ? 1 : 0) << s;
            live_maskP = __builtin_amdgcn_readfirstlane(lm);
        }

        LPCN_X2_PROF(0);
        // ================================================================ interval A ===========
        // ---- shared pieces of the item chains (P1 of group P, candidate heads of group Q)
        float acc[S] = {};
        constexpr int PF = 1;                                // state blocks fetched one item ahead (two, the eight-wave kernel's value, costs four VGPRs that the 168 do not have: a weight tuple is spilled; measured again in round 13 with the tree off the row waves: 177.8 against 177.8 M on wave 9, a tie, not kept)
        float4 hq[PF + 1] = {};
        const unsigned char *hA_cur = gp + L::g_hA;           // state blocks of the group whose items are running
        auto fetch_h = [&](const int j) __attribute__((always_inline)) {
            uint32_t pk = offp[j >> 1];
            LPCN_REMAT_V(pk);
            const uint32_t off = (j & 1) ? (pk >> 16) : (pk & 0xFFFFu);
            hq[j % (PF + 1)] = *(const float4 *)(hA_cur + off);
        };
        typedef float negz_t __attribute__((ext_vector_type(4)));
        negz_t negz = {-0.f, -0.f, -0.f, -0.f};
        auto load_negz = [&]() __attribute__((always_inline)) { negz = (negz_t){-0.f, -0.f, -0.f, -0.f}; asm volatile("" : "+v"(negz)); };
        // one item = (this lane's row) x (one 4-wide input block) for the four streams of a group: the products of a column from ONE
        // v_mfma_f32_4x4x1 with C = -0.0 (bit for bit the separately rounded product), the sums as v_pk_add_f32 over stream pairs, columns
        // 0..3 in order (src/vec.h:355-401)
        auto mac = [&](const int j) __attribute__((always_inline)) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            typedef float f2 __attribute__((ext_vector_type(2)));
            const float4 hv = hq[j % (PF + 1)];
            const float hk[4] = {hv.x, hv.y, hv.z, hv.w};
            const float wk[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
            f2 a01 = {acc[0], acc[1]}, a23 = {acc[2], acc[3]};
            f4 pv[4];
            // (the four products of an item are issued back to back into four result tuples, then the sums.  Round 6 tried to software-pipeline the
            // items by one -- the matrix-pipe instructions of item j + 1 between / behind the adds of item j, in one or in two sets of product
            // registers: bit-exact and far slower, 113.8 vs 145.6 M samples/s -- an MFMA between dependent packed adds stalls both)
#pragma unroll
            for (int c = 0; c < 4; ++c) pv[c] = __builtin_amdgcn_mfma_f32_4x4x1f32(hk[c], wk[c], negz, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                a01 = a01 + __builtin_shufflevector(pv[c], pv[c], 0, 1);
                a23 = a23 + __builtin_shufflevector(pv[c], pv[c], 2, 3);
            }
            acc[0] = a01[0]; acc[1] = a01[1]; acc[2] = a23[0]; acc[3] = a23[1];
        };
        // pre-activation cell of GRU-A row r: update / reset rows share one copy, candidate rows have one per group
        auto pre_cell = [&](const int r, unsigned char *gb) __attribute__((always_inline)) -> float * {
            return (float *)(r < 2 * NA ? smem + L::pre_ur + r * (S * 4) : gb + L::g_prec + (r - 2 * NA) * (S * 4));
        };

        const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
        // Order of an interval on one wave (round 6, third form.  The first ran P3 of Q, then all of P1 of P, and every wave then sat ~4 k clk behind
        // its own embedding gather; the second issued each wave's gather before Q's chain / heads and the 60 values in flight pushed GRU-A's weights
        // into scratch -- profiles/r06_x2_phase_v1.txt):
        //   2. head waves: the first LPCN_X3_HG items of Q's candidate heads (the leader needs ~1.5 k clk to publish P's indices)
        //   3. waves 4..7: poll the indices, then the START VALUES of ALL of P's GRU-A rows as one element-wise pass ("P0"): row r of the natural
        //      [256][1152] tables per lane -- every load a contiguous 256 B per wave, the conditioning row straight from cond_a -- written to the
        //      rows' pre-activation cells (update / reset rows) or the candidate inputs; an arrival counter tells the row owners
        //   4. Q's GRU-B chains (waves 0..3) / the rest of Q's heads
        //   5. P's items from the parked start values, close.
        // The waves that carry GRU-B's chains -- the longest link of an interval -- neither gather nor wait for a gather.
        // ---------------------------------------------------------------- 2..4: P3 of group Q around P's start-value pass ----
        // The HEAD of group Q's next candidate chains: the first `hl` blocks of every row of this wave's candidate slot (items [NW - hl, NW)) from
        // bias + diag*h -- final once Q's gate stage is done -- parked in the rows' pre-activation cells; the slot continues from there in Q's next P1.
        constexpr int J0 = 0;
        constexpr int JM = J0 + LPCN_X3_HG < NW ? J0 + LPCN_X3_HG : NW;
        const bool do_heads = early_wave && q_heads;
        int e0 = NW - hl;
        LPCN_REMAT_S(e0);
        auto head_step = [&](auto self, auto jc, auto jend_c) __attribute__((always_inline)) -> void {
            constexpr int j = decltype(jc)::value, je = decltype(jend_c)::value;
            if constexpr (j < je) {
                if constexpr (j + PF < NW) fetch_h(j + PF);
                if (j >= e0) { asm volatile(""); mac(j); }   // (every step issues the same LDS read whether its item runs or not: exact wait counts)
                self(self, std::integral_constant<int, j + 1>{}, jend_c);
            }
        };
        const uint32_t p0cnt_p = flag_p + 4;                 // arrival counter of P's start-value pass
        // ---- 3: P0 of group P on waves 4..7, in five stages that are interleaved with the rest of Q's heads (the loads of a round land while head items run)
        constexpr int CW = LPCN_X3_CHAIN_WAVES, P0W = LPCN_X3_CHAIN_WAVES, NP0 = LPCN_X3_WAVES - P0W;      // waves 0..3 carry GRU-B's chains (one stream each), waves 4..11 the heads and the start-value pass
        static_assert(NP0 * 64 * 3 == 4 * NA && NP0 * 64 * 2 + 128 == RA && CW == S, "a round and a half of the row waves' lanes cover GRU-A's update / reset rows, two and a quarter all rows");
        const bool p0_wave = p_active && wave >= P0W;
        uint32_t o_sig[S] = {}, o_pred[S] = {}, o_exc[S] = {}, o_cond[S] = {};      // byte offsets of the streams' table rows (scalar) -- the lane adds its row
        constexpr unsigned P0PERM = 0x17065432u;             // waves 4..11 take lanes 128.., 192.., 256.., 320.., 384.., 0.., 448.., 64.. of the pass: the quarter round on waves 9 and 11 (no head / the shortest)
        int i0 = 0;
        float ld[2][4 * S] = {};
        auto p0_open = [&]() __attribute__((always_inline)) {
            int gi[S];
            {   // poll the flag and fetch the four index words in ONE LDS round trip (a wave's LDS operations complete in order: indices read behind a flag that has the
                // new sequence number are the new ones): 156.9 -> 158.0 M.  The polls of this kernel do not sleep between reads (156.1 vs 155.3 M with s_sleep 1).  (The same merge for the chains' counter + the tree's state reads, and for P0's counter +
                // slot 0's cell: 157.5 / 157.1 vs 157.7 M, not kept.)
                typedef int i4 __attribute__((ext_vector_type(4)));
                i4 v;
                int f;
                const uint32_t idx_a = lds_addr(idx_p);
                do {
                    asm volatile("ds_read_b32 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(f), "=&v"(v) : "v"(flag_p), "v"(idx_a) : "memory");
                    f = __builtin_amdgcn_readfirstlane(f);
                } while (f != seqP);
#pragma unroll
                for (int s = 0; s < S; ++s) gi[s] = __builtin_amdgcn_readfirstlane(v[s]);
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                o_sig[s] = (uint32_t)(gi[s] & 0xFF) * (uint32_t)(RA * 4);
                o_pred[s] = (uint32_t)((gi[s] >> 8) & 0xFF) * (uint32_t)(RA * 4);
                o_exc[s] = ((uint32_t)(gi[s] >> 16) & 0xFFu) * (uint32_t)(RA * 4);
                o_cond[s] = (uint32_t)(((size_t)stream_of(S * p + s) * nf + (size_t)fP) * RA * 4);     // (< 4 GB: the engine bounds the chunk)
            }
            int t_ = tid0;
            LPCN_REMAT_V(t_);
            i0 = (int)(((P0PERM >> (4 * (((t_ >> 6) - P0W) & 7))) & 7u) << 6) | (t_ & 63);   // lane i0 of the 512 takes rows i0 + 512 k; the quarter round (k = 2: rows 1024..1151) goes to the two waves with i0 < 128
        };
        const bool third = ((P0PERM >> (4 * ((wave - P0W) & 7))) & 7u) < 2u;      // (wave-uniform)
        auto issue = [&](const int k, const int buf) __attribute__((always_inline)) {
            const uint32_t rb = (uint32_t)(i0 + 512 * k) * 4u;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                ld[buf][4 * s + 0] = *(const LPCN_GLOBAL float *)((const LPCN_GLOBAL char *)cond_a_s + (o_cond[s] + rb));
                ld[buf][4 * s + 1] = *(const LPCN_GLOBAL float *)((const LPCN_GLOBAL char *)emb_nat_sig + (o_sig[s] + rb));
                ld[buf][4 * s + 2] = *(const LPCN_GLOBAL float *)((const LPCN_GLOBAL char *)emb_nat_pred + (o_pred[s] + rb));
                ld[buf][4 * s + 3] = *(const LPCN_GLOBAL float *)((const LPCN_GLOBAL char *)emb_nat_exc + (o_exc[s] + rb));
            }
        };
        auto reduce = [&](const int k, const int buf) __attribute__((always_inline)) {
            const int r = i0 + 512 * k;
            float g[S];
#pragma unroll
            for (int s = 0; s < S; ++s) g[s] = ((ld[buf][4 * s + 0] + ld[buf][4 * s + 1]) + ld[buf][4 * s + 2]) + ld[buf][4 * s + 3];      // src/nnet.c:487-489
            if (r < 2 * NA) {                                // (wave-uniform) update / reset rows: start value = (bias + diag*h) + input (src/nnet.c:431-440)
                const int n = r >= NA ? r - NA : r;
                const float2 bd = *(const float2 *)(sm_abias + 2 * r);
                const float4 hv = *(const float4 *)(hT_p + n * S);
                *(float4 *)(sm_pre_ur + r * S) = make_float4((bd.x + bd.y * hv.x) + g[0], (bd.x + bd.y * hv.y) + g[1], (bd.x + bd.y * hv.z) + g[2], (bd.x + bd.y * hv.w) + g[3]);
            } else {                                         // candidate rows: the input part goes to the gate stage
                *(float4 *)(sm_inh + (r - 2 * NA) * S) = make_float4(g[0], g[1], g[2], g[3]);
            }
        };
        // The two kinds of waves take disjoint paths (so that the 64 registers GRU-B's assembly block names and the 48 loads of the start-value pass in
        // flight never count against each other in the register allocation):
        if (wave < CW) {
            if (q_chain) {
                // GRU-B of stream `wave` of group Q: one lane per output row, 384 dependent adds per row in the reference's order (src/nnet.c:326-372); the
                // state operand is a broadcast LDS read of the block the gate stage has written (grub_lds_loop_s4.inc, tools/gen_grub_asm.py --lds 4).
                // Round 6 measured three other forms of this link on the two-group kernel, all bit-exact, all slower (EXPERIMENTS.md): two streams per
                // wave with 3 reads per block (92 clk per block), the same packed over the stream pair (90), all four streams on one wave with the
                // products on the matrix pipe (135) -- per stream-block cheaper, but the interval waits for its longest chain.
                __builtin_amdgcn_s_setprio(3);
                const int s = wave;
                int ln_ = tid0;
                LPCN_REMAT_V(ln_);                           // (lane-derived addresses are rebuilt here: hoisted out of the loop they are spilled, and their scratch reloads sit in front of the chain)
                ln_ &= 63;
                const int r = ln_ < RB ? ln_ : RB - 1;
                const int g6 = r >> 3, ri = r & 7;
                const float *const condb_q = (const float *)(gq + L::g_condb);
                float zrh = sm_bbias[r] + condb_q[s * RB + r];                  // src/nnet.c:351
                float rec = sm_bbias[RB + r];
#pragma unroll
                for (int j = 0; j < NB; ++j) rec = rec + sm_brec[j * RB + r] * hB_q[s * NB + j];
                uint32_t wp32 = lds_addr(smem + L::bw + (sm_bstart[g6] * 8 + ri) * 16 + ((LPCN_GRUB_SHIFT >> (4 * g6)) & 15) * 128);
                uint32_t hp32 = lds_addr(gq + L::g_hA + s * 16);
                asm volatile(
#include "grub_lds_loop_s4_v168.inc"
                    : [z] "+v"(zrh), [wp] "+v"(wp32), [hp] "+v"(hp32) : : LPCN_GRUB_LDS168_CLOBBERS);
                __builtin_amdgcn_s_setprio(0);
                LPCN_X2_PROF(1);
                // gates: rows [0,16) update, [16,32) reset, [32,48) candidate (src/nnet.c:362-371)
                const int ln = ln_ & 15;
                const float sg = lpcn_sigmoid(zrh + rec, sm_tansig);
                const float r_gate = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((16 + ln) << 2, __builtin_bit_cast(int, sg)));
                const float hc = lpcn_tanh(zrh + rec * r_gate, sm_tansig);
                const float hc_i = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((32 + ln) << 2, __builtin_bit_cast(int, hc)));
                if (ln_ < NB) {
                    const float hold = hB_q[s * NB + ln_];
                    const float hnew = sg * hold + (1.f - sg) * hc_i;
                    if ((live_maskQ >> s) & 1) hB_q[s * NB + ln_] = hnew;
                }
                LPCN_X2_PROF(2);
                // The state is stored: the sample's sequence number goes out behind the stores (a wave's LDS operations complete in order), and this wave
                // goes on to its P1 items -- 15 or 16 of them on the benchmark model, the longest path of interval A.  Stage 1 of the stream's tree, which
                // ran here until round 14, is the helper wave's (below): a clamped copy's chain publishes like any other.
                lds_publish(lds_addr(xq + LdsX3::g_seq) + s * 4, seqQ);
            }
            // (Round 6 also gave these waves a share of P's start-value pass -- a round of update / reset rows and one of candidate inputs, or the candidate
            // inputs alone, issued above the gates: 144.0 / 145.7 vs 147.0 M.  With only the barrier waits instrumented the chain waves have 1.3-2.2 k clk
            // of slack per half-step, not the 4 k the full phase table shows; EXPERIMENTS.md.)
        } else {
            if (do_heads) {
                hA_cur = gq + L::g_hA;
                load_negz();
                {
                    int r = LPCN_ROW(0);
                    LPCN_REMAT_V(r);
                    r = r < 0 ? 0 : r;
                    const int n = r - 2 * NA;
                    const float bias = sm_abias[2 * r], diag = sm_abias[2 * r + 1];
                    const float *hT_q = (const float *)(gq + L::g_hT);
#pragma unroll
                    for (int s = 0; s < S; ++s) acc[s] = bias + diag * hT_q[n * S + s];
                }
#pragma unroll
                for (int j = 0; j < PF; ++j) if (J0 + j < NW) fetch_h(J0 + j);
                head_step(head_step, std::integral_constant<int, J0>{}, std::integral_constant<int, JM>{});
            }
            LPCN_X2_PROF(3);
            // both full rounds are issued at once (32 loads per lane in flight) and announced -- the row owners wait for the update / reset rows in them --,
            // the quarter round of candidate inputs, which only the gate stage behind the barrier needs, lands behind the rest of the heads
            if (p0_wave) {
                p0_open();
                LPCN_X2_PROF(1);                             // (head waves: slot 1 = wait for the indices, slot 2 = issue of the rounds)
                issue(0, 0); issue(1, 1);
                LPCN_X2_PROF(2);
                reduce(0, 0); reduce(1, 1);
                lds_arrive(p0cnt_p);                         // (behind the stores of the two rounds: every update / reset row is in them)
                if (third) issue(2, 0);
            }
            LPCN_X2_PROF(4);
            if (do_heads) {
                head_step(head_step, std::integral_constant<int, JM>{}, std::integral_constant<int, NW>{});
                int r = LPCN_ROW(0);
                LPCN_REMAT_V(r);
                if (r >= 0) {
                    float *c = pre_cell(r, gq);
#pragma unroll
                    for (int s = 0; s < S; ++s) c[s] = acc[s];
                }
            }
            if (p0_wave && third) reduce(2, 0);
            LPCN_X2_PROF(3);
        }

        // ---------------------------------------------------------------- P4 of group Q, stage 2, first part (wave LPCN_X3_S2W) ----
        // Four streams in one pass: lane 16 f + l is local lane l of stream f (tree_stages.h, packed mapping).  Each lane reads its stream's cell until all
        // four carry this sample's sequence number, then fetches the row of its node in the subtree its stream's prefix names.  This happens
        // LPCN_X3_S2_LEAD items before the end of the wave's P1 segments: the rows land under those, and the chains have published by then.
        static_assert(LPCN_X3_S2W != LPCN_X3_LW && LPCN_X3_S2W >= 0 && LPCN_X3_S2W < LPCN_X3_WAVES && LPCN_TREE_FIELDS == S && LPCN_X3_S2_LEAD >= 1, "stage 2 runs on any wave but the leader's, one field per stream");
        const bool s2_wave = q_chain && wave == LPCN_X3_S2W;      // (wave-uniform)
        TreeRow sub = {};
        int pfx = 0;
        auto s2_open = [&]() __attribute__((always_inline)) {
            int t_ = tid0;
            LPCN_REMAT_V(t_);
            const uint32_t cell = lds_addr(gq + L::g_pfx) + (uint32_t)lpcn_tree_packed_field(t_ & 63) * 4u;
            do {
                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(pfx) : "v"(cell) : "memory");
            } while (__ballot((pfx >> LPCN_TREE_TOP) != seqQ) != 0ull);
            pfx &= (1 << LPCN_TREE_TOP) - 1;
            sub = tree_row_load_packed(fc_w_s, fc_b_s, fc_f_s, t_ & 63, pfx);
        };
        const bool s2_in_items = s2_wave && p_active && b4 > 0;      // (a wave without items, a half-step without P1: in front of the barrier's work)
        if (s2_wave && !s2_in_items) s2_open();

        // ---------------------------------------------------------------- 5: P1 of group P ----
        if (p_active && p1_wave) {                           // (wave-uniform.  A wave without P1 items has no rows to start or to close and nothing of P0's to wait for; until round 14 it polled
                                                             // the arrival counter and swapped three absent rows all the same, which on a helper wave stands in front of the tree)
            hA_cur = gp + L::g_hA;
            load_negz();
            lds_poll_until<false>(p0cnt_p, seqP * NP0);       // the start values of the update / reset rows and the candidate inputs come from P0
            LPCN_X2_PROF(11);                                // wait for the start-value pass of the four row waves
            // segment 1 becomes the running row, from the value its cells hold: P0's start value (update / reset rows) or the sums the head has parked
            {
                int r = LPCN_ROW(1);
                LPCN_REMAT_V(r);
                r = r < 0 ? 0 : r;
                const float *c = pre_cell(r, gp);
#pragma unroll
                for (int s = 0; s < S; ++s) acc[s] = c[s];
            }
            auto row_swap = [&](const int k_done, const int k_next) __attribute__((always_inline)) {   // finished row out, next row in
                int r = LPCN_ROW(k_done), r2 = LPCN_ROW(k_next);
                LPCN_REMAT_V(r);
                LPCN_REMAT_V(r2);
                if (r >= 0) {
                    float *c = pre_cell(r, gp);
#pragma unroll
                    for (int s = 0; s < S; ++s) c[s] = acc[s];
                }
                r2 = r2 < 0 ? 0 : r2;
                const float *c2 = pre_cell(r2, gp);
#pragma unroll
                for (int s = 0; s < S; ++s) acc[s] = c2[s];
            };
            auto row_store = [&](const int k) __attribute__((always_inline)) {
                int r = LPCN_ROW(k);
                LPCN_REMAT_V(r);
                if (r >= 0) {
                    float *c = pre_cell(r, gp);
#pragma unroll
                    for (int s = 0; s < S; ++s) c[s] = acc[s];
                }
            };
            const int jend = b4;
            LPCN_X2_PROF(4);
#pragma unroll
            for (int j = 0; j < PF && j < NW; ++j) fetch_h(j);
            LPCN_REMAT_S(b1);
            LPCN_REMAT_S(b2);
            LPCN_REMAT_S(b3);
            LPCN_REMAT_S(b4);
            // All tests below are wave-uniform scalar branches; an ordinary item falls through every one of them.
            int s2_at = s2_in_items ? (jend > LPCN_X3_S2_LEAD ? jend - LPCN_X3_S2_LEAD : 0) : NW + 1;      // stage 2 of Q's trees opens in front of this item
            LPCN_REMAT_S(s2_at);
            int nextb = b1;
            if (s2_at < nextb) nextb = s2_at;
            LPCN_REMAT_S(nextb);
            auto item = [&](const int j) __attribute__((always_inline)) -> bool {           // false: this wave has no more items
                if (__builtin_expect(j >= jend, 0)) return false;
                if (j + PF < NW) fetch_h(j + PF);
                if (__builtin_expect(j == nextb, 0)) {       // slot boundaries (a slot may be empty) and the stage-2 wave's opening: ONE compare per item against the next one
                    if (j == b1) row_swap(1, 2);
                    if (j == b2) row_swap(2, 3);
                    if (j == b3) row_swap(3, 4);
                    if (j == s2_at) s2_open();
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    nextb = b1 > j ? b1 : (b2 > j ? b2 : (b3 > j ? b3 : NW));
                    if (s2_at > j && s2_at < nextb) nextb = s2_at;
                }
                mac(j);
                return true;
            };
            auto run_items = [&](auto self, auto jc) __attribute__((always_inline)) -> void {
                constexpr int j = decltype(jc)::value;
                if constexpr (j < NW) {
                    if (!item(j)) return;
                    self(self, std::integral_constant<int, j + 1>{});
                }
            };
            run_items(run_items, std::integral_constant<int, 0>{});
            LPCN_X2_PROF(5);
            // close whichever slot is still open; slots that start exactly at the end have no items
            if (b1 >= jend) {
                row_swap(1, 2);
                row_swap(2, 3);
                row_swap(3, 4);
            } else if (b2 >= jend) {
                row_swap(2, 3);
                row_swap(3, 4);
            } else if (b3 >= jend) {
                row_swap(3, 4);
            }
            row_store(4);
            LPCN_X2_PROF(6);
        }
        // ---------------------------------------------------------------- P4 of group Q, stage 1 (the streams' helper waves) ----
        // The top five levels of stream s's tree on a ROW wave (LPCN_X3_HELPERS), behind the close of its P1 segments -- none on the benchmark model --:
        // the rows of the top levels are the same every sample and are fetched before the poll; the wave then reads the stream's sequence word until
        // the chain wave has published this sample's number behind its state stores, evaluates the 31 nodes on that state and publishes the five
        // decided bits under the same number for the stage-2 wave.  Every half-step with a chain has a publisher for every stream (clamped copies
        // included) and none without one polls: a launch of one sample runs this once per group.
        const int hs = lpcn_x3_helper_stream(wave);           // (wave-uniform)
        if (q_chain && hs >= 0) {
            const int s = hs;
            int ln_ = tid0;
            LPCN_REMAT_V(ln_);
            ln_ &= 63;
            const TreeRow top = tree_row_load<0>(fc_w_s, fc_b_s, fc_f_s, ln_, 0);
            lds_poll_until<false>(lds_addr(xq + LdsX3::g_seq) + s * 4, seqQ);
            const float *const thr_s = (const float *)(gq + L::g_thr) + s * 8;
            const int val = tree_stage_walk<0>(top, hB_q + s * NB, thr_s, sm_tansig, ln_);
            if (ln_ == 0) lds_publish(lds_addr(gq + L::g_pfx) + s * 4, (seqQ << LPCN_TREE_TOP) | val);
        }
        // ---------------------------------------------------------------- P4 of group Q, stage 2, second part ----
        // Behind the close of the segments: the state and the thresholds of the lane's stream, one 64-bit ballot, four three-level walks over its 16-bit
        // fields (scalar); lane 16 f stores stream f's 8 bits for the leader, which reads them behind barriers 1 and 2.  In a group with fewer than four
        // streams the unused fields belong to clamped copies: valid rows, values nobody reads.
        if (s2_wave) {
            int t_ = tid0;
            LPCN_REMAT_V(t_);
            const int ln = t_ & 63, f = lpcn_tree_packed_field(ln);
            const unsigned long long m = tree_node_ballot(sub, hB_q + f * NB, (const float *)(gq + L::g_thr) + f * 8 + lpcn_tree_packed_level(ln), sm_tansig) & lpcn_tree_packed_mask();
            int walks = 0;
#pragma unroll
            for (int k = 0; k < S; ++k) walks |= lpcn_tree_packed_walk(m, k) << (8 * k);
            if ((ln & (LPCN_TREE_FIELD_LANES - 1)) == 0)
                ((int *)(gq + L::g_mask))[f] = (pfx << (LPCN_TREE_LEVELS - LPCN_TREE_TOP)) | ((walks >> (8 * f)) & ((1 << (LPCN_TREE_LEVELS - LPCN_TREE_TOP)) - 1));
        }
        // wave LW: the prediction terms of Q's next sample that do not involve the sample about to be drawn (src/lpcnet.c:252,262)
        if (q_chain && is_lw) {
            int t_ = tid0;
            LPCN_REMAT_V(t_);
            lpc_tap = ((const float *)(gq + L::g_lpc))[t_ & 63];
            prod_old = row_shr1(histQ, 0.f) * lpc_tap;
        }
        LPCN_X2_PROF(9);
        __syncthreads();                                                       // B1
        LPCN_X2_PROF(7);

        // ================================================================ interval B ===========
        int tid = tid0;
        LPCN_REMAT_V(tid);
        // ------------------------------------------------------------ P2 of group P: GRU-A gates (src/nnet.c:441-447) --
        if (p_active) {
            constexpr int NI = NA * S, NQ = NI / WGT;
            const float *const prec_p = (const float *)(gp + L::g_prec);
            float z[NQ], rg[NQ], a[NQ], hold[NQ];
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int i = tid + k * WGT;
                z[k] = sm_pre_ur[i];
                rg[k] = sm_pre_ur[NI + i];
                a[k] = prec_p[i];
                hold[k] = hT_p[i];
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) { z[k] = lpcn_sigmoid(z[k], sm_tansig); rg[k] = lpcn_sigmoid(rg[k], sm_tansig); }
#pragma unroll
            for (int k = 0; k < NQ; ++k) a[k] = a[k] * rg[k] + sm_inh[tid + k * WGT];
#pragma unroll
            for (int k = 0; k < NQ; ++k) a[k] = lpcn_tanh(a[k], sm_tansig);
            // item i = tid + 768 k is (neuron (tid >> 2) + 192 k, stream tid & 3): the stream is the lane's own for both, and the block-ordered copy's address
            // advances by a constant (48 blocks of 64 B + 12 pads of 16 B per 192 neurons)
            const unsigned ut = (unsigned)tid;
            const bool live_s = ((live_maskP >> (ut & 3u)) & 1) != 0;
            unsigned char *const ha0 = gp + L::g_hA + L::ha_off((int)(ut >> 4)) + (ut & 3u) * 16u + ((ut >> 2) & 3u) * 4u;
            static_assert(L::ha_off(48) == 48 * L::HA_STRIDE + 12 * 16 && WGT == 768 && S == 4 && NI % WGT == 0, "gate-stage address stride");
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const float hnew = z[k] * hold[k] + (1.f - z[k]) * a[k];      // src/nnet.c:447
                const float hv = live_s ? hnew : hold[k];
                hT_p[tid + k * WGT] = hv;
                *(float *)(ha0 + k * L::ha_off(48)) = hv;
            }
        }
        LPCN_X2_PROF(8);
        __syncthreads();                                                       // B2
        LPCN_X2_PROF(10);

        // ---- the groups swap roles; P's position advances by the sample it has just started
        if (p_active) { if (++smpP == frame_len) { smpP = 0; ++fP; } }
        { const float t = histP; histP = histQ; histQ = t; }
        { const bool t = liveP; liveP = liveQ; liveQ = t; }
        { const int t = live_maskP; live_maskP = live_maskQ; live_maskQ = t; }
        { const int t = seqP; seqP = seqQ; seqQ = t; }
        { const int t = smpP; smpP = smpQ; smpQ = t; }
        { const int t = fP; fP = fQ; fQ = t; }
        asm volatile("; LPCN_SAMPLE_LOOP_END" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }

#if LPCN_ENABLE_PROF
    if (profiling && (tid0 & 63) == 0 && (tid0 >> 6) < LPCN_WAVES) {      // (the buffer holds eight waves)
#pragma unroll
        for (int i = 0; i < 12; ++i) prof[(tid0 >> 6) * 12 + i] += pt[i];
    }
#endif
    // ---- flush the last frame's PCM of both groups, write the state back.  (After the loop the P variables belong to group 0:
    // 2 T + 3 half-steps = an odd number of swaps from P = group 1.)
    __syncthreads();
    {
        auto *out = as_global_rw(Ap->pcm);
        const size_t pstride = (size_t)Ap->pcm_stride;
        for (int i = tid0; i < 2 * S * LPCN_FRAME_SIZE; i += WGT) {
            const int gs = i / LPCN_FRAME_SIZE, k = i % LPCN_FRAME_SIZE;
            const short *pb = (const short *)(smem + (gs >> 2) * L::G_SZ + L::g_pcm);
            if (gs < n_valid && k < frame_len) out[(size_t)(s0 + gs) * pstride + (size_t)(n_frames - 1) * LPCN_FRAME_SIZE + k] = pb[(gs & 3) * LPCN_FRAME_SIZE + k];
        }
    }
    {
        const int tid = tid0;
        for (int i = tid; i < 2 * S * NA; i += WGT) {
            const int gs = i / NA, n = i % NA;
            if (gs < n_valid) states[s0 + gs].gru_a[n] = ((const float *)(smem + (gs >> 2) * L::G_SZ + L::g_hT))[n * S + (gs & 3)];
        }
        for (int i = tid; i < 2 * S * NB; i += WGT) {
            const int gs = i / NB;
            if (gs < n_valid) states[s0 + gs].gru_b[i % NB] = ((const float *)(smem + (gs >> 2) * L::G_SZ + L::g_hB))[(gs & 3) * NB + i % NB];
        }
        if (is_lw) {
            if (LPCN_LROW < n_valid) states[s0 + LPCN_LROW].last_sig[LPCN_TAP] = histP;
            if (S + LPCN_LROW < n_valid) states[s0 + S + LPCN_LROW].last_sig[LPCN_TAP] = histQ;
        }
        if (tid < n_valid) {
            auto *st = &states[s0 + tid];
            const unsigned char *gb = smem + (tid >> 2) * L::G_SZ;
            const int *li = (const int *)(gb + L::g_lead) + (tid & 3) * 8;
            const float *lp = (const float *)(gb + L::g_lpc);
#pragma unroll
            for (int j = 0; j < LPCN_LPC_ORDER; ++j) st->lpc[j] = lp[(tid & 3) * LPCN_LPC_ORDER + j];
            st->deemph_mem = ((const float *)li)[1];
            st->last_exc = li[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) st->rng[j] = (uint32_t)li[4 + j];
        }
    }
#undef LPCN_ROW
#undef LPCN_LROW
#undef LPCN_TAP
}

}  // namespace lpcn
