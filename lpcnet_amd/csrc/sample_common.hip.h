// What the sample kernels share whatever their schedule (sample_kernel.hip.h: four streams per workgroup, one sample at a time;
// sample_kernel_x2.hip.h: two groups of four, half a step apart): the leader's arithmetic -- the part of a sample that defines
// bit-exactness against the reference beside the mat-vec order --, the hand-offs through LDS that replace workgroup barriers, and
// the staging of tables and leader state into LDS and back.  Written down ONCE: a kernel binds "which LDS cells" (LeaderCells,
// an LDS address) to these functions and keeps only its schedule.  Everything is __forceinline__: the kernels sit at their
// register limit, and tests/test_kernel_resources.py pins what the compiler makes of them.
// Included by sample_kernel.hip.h behind the argument block (LpcnSampleArgs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lpcnet_engine.h"
#include "lpcnet_math.h"

namespace lpcn {

constexpr int NA = LPCN_N_A, NB = LPCN_N_B, RA = LPCN_ROWS_A, RB = LPCN_ROWS_B;

// pointers fetched from the argument block are generic; tell the compiler they are global memory
#define LPCN_GLOBAL __attribute__((address_space(1)))
template <typename T> __device__ __forceinline__ const LPCN_GLOBAL T *as_global(const T *p)
{
    return (const LPCN_GLOBAL T *)(uintptr_t)p;
}
template <typename T> __device__ __forceinline__ LPCN_GLOBAL T *as_global_rw(T *p)
{
    return (LPCN_GLOBAL T *)(uintptr_t)p;
}
// Loop-invariant values that hipcc would otherwise hoist out of the 160-sample loop and keep in
// VGPRs for the whole launch; the weights need that register space.
#define LPCN_REMAT_V(x) asm volatile("" : "+v"(x))
#define LPCN_REMAT_S(x) asm volatile("" : "+s"(x))

// ---- hand-offs through LDS ----------------------------------------------------------------------
// A wave's LDS operations complete in order, so a flag or counter written BEHIND a wave's stores tells every reader that the
// stores have landed: no workgroup barrier, and no store round trip to wait for.
__device__ __forceinline__ uint32_t lds_addr(const void *ptr)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)(unsigned char *)ptr;
}
__device__ __forceinline__ void lds_publish(const uint32_t addr, const int seq)      // behind the data stores of the same lane
{
    asm volatile("ds_write_b32 %0, %1" :: "v"(addr), "v"(seq) : "memory");
}
__device__ __forceinline__ void lds_arrive(const uint32_t addr)                     // one add per wave to an arrival counter
{
    int one = 1;
    unsigned long long ex;
    asm volatile("s_mov_b64 %0, exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "ds_add_u32 %1, %2\n\t"
                 "s_mov_b64 exec, %0"
                 : "=&s"(ex) : "v"(addr), "v"(one) : "memory");
}
// SLEEP: s_sleep 1 between reads -- the four-stream kernel's polls; the two-group kernel's do not sleep (156.1 vs 155.3 M samples/s with it)
template <bool SLEEP> __device__ __forceinline__ void lds_poll_until(const uint32_t addr, const int want)
{
    int v;
    do {
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
        v = __builtin_amdgcn_readfirstlane(v);
        if (SLEEP && v != want) __builtin_amdgcn_s_sleep(1);
    } while (v != want);
}

// ---- the leader: LPC prediction, mu-law indices, thresholds, tree walk, PCM ---------------------
// Leader lanes: the 16 lanes of row s of the leading wave hold stream s's 16-sample history (lane = tap, tap 0 newest,
// src/lpcnet.c:252-263) and walk its tree together; a threshold lane per stream draws the next sample's thresholds on another wave.
// (Callers recompute row / tap from the thread id and re-read the coefficient from LDS where needed: every VGPR that stays live
// across the GRU-A item loop costs the float kernels a spill.)

// value of lane J of the caller's 16-lane row (DPP row_newbcast); the compiler folds it into the consuming VALU op
template <int J> __device__ __forceinline__ float row_bcast(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + J, 0xf, 0xf, false));
}
template <int J> __device__ __forceinline__ float lpc_chain(float r, float prod)
{
    if constexpr (J < LPCN_LPC_ORDER) return lpc_chain<J + 1>(r - row_bcast<J>(prod), prod);
    else return r;
}
// value of the previous lane of the 16-lane row; lane 0 gets `fill`
__device__ __forceinline__ float row_shr1(float v, float fill)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, false));
}

// The LDS cells of one group of S streams that the leader works on
struct LeaderCells {
    float *lead;                    // [S][8] leader record: pred, deemph, last exc (i32), -, rng[4] (u32)
    int *idx;                       // [S] packed (sig, pred, exc) mu-law indices of the sample being opened, [S] live flags
    float *thr;                     // [S][8] the sample's tree thresholds
    short *pcm;                     // [S][160] the frame's PCM (teacher forcing: the caller's samples on entry)
};

// Open a sample: prediction and the three mu-law indices of the embedding gather (src/lpcnet.c:252-254), for the caller to publish.
// `prod` = this lane's term s_j*a_j of the prediction (tap j); `per_frame`: also (re)write the stream's live flag
template <int S> __device__ __forceinline__ void open_sample(const LeaderCells &c, const int tid0, const bool live, const float newest, const float prod, const int exc, const bool per_frame)
{
    int t_ = tid0;
    LPCN_REMAT_V(t_);
    const int lrow = (t_ & 63) >> 4, tap = t_ & 15;
    // pred = ((0 - s0*a0) - s1*a1) - ... in tap order (src/lpcnet.c:252): every lane of the row runs the whole chain,
    // taking product j from lane j of its row through a DPP row broadcast folded into the subtract -- the
    // broadcast operand does not depend on the chain, so the 16 steps cost only the add latency
    const float r = lpc_chain<0>(0.f, prod);
    // mu-law index of the newest sample (even taps) and of the prediction (odd taps) in one pass; tap 0 collects both
    const int u = lpcn_lin2ulaw((tap & 1) ? r : newest);
    const int u_pred = __builtin_amdgcn_mov_dpp(u, 0xB1, 0xf, 0xf, true);      // neighbour lane (quad_perm [1,0,3,2])
    if (tap == 0) {
        if (live) {
            c.lead[lrow * 8 + 0] = r;
            c.idx[lrow] = u | (u_pred << 8) | (exc << 16);     // (sig, pred, exc) indices packed into one word per stream
        } else {
            c.idx[lrow] = 0;
        }
        if (per_frame) c.idx[S + lrow] = live ? 1 : 0;
    }
}

// Threshold lane of stream `ls`: two KISS99 words become the 8 logit thresholds of the sample's tree (src/nnet.c:178-184)
__device__ __forceinline__ void draw_thresholds(const LeaderCells &c, const float *logit_tab, const int ls)
{
    int *li = (int *)c.lead + ls * 8;
    uint32_t rng[4] = {(uint32_t)li[4], (uint32_t)li[5], (uint32_t)li[6], (uint32_t)li[7]};
    const uint32_t r0 = lpcn_kiss99(rng), r1 = lpcn_kiss99(rng);
    li[4] = (int)rng[0]; li[5] = (int)rng[1]; li[6] = (int)rng[2]; li[7] = (int)rng[3];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        c.thr[ls * 8 + b] = logit_tab[(r0 >> (8 * b)) & 0xFF];
        c.thr[ls * 8 + 4 + b] = logit_tab[(r1 >> (8 * b)) & 0xFF];
    }
}

// The sampler's 8 decisions from the 255 ballot bits of one stream (mask_row: 8 u64, wave w's ballot in word w; node n = lane 2 n).
// (Tried in round 5: the walk by the row's 16 lanes in two dependent steps -- lane c tests the c-th root-to-leaf path of a 4-level
// subtree, a ballot names the lane that matched -- a third of the dependent depth, bit-exact, and slower: fp32 123.1 vs 126.3 M,
// int8 164.1 vs 170.4 M.)
__device__ __forceinline__ int tree_walk(const unsigned long long *mask_row)
{
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const u4 *mk = (const u4 *)mask_row;
    const u4 qa = mk[0], qb = mk[1], qc = mk[2], qd = mk[3];
    auto bit_of = [](unsigned word, int k) { return (int)((word >> (2 * k)) & 1u); };
    int val = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) val = (val << 1) | bit_of(qa[0], (1 << b) | val);        // nodes 1..15
    val = (val << 1) | bit_of(qa[1], val);                                               // nodes 16..31
    val = (val << 1) | bit_of((val & 16) ? qa[3] : qa[2], val & 15);                     // nodes 32..63
    {
        const int k = val >> 4;                                                          // nodes 64..127: dwords 4..7
        const unsigned lo = (k & 1) ? qb[1] : qb[0], hi = (k & 1) ? qb[3] : qb[2];
        val = (val << 1) | bit_of((k & 2) ? hi : lo, val & 15);
    }
    {
        const int k = val >> 4;                                                          // nodes 128..255: dwords 8..15
        const unsigned a0 = (k & 1) ? qc[1] : qc[0], a1 = (k & 1) ? qc[3] : qc[2];
        const unsigned a2 = (k & 1) ? qd[1] : qd[0], a3 = (k & 1) ? qd[3] : qd[2];
        const unsigned b0 = (k & 2) ? a1 : a0, b1 = (k & 2) ? a3 : a2;
        val = (val << 1) | bit_of((k & 4) ? b1 : b0, val & 15);
    }
    return val;
}

// Leader lanes, once the tree of sample `smp` of the frame has been evaluated: the excitation (walked, or forced from the caller's
// PCM while smp < preload), the sample before de-emphasis, the history shift.  Out: pcm, deemph, exc for open_sample / finish_sample.
// `walked()` returns the tree's 8 decisions; the two forms below bind it.
template <class Walked>
__device__ __forceinline__ void draw_sample_with(const LeaderCells &c, const Walked walked, const float *ulaw_tab, const int lrow, const int tap,
                                                 const bool live, const int smp, const int preload, float &hist, float &pcm, float &deemph, int &exc)
{
    pcm = 0.f; deemph = 0.f; exc = 0;
    if (live) {                                  // (all 16 lanes of a stream's row do the same walk)
        const float pred = c.lead[lrow * 8 + 0];           // (issued together with the mask reads)
        deemph = c.lead[lrow * 8 + 1];
        exc = walked();
        if (smp < preload) {                                        // src/lpcnet.c:256-258
            const float x = (float)c.pcm[lrow * LPCN_FRAME_SIZE + smp];
            exc = lpcn_lin2ulaw(x - 0.85f * deemph - pred);
            pcm = x - 0.85f * deemph;
        } else {
            pcm = pred + ulaw_tab[exc];                              // src/lpcnet.c:260
        }
    }
    {                                            // history shifts by one, the new sample enters at tap 0 (src/lpcnet.c:262-263)
        const float shifted = row_shr1(hist, pcm);
        hist = live ? shifted : hist;
    }
    if (tap == 0 && live) ((int *)c.lead)[lrow * 8 + 2] = exc;
}
// the tree as 255 ballot bits per stream (every node evaluated): the leader walks them
__device__ __forceinline__ void draw_sample(const LeaderCells &c, const unsigned long long *mask_row, const float *ulaw_tab, const int lrow, const int tap,
                                            const bool live, const int smp, const int preload, float &hist, float &pcm, float &deemph, int &exc)
{
    draw_sample_with(c, [&]() { return tree_walk(mask_row); }, ulaw_tab, lrow, tap, live, smp, preload, hist, pcm, deemph, exc);
}
// the tree already walked by the wave that evaluated it (tree_stages.h): one cell per stream holds the 8 decisions
__device__ __forceinline__ void draw_sample_walked(const LeaderCells &c, const int *walked_cell, const float *ulaw_tab, const int lrow, const int tap,
                                                   const bool live, const int smp, const int preload, float &hist, float &pcm, float &deemph, int &exc)
{
    draw_sample_with(c, [&]() { return *walked_cell & 0xFF; }, ulaw_tab, lrow, tap, live, smp, preload, hist, pcm, deemph, exc);
}
// ... and behind the next sample's indices (the other waves are waiting for those): de-emphasis and the PCM store
// (src/lpcnet.c:264-269); start-up frames produce zeros
__device__ __forceinline__ void finish_sample(const LeaderCells &c, const int lrow, const int tap, const bool live, const int smp, const int preload, float pcm, const float deemph)
{
    if (tap == 0) {
        if (live) {
            pcm = pcm + 0.85f * deemph;
            c.lead[lrow * 8 + 1] = pcm;                            // de-emphasis memory
            if (smp >= preload) c.pcm[lrow * LPCN_FRAME_SIZE + smp] = (short)lpcn_round_pcm(pcm);
        } else {
            c.pcm[lrow * LPCN_FRAME_SIZE + smp] = 0;
        }
    }
}
// whether a stream produces samples in frame f of the launch (src/lpcnet.c:239-243: the first frames only fill the feature pipeline)
__device__ __forceinline__ bool stream_is_live(const LpcnSampleArgs *Ap, const LPCN_GLOBAL lpcn_stream_state *states, const int stream, const int f)
{
    const int fc_ref = Ap->fc_base ? as_global(Ap->fc_base)[stream] : states[stream].frame_count;
    int fc = Ap->fc_advance ? fc_ref + f + 1 : fc_ref;
    if (fc > 1000) fc = 1000;
    return fc > LPCN_FEATURES_DELAY;
}

// ---- staging: launch prologue / epilogue --------------------------------------------------------
// The tables and small matrices every variant keeps in LDS; L = the kernel's LDS layout.  brec_dwords: GRU-B's recurrent matrix is
// copied bit for bit ([16][48] floats, or [48 rows] x 4 dwords of 4 int8).
template <class L> __device__ __forceinline__ void stage_tables(unsigned char *smem, const LpcnSampleArgs *Ap, const int tid, const int brec_dwords)
{
    const auto *t0 = as_global(Ap->tab_tansig), *t1 = as_global(Ap->tab_ulaw2lin), *t2 = as_global(Ap->tab_logit);
    for (int i = tid; i < 201; i += LPCN_WG_THREADS) ((float *)(smem + L::tansig))[i] = t0[i];
    for (int i = tid; i < 256; i += LPCN_WG_THREADS) {
        ((float *)(smem + L::ulaw))[i] = t1[i];
        ((float *)(smem + L::logit))[i] = t2[i];
    }
    const auto *ab1 = as_global(Ap->a_bias1), *adg = as_global(Ap->a_diag);
    for (int i = tid; i < RA; i += LPCN_WG_THREADS) {
        ((float *)(smem + L::abias))[2 * i] = ab1[i];          // [row]{bias, diag}: one 8-byte read per row
        ((float *)(smem + L::abias))[2 * i + 1] = adg[i];
    }
    const auto *br = as_global(Ap->b_rec), *bb = as_global(Ap->b_bias);
    for (int i = tid; i < brec_dwords; i += LPCN_WG_THREADS) ((uint32_t *)(smem + L::brec))[i] = ((const LPCN_GLOBAL uint32_t *)br)[i];
    for (int i = tid; i < 2 * RB; i += LPCN_WG_THREADS) ((float *)(smem + L::bbias))[i] = bb[i];
    if (tid < 7) ((int *)(smem + L::bstart))[tid] = as_global(Ap->b_start)[tid];
}
// GRU-B's float input weights, [block][8 rows][4], plus 8 blocks of padding (the chain loops read ahead).
// shifted (dense matrix, PARITY: the grub_lds_loop_s*.inc forms): a wave's weight read fetches 16 B per row from six row groups
// 12 288 B apart -- the same 32 banks for every group, a two-way conflict inside each 16-lane service group of ds_read_b128.  Row
// groups 2, 3 and 5 are shifted by one more block (128 B = the other half of the banks; LPCN_GRUB_SHIFT, one nibble per group);
// zero blocks behind the shifted last group, and the pad absorbs the shift.
#define LPCN_GRUB_SHIFT 0x321100
__device__ __forceinline__ void stage_grub_weights(unsigned char *bw, const LpcnSampleArgs *Ap, const int tid, const bool shifted)
{
    const int nb_b = Ap->nb_b;
    const auto *src = (const LPCN_GLOBAL uint32_t *)as_global(Ap->b_w);
    for (int i = tid; i < (nb_b + 8) * 32; i += LPCN_WG_THREADS) {
        int di = i;
        if (shifted) {
            if (i < nb_b * 32) di = i + ((LPCN_GRUB_SHIFT >> (4 * ((i >> 5) / 96))) & 15) * 32;
            else if (i < (nb_b + 5) * 32) di = i + 3 * 32;
            else continue;
        }
        ((uint32_t *)bw)[di] = i < nb_b * 32 ? src[i] : 0u;
    }
}
// leader record of one stream: lpcn_stream_state -> LDS, where it lives between the samples of a launch (the kernels write it back themselves)
__device__ __forceinline__ void stage_leader_record(const LeaderCells &c, const int s, const LPCN_GLOBAL lpcn_stream_state *st)
{
    c.idx[s] = 0;
    c.lead[s * 8 + 0] = 0.f;                                       // pred
    c.lead[s * 8 + 1] = st->deemph_mem;
    ((int *)c.lead)[s * 8 + 2] = st->last_exc;
#pragma unroll
    for (int j = 0; j < 4; ++j) ((uint32_t *)c.lead)[s * 8 + 4 + j] = st->rng[j];
}
}  // namespace lpcn
