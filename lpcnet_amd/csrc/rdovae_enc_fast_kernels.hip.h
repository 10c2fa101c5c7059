// The DRED encoder's FAST flavour (lpcnet_batch_dred_enc_set_fast): the same network as rdovae_enc_kernel in the arithmetic of the
// reference's AVX2+FMA float build, with the streams of a workgroup on the column index of an fp32 MFMA -- the tile machinery of the decoder's FAST
// kernel (dred_fast_kernels.hip.h: DredFastAcc, dred_fast_chain, dred_fast_dense, the activations), used as it is.
//
// Arithmetic.  Every sum is ONE fma chain from its bias in ascending input order: a dense row from bias[i] over j ascending; a GRU's input part from
// bias[i] over the row group's blocks in list order, its recurrent part from bias[3 N + i] over j ascending; bits_dense from bias[i] over the whole
// window ascending -- the oldest tap first, this double frame's buffer last, the layers' outputs in the order they are appended; gdense1 over the buffer
// in append order.  The MFMAs are that chain with one rounding per step; no sum is split over k.
//
// Layout.  A workgroup carries T streams through the double frames of a call on twelve waves.  Waves 0..7 are the layer waves of the decoder's kernel:
// each owns one 32-row tile of the current layer, a GRU wave the z, r and h rows of its 32 units.  Waves 8..11 are the trailing waves: they own the
// accumulators of bits_dense (latent_dim rows) and gdense1 (gd1 rows), up to three 32-row tiles a wave -- tile c = w + 4 s of the list [bits_dense's
// tiles | gdense1's tiles] in slot s of trailing wave w, so a bits_dense tile is always a wave's slot 0.  LDS holds the three GRU states, ONE
// activation buffer, gdense1's output and one staging chunk per bits_dense wave, all [k][T].  The concatenated buffer of the PARITY kernel does not
// exist: a layer's output goes to the accumulators of the trailing waves while the layer waves compute the next layer, and to the stream's ring slot
// straight from the registers of the wave that computed it.
//
// The ring.  A double frame begins with bits_dense over the taps - 1 earlier buffers.  They lie in global memory as [slot][j] per stream, the records
// about 18 KB apart: read as a B operand directly, every lane would touch a cache line of its own at every step.  A trailing wave that owns a
// bits_dense tile stages them through its own LDS chunk instead: ENC_FAST_STAGE floats at a time, every load instruction taking 8 consecutive j of 8
// streams (a 32-byte sector per stream, so a stream's cache line is fetched whole over four instructions and nothing of it is fetched twice), every
// LDS store 8 lanes deep on a bank (bank = stream: the B operand's layout fixes that, and the loads' coalescing is bought with it).  The chunk is
// private to the wave -- no workgroup barrier orders it, the wave's own LDS operations are in order -- and the next chunk's loads are in flight, in
// registers, while the MFMAs run over the present one.  Each bits_dense wave stages for itself: up to three times the loads, all but the first from
// L2, for a ring part that meets no barrier.
// The ring part runs before the first barrier of the layer walk: beside the input's load and beside nothing else.  It cannot run beside the stack
// without a second activation buffer, because the chain must have passed the ring before it takes layer 0's output, and that output lives in the one
// activation buffer only until layer 2 writes.  (DESIGN.md §4.7a has the arithmetic of what that costs.)
// The buffer goes to the ring from registers: an accumulator lane holds four consecutive rows of one stream, which are four consecutive floats of the
// slot -- a 16-byte run per lane, no LDS read at stride T.  Every ring read of a double frame is through before the layer walk's first write (the
// bits_dense waves arrive at the barrier in front of it only then), so the slot of the oldest tap is free to be overwritten layer by layer.
//
// A stream's column never meets another's: its bits do not depend on the tile size, on the streams that share its tile and their counts, on the active
// prefix, on the shards or on how a run of double frames is cut into calls.  The record is the PARITY kernel's (rdovae_enc_rec_floats): GRU states read
// at the start of a call and written at the end, the buffer into the head slot, the head moved.
#pragma once
#include "dred_fast_kernels.hip.h"
#include "rdovae_enc_kernels.hip.h"      // rdovae_enc_rec_floats, RDOVAE_ENC_IN

namespace lpcn {

constexpr int ENC_FAST_LAYER_WAVES = DRED_FAST_LAYER_WAVES;            // one 32-row tile each: the widest layer has 256 rows (per gate)
constexpr int ENC_FAST_TRAIL_WAVES = 4, ENC_FAST_SLOTS = 3;            // 12 tiles: bits_dense's (up to 4) and gdense1's (up to 8)
constexpr int ENC_FAST_THREADS = 64 * (ENC_FAST_LAYER_WAVES + ENC_FAST_TRAIL_WAVES);      // twelve waves, three per SIMD
constexpr int ENC_FAST_STAGE = 1024;                                   // floats of a trailing wave's staging chunk: 1024 / T rows of the ring, 16 per lane

// floats of dynamic LDS: the three GRU states, the activation buffer (the widest of the input and the dense layers), gdense1's output -- in whole tiles
// of 32 rows like the decoder's -- and the bits_dense waves' staging chunks
__host__ __device__ inline int rdovae_enc_fast_act_rows(const DredEncNet &P)
{
    int m = RDOVAE_ENC_IN;
    for (int k = 0; k < 8; ++k) if (!P.step[k].gru && P.step[k].n_out > m) m = P.step[k].n_out;
    return m;
}
__host__ __device__ inline int rdovae_enc_fast_lds_floats(const DredEncNet &P, int T)
{
    return T * (dred_fast_pad(P.gru_n[0]) + dred_fast_pad(P.gru_n[1]) + dred_fast_pad(P.gru_n[2]) + dred_fast_pad(rdovae_enc_fast_act_rows(P)) + dred_fast_pad(P.gd1)) +
           (P.latent_dim + 31) / 32 * ENC_FAST_STAGE;      // (one chunk per trailing wave that owns a tile of bits_dense)
}
// what the tile assignment holds: bits_dense's tiles in slot 0 of a trailing wave each, every tile in some slot
__host__ __device__ inline bool rdovae_enc_fast_tiles_fit(const DredEncNet &P)
{
    const int nb = (P.latent_dim + 31) / 32, ng = (P.gd1 + 31) / 32;
    return nb <= ENC_FAST_TRAIL_WAVES && nb + ng <= ENC_FAST_TRAIL_WAVES * ENC_FAST_SLOTS;
}

// Workgroup w encodes streams [w T, w T + T) of the n active ones; arguments as rdovae_enc_kernel's, plus the GRUs' packed input matrices.
// U: steps whose weights are in flight per wave
template <int T, int U>
__global__ __launch_bounds__(ENC_FAST_THREADS) void rdovae_enc_fast_kernel(const DredEncNet *P, const DredFastImage *img, int n, int max_dframes, const int *count,
                                                                            int uniform, const float *features, int stride, float *state, float *latents, float *initial)
{
    static_assert(T == 32 || T == 16, "32 streams on the 32x32x2 MFMA, 16 on the 16x16x4");
    using Acc = DredFastAcc<T>;
    constexpr int KS = 64 / T, NJ = Acc::NJ, NE = Acc::NE;
    constexpr int CH = ENC_FAST_STAGE / T;      // rows of a staging chunk
    extern __shared__ float4 rdovae_enc_fast_lds[];
    __shared__ int cnt[T], head0[T];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, col = lane % T;
    // (the block's fields are read where they are used, not kept: the chains' loops need the scalar registers)
    const int rec = rdovae_enc_rec_floats(*P);
    float *const h0 = (float *)rdovae_enc_fast_lds, *const h1 = h0 + T * dred_fast_pad(P->gru_n[0]), *const h2 = h1 + T * dred_fast_pad(P->gru_n[1]);
    float *const act = h2 + T * dred_fast_pad(P->gru_n[2]);
    float *const g1 = act + T * dred_fast_pad(rdovae_enc_fast_act_rows(*P));
    float *const stage = g1 + T * dred_fast_pad(P->gd1);
    const auto h = [&](int g) { return g == 0 ? h0 : g == 1 ? h1 : h2; };
    const int s0 = blockIdx.x * T;
    if (t < T) {
        const int c = s0 + t < n ? (count ? count[s0 + t] : uniform) : 0;
        cnt[t] = c;
        head0[t] = c > 0 ? ((const int *)(state + (size_t)(s0 + t) * rec))[rec - 1] : 0;
    }
    __syncthreads();
    int maxc = 0;
    for (int a = 0; a < T; ++a) maxc = cnt[a] > maxc ? cnt[a] : maxc;
    if (maxc == 0) return;                  // (the whole workgroup)
    const int my_cnt = cnt[col];
    float *const my_rec = state + (size_t)(s0 + (my_cnt > 0 ? col : 0)) * rec;      // (a stream without a count is never written: its pointer only stays in bounds)
    const int my_head0 = head0[col];
    const bool layer_wave = wave < ENC_FAST_LAYER_WAVES;
    const int i0 = 32 * wave;

    // the GRU states out of the records
    for (int g = 0, at = 0; g < 3; at += P->gru_n[g], ++g) {
        const int N = P->gru_n[g];
        for (int e = t; e < T * N; e += ENC_FAST_THREADS) {
            const int j = e / T, a = e % T;
            h(g)[e] = cnt[a] > 0 ? state[(size_t)(s0 + a) * rec + at + j] : 0.f;
        }
    }
    // double frame l of every stream into the activation buffer, by the whole workgroup.  The barrier also stands behind the GRU states' load (l = 0)
    // and behind the last reader of the previous double frame's activation buffer
    const auto load_input = [&](int l) {
        int tl = t;                         // (opaque: the addresses of a double frame's loads are formed per double frame, not held in registers)
        asm volatile("" : "+v"(tl));
        for (int e = tl; e < T * RDOVAE_ENC_IN; e += ENC_FAST_THREADS) {
            const int j = e / T, a = e % T;
            act[e] = l < cnt[a] ? features[((size_t)(s0 + a) * 2 * max_dframes + 2 * l + j / LPCN_NB_FEAT) * stride + j % LPCN_NB_FEAT] : 0.f;
        }
        __syncthreads();
    };
    // The two roles run the double-frame loop apart, so that neither holds the other's addresses in registers.  They meet at the same barriers, and
    // the counts on the two sides are kept equal by hand.  Per double frame, on BOTH roles: ONE in load_input, TWO per layer (16 in all), ONE after
    // gdense1's output is written: 18.  Behind the loop, on both roles: ONE in front of the states' write-back.  A barrier added or dropped on one side
    // alone hangs the workgroup.
    if (layer_wave) {
        // dred_rdovae_encode_dframe (src/dred_rdovae_enc.c:52-84): dense 1, GRU 2, dense 3, GRU 4, dense 5, GRU 6, dense 7, dense 8.  Step k: compute
        // layer k, barrier (every reader of what it overwrites is through), write -- to LDS and to the ring slot -- barrier
#pragma unroll 1
        for (int l = 0; l < maxc; ++l) {
            load_input(l);                  // (1 barrier)
            int off = 0;                    // of layer k in the buffer
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
                __syncthreads();            // (2 k + 1) every reader of what layer k overwrites is through -- and, k = 0, every ring read of this double frame
                if (mine) {
                    const bool live = l < my_cnt;
                    // a stream past its count keeps its GRU state (a dense layer's output of it is read by its own column alone)
                    if (live || !q->gru) {
#pragma unroll
                        for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) out[(i0 + dred_fast_row<T>(e, r0)) * T + col] = res.get(e);
                    }
                    // compute_conv1d's shift of its memory (src/nnet.c:468-469): this buffer replaces the oldest tap.  Runs of four rows per lane
                    const int ring = P->taps - 1;
                    if (live && ring > 0) {
                        int slot = my_head0 + l % ring;
                        slot = slot >= ring ? slot - ring : slot;
                        float *dst = my_rec + P->gru_floats + (size_t)slot * P->total + off;
#pragma unroll
                        for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) {
                            const int i = i0 + dred_fast_row<T>(e, r0);
                            if (i < n_out) dst[i] = res.get(e);
                        }
                    }
                }
                __syncthreads();            // (2 k + 2) layer k's output is written
                off += n_out;
            }
            __syncthreads();                // (18) gdense1's output is written (the trailing waves'), and bits_dense and gdense1 have read layer 8's
        }
        __syncthreads();                    // (behind the loop) the states' write-back follows
    } else {
        // the wave among the trailing ones, opaque at every use: what a step derives from it -- the slots' tiles, their matrices -- is formed where
        // it is used, not hoisted out of the loops and held in scalar registers all along
        const auto trail = [&] { int w = wave - ENC_FAST_LAYER_WAVES; asm volatile("" : "+s"(w)); return w; };
        // a slot's tile c = tw + 4 s of the list: of bits_dense (c < nb) or of gdense1, or none
        const auto slot_bits = [&](int tw, int s) { return tw + ENC_FAST_TRAIL_WAVES * s < (P->latent_dim + 31) / 32; };
        const auto slot_rows = [&](int tw, int s) {
            const int c = tw + ENC_FAST_TRAIL_WAVES * s, nb = (P->latent_dim + 31) / 32, ng = (P->gd1 + 31) / 32;
            return c < nb ? P->latent_dim : c < nb + ng ? P->gd1 : 0;
        };
        const auto slot_i0 = [&](int tw, int s) { const int c = tw + ENC_FAST_TRAIL_WAVES * s, nb = (P->latent_dim + 31) / 32; return 32 * (c < nb ? c : c - nb); };
#pragma unroll 1
        for (int l = 0; l < maxc; ++l) {
            load_input(l);                  // (1 barrier)
            Acc acc[ENC_FAST_SLOTS] = {};
            bool begun = false;             // slot 0's chain has left its bias
            if (slot_bits(trail(), 0) && P->taps > 1) {
                const int tw = trail(), ring = P->taps - 1, total = P->total, gruf = P->gru_floats, latent_dim = P->latent_dim;
                float *const chunk = stage + tw * ENC_FAST_STAGE;
                // bits_dense over the ring, the oldest tap first: chunk by chunk through this wave's staging buffer.  Element 64 i + lane of a chunk's
                // loads: 8 consecutive j (lane % 8) of 8 streams (lane / 8), stream group i % (T / 8), j group i / (T / 8)
                float nxt[ENC_FAST_STAGE / 64];
                const int per_tap = (total + CH - 1) / CH, chunks = ring * per_tap;
                const auto fetch = [&](int c) {
                    const int tap = c / per_tap, j0 = (c - tap * per_tap) * CH;
#pragma unroll
                    for (int i = 0; i < ENC_FAST_STAGE / 64; ++i) {
                        const int a = 8 * (i % (T / 8)) + lane / 8, j = j0 + 8 * (i / (T / 8)) + lane % 8;
                        int slot = head0[a] + (l + tap) % ring;
                        slot = slot >= ring ? slot - ring : slot;
                        const bool ok = l < cnt[a] && j < total;
                        const float *src = state + (size_t)(s0 + (ok ? a : 0)) * rec + gruf + (size_t)slot * total + (ok ? j : 0);
                        nxt[i] = ok ? *src : 0.f;
                    }
                };
                fetch(0);
#pragma unroll 1
                for (int c = 0; c < chunks; ++c) {
#pragma unroll
                    for (int i = 0; i < ENC_FAST_STAGE / 64; ++i) {
                        const int a = 8 * (i % (T / 8)) + lane / 8, jj = 8 * (i / (T / 8)) + lane % 8;
                        chunk[jj * T + a] = nxt[i];
                    }
                    if (c + 1 < chunks) fetch(c + 1);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const int tap = c / per_tap, j0 = (c - tap * per_tap) * CH, rows = min(CH, total - j0);
                    acc[0] = dred_fast_dense<T, U>(begun ? nullptr : P->bits_b, acc[0], P->bits_w + ((size_t)tap * total + j0) * latent_dim, latent_dim, 32 * tw, latent_dim,
                                                   rows, chunk);
                    begun = true;
                    __builtin_amdgcn_wave_barrier();        // (the next chunk's stores follow the chain's reads)
                }
            }
            int off = 0;                    // of layer k in the buffer
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                __syncthreads();            // (2 k + 1)
                __syncthreads();            // (2 k + 2) layer k's output is written
                const DredStep *q = &P->step[k];
                const float *x = q->gru ? h(k >> 1) : act;
#pragma unroll
                for (int s = 0; s < ENC_FAST_SLOTS; ++s) {
                    const int tw = trail(), rows = slot_rows(tw, s);
                    if (!rows) continue;
                    const bool bits = slot_bits(tw, s);
                    const float *w = bits ? P->bits_w + ((size_t)(P->taps - 1) * P->total + off) * rows : P->step[8].w + (size_t)off * rows;
                    const float *b = bits ? (begun ? nullptr : P->bits_b) : (k ? nullptr : P->step[8].b);
                    acc[s] = dred_fast_dense<T, U>(b, acc[s], w, rows, slot_i0(tw, s), rows, q->n_out, x);
                }
                begun = true;
                off += q->n_out;
            }
            // the latents straight from the accumulators, gdense1's output (tanh) to LDS
#pragma unroll
            for (int s = 0; s < ENC_FAST_SLOTS; ++s) {
                const int tw = trail(), rows = slot_rows(tw, s);
                if (!rows) continue;
                const int r0 = dred_fast_row0<T>(), ti0 = slot_i0(tw, s);
                if (slot_bits(tw, s)) {
                    if (l < my_cnt) {
                        float *dst = latents + ((size_t)(s0 + col) * max_dframes + l) * rows;
#pragma unroll
                        for (int e = 0; e < NE; ++e) {
                            const int i = ti0 + dred_fast_row<T>(e, r0);
                            if (i < rows) dst[i] = acc[s].get(e);
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < NE; ++e) g1[(ti0 + dred_fast_row<T>(e, r0)) * T + col] = dred_fast_tanh(acc[s].get(e));
                }
            }
            __syncthreads();                // (18) gdense1's output is written
            // gdense2 straight to the output (src/dred_rdovae_enc.c:93): tiles tw and tw + 4 of its rows.  The next write of g1 is this role's own,
            // behind the next double frame's barriers
#pragma unroll 1
            for (int ti = 32 * trail(), state_dim = P->state_dim; ti < state_dim; ti += 32 * ENC_FAST_TRAIL_WAVES) {
                const Acc o = dred_fast_dense<T, U>(P->g2_b, Acc{}, P->g2_w, state_dim, ti, state_dim, P->gd1, g1);
                if (l < my_cnt) {
                    float *dst = initial + ((size_t)(s0 + col) * max_dframes + l) * state_dim;
#pragma unroll
                    for (int e = 0, r0 = dred_fast_row0<T>(); e < NE; ++e) {
                        const int i = ti + dred_fast_row<T>(e, r0);
                        if (i < state_dim) dst[i] = dred_fast_tanh(o.get(e));
                    }
                }
            }
        }
        __syncthreads();                    // (behind the loop) the states' write-back follows
    }
    // the GRU states back into the records, and the heads moved by the streams' counts
    for (int g = 0, at = 0; g < 3; at += P->gru_n[g], ++g) {
        const int N = P->gru_n[g];
        for (int e = t; e < T * N; e += ENC_FAST_THREADS) {
            const int j = e / T, a = e % T;
            if (cnt[a] > 0) state[(size_t)(s0 + a) * rec + at + j] = h(g)[e];
        }
    }
    if (t < T && cnt[t] > 0 && P->taps > 1) ((int *)(state + (size_t)(s0 + t) * rec))[rec - 1] = (head0[t] + cnt[t]) % (P->taps - 1);
}

}  // namespace lpcn
