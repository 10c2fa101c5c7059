// What the units of the engine's host runtime share (engine.hip, engine_synth.hip, engine_codec.hip, engine_plc.hip, engine_probe.hip): the
// error macro, the owning buffer types, the engine and batch records and the helpers more than one unit calls.  C++ only: the C host
// shell sees lpcnet_engine.h alone.  The seam between units is host functions; each kernel header belongs to one unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <type_traits>
#include <vector>
#include "lpcnet_engine.h"
#include "sample_kernel.hip.h"
#include "kernel_params.h"
#include "plc_plan.h"
#include "snapshot_plan.h"

// The calling thread's last error message (engine.hip; lpcn_last_error).  __thread: no dynamic initialiser, so every unit reaches it directly; a
// thread_local declared extern goes through the C++ wrapper and its weak init hook, whose address test fails in a shared library.
extern __attribute__((visibility("hidden"))) __thread char g_err[512];

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            snprintf(g_err, sizeof(g_err), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,      \
                     hipGetErrorString(_e));                                                  \
            return LPCN_E_HIP;                                                                \
        }                                                                                     \
    } while (0)

// Every entry point selects the engine's device and restores the caller's current device on return.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
// Device memory with an owner: the destructor frees, nothing copies.  `cap` counts elements.  What a batch owns goes with `delete b`, inside
// the DeviceGuard of lpcn_batch_dev_destroy.
struct lpcn_batch_dev;
int wait_all(lpcn_batch_dev *b);
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // exactly `count` elements, optionally zeroed
    int alloc(size_t count, bool zero = false)
    {
        release();
        if (hipMalloc((void **)&p, count * sizeof(T)) != hipSuccess) { p = nullptr; snprintf(g_err, sizeof(g_err), "hipMalloc(%zu) failed", count * sizeof(T)); return LPCN_E_HIP; }
        cap = count;
        if (zero) HIP_TRY(hipMemset(p, 0, count * sizeof(T)));
        return 0;
    }
    // at least `count` elements, contents not kept.  Growing first waits for everything enqueued for the batch, whichever stream it went to:
    // the old buffer may still be in use.  It happens once per size.
    int reserve(lpcn_batch_dev *b, size_t count)
    {
        if (count <= cap) return 0;
        const int rc = wait_all(b);
        return rc ? rc : alloc(count);
    }
};
// Pinned host memory, grown to the bytes its user asks for.  Its users synchronise before they return, so nothing is in flight when it grows.
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { p = nullptr; snprintf(g_err, sizeof(g_err), "hipHostMalloc(%zu) failed", bytes); return LPCN_E_HIP; }
        cap = bytes;
        return 0;
    }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

// GRU-A as dealt to waves and lanes, once per dealing: the model part of the argument block with that image's pointers, and the compiled
// items-per-lane variant its item arrays are padded to.  PARITY's always exists; FAST has its own for int8 blobs (dealt without candidate heads);
// the two-group kernel's (float blobs; model_pack.c: lpcn_model_pack_x2) is the only one with the natural-order embedding tables; its twelve-wave
// form runs on an image of its own (lpcn_model_pack_x3: 12 waves x 16 items, candidate slots cut head / tail) and shares those tables.
enum { IMG_PARITY, IMG_FAST, IMG_X2, IMG_X3, IMG_COUNT };
struct GruAImage { LpcnSampleArgs args{}; int nw_variant = 0; bool present = false; };

// The two-group kernel's wide image (more than 32 items per lane: the streamed variants) as dealt when the engine was created, on the host, with a
// copy of the blob's embedding tables, until a batch asks for it (lpcn_batch_dev_set_x2_streamed uploads it and drops this)
struct X2WideHost {
    lpcn_model_host mx{};
    bool packed = false;
    std::vector<float> emb[3];
    X2WideHost() = default;
    X2WideHost(const X2WideHost &) = delete;
    X2WideHost &operator=(const X2WideHost &) = delete;
    ~X2WideHost() { if (packed) lpcn_model_release(&mx); }
};

// A host copy of the arrays of a frame-rate network's layers (the blob is the caller's): take() copies every array into the two arenas and points
// the layer records at the copies.  q8: the GRUs are int8 layers, whose two weight arrays hold a byte per weight (a multiple of four)
struct LayerArena {
    std::vector<float> f;
    std::vector<int> i;
    void take(const std::vector<lpcn_dense_layer *> &dense, lpcn_gru_layer *gru, int n_gru, bool q8 = false)
    {
        size_t nf = 0, ni = 0;
        const size_t per = q8 ? 4 : 1;      // weights per float-sized cell
        std::vector<size_t> idx_len(n_gru);
        for (lpcn_dense_layer *q : dense) nf += (size_t)q->n_in * q->n_out + q->n_out;
        for (int g = 0; g < n_gru; ++g) {
            const lpcn_gru_layer &G = gru[g];
            idx_len[g] = (size_t)(3 * G.n / 8) + G.nb;
            nf += 32 * (size_t)G.nb / per + 3 * (size_t)G.n * G.n / per + 6 * (size_t)G.n;
            ni += idx_len[g];
        }
        f.resize(nf);
        i.resize(ni);
        float *fp = f.data();
        int *ip = i.data();
        auto copy = [&](const float *&src, size_t count) { memcpy(fp, src, sizeof(float) * count); src = fp; fp += count; };
        for (lpcn_dense_layer *q : dense) { copy(q->w, (size_t)q->n_in * q->n_out); copy(q->b, q->n_out); }
        for (int g = 0; g < n_gru; ++g) {
            lpcn_gru_layer &G = gru[g];
            copy(G.w, 32 * (size_t)G.nb / per); copy(G.rec, 3 * (size_t)G.n * G.n / per); copy(G.bias, 6 * (size_t)G.n);
            memcpy(ip, G.idx, sizeof(int) * idx_len[g]); G.idx = ip; ip += idx_len[g];
        }
    }
};
// The blob's DRED decoder as copied when the engine was created, on the host until a batch asks for it: lpcn_batch_dev_dred_enable uploads it and
// drops this.  `m` points into the arena.  The encoder likewise (lpcn_batch_dev_dred_enc_enable).
struct DredHostModel {
    lpcn_dred_model m{};
    LayerArena a;
};
// What the FAST flavour's image is packed from (dred_fast_pack.h): the three GRUs' sparse input matrices and their index streams, nothing else
struct DredFastHost {
    std::vector<float> w[3];
    std::vector<int> idx[3];
    int n_in[3] = {0, 0, 0}, n[3] = {0, 0, 0};
};
struct DredEncHostModel {
    lpcn_dred_enc_model m{};
    LayerArena a;
};

struct lpcn_engine {
    int device = 0;
    int nw = 0, nb_b = 0;
    bool is_int8 = false;
    bool fc_f16 = false;               // FAST sub-option: fp16 dual FC (lpcn_engine_set_fast(e, 2))
    bool fast = false;                 // FAST arithmetic (lpcn_engine_set_fast): fused / integer accumulation instead of the reference's generic-C order
    float lpc_gamma = 1.f;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    GruAImage image[IMG_COUNT];
    bool x2_wide = false;              // image[IMG_X2] is the wide image: only batches that asked for it run on it (lpcn_batch_dev::x2_streamed)
    std::unique_ptr<X2WideHost> x2w_host;         //   ... not uploaded yet
    LpcnFrameModel fmodel{};
    lpcn::DecodeTables dec{};      // codec path: VQ codebooks + pitch table (set by lpcn_engine_set_codebooks)
    bool has_codebooks = false;
    lpcn::EncodeTables enc{};      // encoder: the same codebooks and their transposed copies, refreshed together
    lpcn::PlcNet plc{};            // packet-loss concealment: the blob's PLC network, a float blob's (plc_pred_kernel) ...
    lpcn::PlcNetQ plcq{};          //   ... or an int8 blob's (plc_pred_i8_kernel)
    int plc_present = 0;           //   ... lpcn_plc_model.present of the blob
    bool plc_servable = false;     //   ... and whether it is in the blob's own flavour (lpcn_plc_servable): uploaded only then
    lpcn::DredNet dred{};          // DRED decoder (engine_dred.hip): the blob's decoder on the device, once a batch has enabled it: a float blob's ...
    lpcn::DredNetQ dredq{};        //   ... or an int8 blob's (dred_decode_i8_kernel) ...
    const lpcn::DredNet *d_dred = nullptr;        //   ... and the device copy of this block, which the kernel walks
    const lpcn::DredNetQ *d_dredq = nullptr;
    int dred_present = 0;          //   ... lpcn_dred_model.present of the blob
    bool dred_servable = false;    //   ... and whether it is in the blob's own flavour (lpcn_dred_servable)
    std::unique_ptr<DredHostModel> dred_host;     //   ... not uploaded yet
    std::unique_ptr<DredFastHost> dred_fast_host;   //   ... a float decoder's GRU input matrices, kept from the upload until the FAST image is packed from them
    const lpcn::DredFastImage *d_dred_fast = nullptr;   //   ... the FAST flavour's image of the GRU input matrices, once a batch has asked for FAST
    lpcn::DredEncNet denc{};       // DRED encoder (engine_dred_enc.hip), the same: the block of either flavour, its device copy, ...
    lpcn::DredEncNetQ dencq{};
    const lpcn::DredEncNet *d_denc = nullptr;
    const lpcn::DredEncNetQ *d_dencq = nullptr;
    int denc_present = 0;          //   ... lpcn_dred_enc_model.present of the blob, lpcn_dred_enc_servable, ...
    bool denc_servable = false;
    std::unique_ptr<DredEncHostModel> denc_host;  //   ... not uploaded yet
    std::unique_ptr<DredFastHost> denc_fast_host;   //   ... a float encoder's GRU input matrices, kept from the upload until its FAST image is packed from them
    const lpcn::DredFastImage *d_denc_fast = nullptr;   //   ... the encoder's FAST image (rdovae_enc_fast_kernel), once a batch has asked for FAST
};

// width of GRU g (0, 1) of the engine's PLC network, read from the net that was uploaded: a stream's network state is four copies of g1 + g2 floats
inline int plc_units(const lpcn_engine *e, int g) { return e->is_int8 ? e->plcq.gru[g].n : e->plc.gru[g].n; }

// ---- model upload.  A device copy of `count` elements that is freed with the engine
template <typename T>
int upload(lpcn_engine *e, const T **dst, const void *src, size_t count)
{
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, count * sizeof(T) ? count * sizeof(T) : 16));
    e->allocs.push_back(p);
    if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = (const T *)p;
    return 0;
}
// A GRU-B layer of a frame-rate network (kernel_params.h: GruLayer).  The bias as it is (`bias` -- the generic-C build never reads `subias`); the sparse
// input matrix's index stream {count, pos...} (src/vec.h:347-360) split into the first block of every 8-row group and the blocks' input positions; the
// weights per flavour.  W = float: the blob's arrays as they are.  W = int, an int8 layer: one dword per (row, block) -- the input blocks [block][8 rows]
// [4 cols] are that already, the positions become input dwords, the recurrent weights go block-major (model_pack.c: lpcn_plc_pack_rec_i8)
template <typename W>
int upload_gru(lpcn_engine *e, lpcn::GruLayer<W> &o, const lpcn_gru_layer &g)
{
    constexpr bool q8 = !std::is_same<W, float>::value;
    const int groups = 3 * g.n / 8;
    const int *idx = g.idx;
    std::vector<int> start(groups + 1, 0), pos;
    for (int r = 0; r < groups; ++r) {
        const int cnt = *idx++;
        for (int k = 0; k < cnt; ++k) pos.push_back(*idx++ >> (q8 ? 2 : 0));
        start[r + 1] = (int)pos.size();
    }
    o.n_in = g.n_in; o.n = g.n;
    int rc = 0;
    if ((rc = upload<float>(e, &o.bias, g.bias, 6 * (size_t)g.n)) || (rc = upload<int>(e, &o.start, start.data(), start.size())) ||
        (rc = upload<int>(e, &o.pos, pos.data(), pos.size()))) return rc;
    if constexpr (q8) {
        std::vector<int32_t> rec((size_t)3 * g.n * g.n / 4);
        lpcn_plc_pack_rec_i8((const signed char *)g.rec, g.n, rec.data());
        if ((rc = upload<int>(e, &o.w, g.w, (size_t)8 * g.nb))) return rc;      // (32 bytes per block)
        return upload<int>(e, &o.rec, rec.data(), rec.size());
    } else {
        if ((rc = upload<float>(e, &o.w, g.w, 32 * (size_t)g.nb))) return rc;
        return upload<float>(e, &o.rec, g.rec, 3 * (size_t)g.n * g.n);
    }
}

// packet-loss concealment of a batch (lpcn_batch_dev_plc_enable): the control state on the host, the data on the device
struct lpcn_plc_host {
    int options = 0;
    bool remove_dc = false;
    int cus = 0;                                    // the device's compute units, for the prediction kernels' form table
    int pred_form = 0;                              // records per workgroup pinned by lpcn_batch_dev_plc_pred_set_form (0: the table's choice)
    std::vector<lpcn_plc_ctl> ctl;
    DevBuf<short> q, lp;                            // the arrays of lpcn::PlcData (kernel_params.h) ...
    DevBuf<float> feat, net, fec, fbuf, burg, an;
    DevBuf<double> dc;
    DevBuf<int> delta;
    lpcn::PlcData D{};                              // ... and their addresses as the kernels take them
    DevBuf<short> d_pcm;                            // staging of the host-pointer call
    DevBuf<int> d_ident;                            // 0 .. n-1
    DevBuf<int> d_ctl;                              // the step's lists: device copy (its capacity bounds a step's lists) ...
    PinBuf h_ctl;                                   // ... and its pinned source
    Event ev_ctl;                                   // the upload of the previous step's lists has left h_ctl
    bool ctl_pending = false;
    PlcPlan plan;
    DevBuf<int> d_feed;                             // a batched FEC feed's records (their pinned source: h_ctl past the step's lists, so that a feed
    Event ev_feed;                                  //   and a step never wait for each other's upload) and "the previous feed's have left it"
    bool feed_pending = false;
    DevBuf<float> d_feed_src;                       //   ... and the host-pointer call's packed vectors, grown to the largest call
};

// DRED decoding of a batch (lpcn_batch_dev_dred_enable): the scratch of a call, and -- once lpcn_batch_dev_dred_state_enable has run -- every
// stream's decoder state for the init / step pair
struct lpcn_dred_host {
    int max_latents = 0, cus = 0;                   // (cus: the device's compute units, for the form table)
    int form = 0;                                   // streams per workgroup pinned by lpcn_batch_dev_dred_set_form (0: the table's choice)
    int fast = 0;                                   // lpcn_batch_dev_dred_set_fast: 0 PARITY, 1 FAST at the engine's tile, else FAST at that tile
    DevBuf<int> d_rec;                              // a call's per-stream records (dred_kernels.hip.h: DRED_REC) ...
    PinBuf h_rec;                                   // ... their pinned source ...
    Event ev_rec;                                   // ... and "the previous call's have left it"
    bool rec_pending = false;
    DevBuf<float> d_state, d_latents, d_feat;       // staging of the host-pointer call
    PinBuf h_feat;                                  //   ... whose output comes down whole and goes to the caller row by row (rows past a stream's count stay)
    size_t st_rec = 0;                              // floats of a stream's decoder record (dred_kernels.hip.h: dred_state_rec_floats); 0: not enabled
    DevBuf<float> st;                               // [n][st_rec]: dense2_state, dense4_state, dense6_state, padded to 16 bytes
    DevBuf<int> d_srec;                             // an init's or a step's per-stream records (DRED_SREC) ...
    PinBuf h_srec;                                  // ... their pinned source ...
    Event ev_srec;                                  // ... and "the previous call's have left it"
    bool srec_pending = false;
};

// DRED encoding of a batch (lpcn_batch_dev_dred_enc_enable): every stream's state record (rdovae_enc_kernels.hip.h) and the scratch of a call
struct lpcn_denc_host {
    int max_dframes = 0, cus = 0;                   // (cus: the device's compute units, for the form table)
    int form = 0;                                   // streams per workgroup pinned by lpcn_batch_dev_dred_enc_set_form (0: the table's choice)
    int fast = 0;                                   // lpcn_batch_dev_dred_enc_set_fast: 0 PARITY, 1 FAST at the engine's tile, else FAST at that tile
    size_t rec = 0;                                 // floats of a stream's record
    DevBuf<float> state;                            // [n][rec]: GRU states, the conv memory as a ring, the ring's head
    DevBuf<int> d_cnt;                              // a call's per-stream counts ...
    PinBuf h_cnt;                                   // ... their pinned source ...
    Event ev_cnt;                                   // ... and "the previous call's have left it"
    bool cnt_pending = false;
    DevBuf<float> d_feat, d_lat, d_init;            // staging of the host-pointer call
    PinBuf h_out;                                   //   ... whose outputs come down whole and go to the caller row by row (rows past a stream's count stay)
};

struct lpcn_batch_dev {
    lpcn_engine *e = nullptr;
    int n = 0, max_chunk = 0, S = 0, frame_len = LPCN_FRAME_SIZE;
    int active = 0;                    // the active prefix (lpcn_batch_dev_set_active; default n): every call that advances streams works on streams [0, active).
                                       //   Launch sizes and copy lengths take it; allocation sizes and range checks keep n
    bool S_auto = true;                // streams per workgroup are chosen by the engine (measured on this batch, see autotune_streams_per_wg)
    bool tuned = false;                // ... and have been measured for the current arithmetic flavour
    bool pack2 = false;                // 128-VGPR variant: two workgroups per CU (int8, <= 32 items per lane, more workgroups than CUs)
    bool no_x2 = false;                // LPCNET_HIP_NO_X2=1 when the batch was created (tools / tests): never the two-group kernel
    bool x2_streamed = false;          // lpcn_batch_dev_set_x2_streamed: this batch may run the two-group kernel's streamed variants (a wide image)
    bool x2_fast = false;              // lpcn_batch_dev_set_x2_fast: this batch may run the two-group kernel under FAST fp32 arithmetic (sample_x2f.hip)
    bool x3 = false;                   // at eight streams per workgroup: the twelve-wave form of the two-group kernel (measured faster on this batch, or asked for)
    int x3_mode = -1;                  // lpcn_batch_dev_set_x3: 0 never, 1 always, -1 measured (the table's value, the eight-wave form, until then)
    int pack2_force = -1;              // LPCNET_HIP_PACK2 when the batch was created (tools / tests): 0 never, 1 whenever the variant exists, -1 unset
    DevBuf<lpcn_stream_state> d_state;
    DevBuf<int> d_fc_base;
    DevBuf<float> d_cond_a, d_cond_b, d_lpc, d_cond;
    DevBuf<float> d_feat;              // staging for host-pointer runs / decoded feature vectors
    DevBuf<short> d_pcm;
    DevBuf<unsigned char> d_packets;   // packet staging of the host-pointer codec calls (decode: in, encode: out)
    DevBuf<float> d_vq_mem;            // [n][18] VQ memory of the codec path (src/lpcnet_private.h:52)
    DevBuf<lpcn_analysis_state> d_an_state;      // feature analysis (lpcn_batch_dev_analysis_enable): per-stream state, allocated on first use
    DevBuf<float> d_an_resid, d_an_xc, d_an_fw;  //   ... and the kernels' scratch for an_chunk frames per launch
    int an_chunk = 0;
    DevBuf<unsigned char> d_an_pcm;    //   ... and the staging of host-pointer calls (PCM in, as bytes; features out)
    DevBuf<float> d_an_feat;
    DevBuf<float> d_enc_vq_mem;        // encoder (lpcn_batch_dev_encoder_enable): [n][18] vq_mem of LPCNetEncState, beside the analysis state
    DevBuf<float> d_enc_feat, d_enc_qf3;         //   ... scratch of enc_chunk packets per launch: cepstrum / LPC rows, quantised frame 3 (+ the entry vq_mem)
    DevBuf<int> d_enc_pk;              //   ... and the packets' bit fields
    int enc_chunk = 0;
    DevBuf<lpcn_stream_state> d_state_tmp;       // compacted groups (run_group: the per-stream-arguments step, the PLC): the group's states
    DevBuf<float> d_gfeat;             //   ... features (also the PLC parity seam's output)
    DevBuf<short> d_gpcm;              //   ... and PCM
    DevBuf<int> d_map;                 //   ... the index maps of one lpcn_batch_dev_step_host call (the PLC's are part of its control lists)
    DevBuf<float> d_keep_a, d_keep_b, d_keep_lpc;   //   ... and every stream's most recent frame products
    std::vector<char> keep_ok;         //   ... which exist only for streams whose last frame step went through the step call (mode 1)
    DevBuf<LpcnSampleArgs> d_args;     // one record per sample launch of a step (a whole-batch launch uses record 0) ...
    int args_next = 0;                 //   ... and the next free one of the step being enqueued
    // the group schedule (lpcn_batch_dev_set_group_schedule; default off: every group launches in the batch's form, on the caller's stream)
    int sched_form = 0, sched_lanes = 1;
    Stream side[PLC_MAX_LANES - 1];    // lanes 1 .. 3: created when the schedule is first set with more than one lane
    Event ev_fork, ev_join[PLC_MAX_LANES - 1];
    struct GroupRec { int v[8]; };     // {lane, slot, cnt, kind, N, preload, streams per workgroup, workgroups}
    std::vector<GroupRec> last_groups; // the groups of the most recent PLC step / per-stream step
    DevBuf<float> d_dbg;
    DevBuf<unsigned long long> d_prof;
    Event ev[3];
    // Ordering across caller streams: the batch's scratch buffers and state are shared by every call, so each enqueue
    // records ev_last on its stream; a call on a DIFFERENT stream first waits for it, and every host-side access
    // (sync, state get/set, reset, destroy, buffer growth) waits for it as well.
    Event ev_last;
    hipStream_t last_stream = nullptr;
    bool pending = false;
    DevBuf<int> d_pairs;               // lpcn_batch_dev_copy_streams (engine_roster.hip): the (src, dst) list of a call, or a snapshot's streams and meta rows, [11 n] ...
    PinBuf h_pairs;                    //   ... its pinned source ...
    Event ev_pairs;                    //   ... and "the previous call's list has left it"
    bool pairs_pending = false;
    DevBuf<char> d_snap;               // stream snapshots (engine_snapshot.hip): the records of a host-form call or of a copy to another batch, grown to the largest ...
    PinBuf h_snap;                     //   ... their pinned copy (host forms; the bounce between devices that cannot reach each other) ...
    std::vector<int> snap_meta;        //   ... the meta rows of a copy to another batch ...
    std::vector<unsigned char> snap_mark;         //   ... and one mark per stream for the check of a list
    std::unique_ptr<lpcn_plc_host> plc;           // packet-loss concealment (lpcn_batch_dev_plc_enable): host control state and device data
    std::unique_ptr<lpcn_dred_host> dred;         // DRED decoding (lpcn_batch_dev_dred_enable)
    std::unique_ptr<lpcn_denc_host> denc;         // DRED encoding (lpcn_batch_dev_dred_enc_enable)
    PinBuf h_pin;                      // pinned host staging of the single-stream fast path and the combined pass: each reserves what it lays out
    bool timing = false;
    float ms_sample = 0.f, ms_frame = 0.f;
};

// engine_roster.hip, engine_snapshot.hip: every per-stream array of the batch that is allocated now, as (base, bytes per stream).  `fn(buffer, elements per stream)`.
template <typename F>
void each_stream_array(lpcn_batch_dev *b, F fn)
{
    fn(b->d_state, (size_t)1);
    fn(b->d_vq_mem, (size_t)LPCN_NB_BANDS);
    if (b->d_an_state) fn(b->d_an_state, (size_t)1);
    if (b->d_enc_vq_mem) fn(b->d_enc_vq_mem, (size_t)LPCN_NB_BANDS);
    if (b->d_keep_lpc) { fn(b->d_keep_a, (size_t)LPCN_ROWS_A); fn(b->d_keep_b, (size_t)LPCN_ROWS_B); fn(b->d_keep_lpc, (size_t)LPCN_LPC_ORDER); }
    if (lpcn_plc_host *p = b->plc.get()) {
        fn(p->q, (size_t)LPCN_PLC_QUEUE); fn(p->feat, (size_t)LPCN_NB_FEAT); fn(p->net, 4 * (size_t)(plc_units(b->e, 0) + plc_units(b->e, 1))); fn(p->dc, (size_t)2);
        fn(p->delta, (size_t)1); fn(p->fec, (size_t)LPCN_PLC_MAX_FEC * LPCN_NB_FEAT); fn(p->fbuf, (size_t)LPCN_PLC_FBUF * LPCN_NB_FEAT);
        fn(p->lp, (size_t)LPCN_FRAME_SIZE); fn(p->burg, (size_t)2 * LPCN_NB_BANDS); fn(p->an, (size_t)LPCN_AN_NB_FEATURES);
    }
    if (lpcn_denc_host *p = b->denc.get()) fn(p->state, p->rec);
    if (lpcn_dred_host *p = b->dred.get()) if (p->st) fn(p->st, p->st_rec);
}
int stream_list_buffers(lpcn_batch_dev *b);      // engine_roster.hip: d_pairs / h_pairs / ev_pairs, on first use

// What a launch works on and the batch does not own for good: a call on part of the batch, on other states or with another S passes another
// shape; nothing overwrites the batch's settings to steer a launch.
struct LaunchShape {
    int n, frame_len;                  // streams in this launch, samples per frame
    lpcn_stream_state *d_state;        // [n] the states it reads and writes
    int S;                             // streams per workgroup asked for (plan_sample() decides what the launch gets)
    bool pack2;                        //   ... and use_pack2() for that S
    bool x3 = false;                   //   ... at eight: the twelve-wave form of the two-group kernel
    int slot = 0;                      // first row of the per-stream scratch arrays (frame products, conditioning, frame counts) the launch works in
    int arg = 0;                       // its record of d_args
};

// Which sample kernel a launch of n_frames frames per stream gets, on which GRU-A image.  No side effects.
struct SamplePlan {
    int S;                             // streams per workgroup the launch runs with
    bool pack2;
    bool x3;                           // eight streams per workgroup on twelve waves
    const GruAImage *image;            // (with its items-per-lane variant)
    int lds, grid;                     // dynamic LDS bytes per workgroup, workgroups
};
SamplePlan plan_sample(const lpcn_batch_dev *b, const LaunchShape &sh, int n_frames);

// The GRU-A image a launch at S streams per workgroup runs on: the two-group kernel's at eight; else FAST's own where the engine's
// current arithmetic is FAST and it has one; else PARITY's.
inline const GruAImage &gru_a_image(const lpcn_engine *e, int S) { return e->image[S == 8 ? IMG_X2 : (e->fast && e->image[IMG_FAST].present) ? IMG_FAST : IMG_PARITY]; }
// Two groups of four float streams per workgroup, half a step apart (sample_kernel_x2.hip.h): float blobs, PARITY arithmetic, dense GRU-B input
// matrix, <= 32 items per lane -- or up to 96 on its streamed variants, for the batches that opted in.  Eight streams per workgroup select it.
// FAST fp32 arithmetic (not its fp16 dual FC) has the kernel too, on the ordinary image only and for the batches that opted in (x2_fast).
inline bool x2_fast_servable(const lpcn_engine *e) { return !e->is_int8 && e->image[IMG_X2].present && !e->x2_wide; }      // (the register-resident variants)
inline bool x2_fast_active(const lpcn_batch_dev *b) { return b->x2_fast && b->e->fast && !b->e->fc_f16 && !b->e->x2_wide; }
inline bool x2_available(const lpcn_batch_dev *b) { return !b->no_x2 && b->e->image[IMG_X2].present && (!b->e->fast || x2_fast_active(b)) && (!b->e->x2_wide || b->x2_streamed); }
// ... and its twelve-wave form (sample_kernel_x3.hip.h), where the model has the image for it; never under FAST
inline bool x3_available(const lpcn_batch_dev *b) { return x2_available(b) && !b->e->fast && b->e->image[IMG_X3].present; }

// engine.hip: ordering across caller streams, argument checks, the cost table
bool stream_is_capturing(hipStream_t st);
int order_begin(lpcn_batch_dev *b, hipStream_t st);
int order_end(lpcn_batch_dev *b, hipStream_t st);
void forget_keep(lpcn_batch_dev *b);           // the ACTIVE streams' kept frame products are stale (a call advanced them) ...
void forget_keep_all(lpcn_batch_dev *b);       // ... every stream's (a maintenance call rewrote states)
int check_range(const lpcn_batch_dev *b, int first, int count, const char *what);
int device_cus(const lpcn_engine *e);
bool use_pack2(const lpcn_batch_dev *b, int n, int S);
int auto_streams_per_wg(const lpcn_batch_dev *b, int n);
// engine_synth.hip: staging, the tuner, the sample and frame launches (frame_kernels.hip.h)
int ensure_staging(lpcn_batch_dev *b, size_t feat_floats, size_t pcm_samples);
int tune_if_due(lpcn_batch_dev *b, hipStream_t st);
int launch_sample(lpcn_batch_dev *b, const LaunchShape &sh, hipStream_t st, short *d_pcm, size_t pcm_stride, int n_frames, int preload, bool fc_from_frames);
int launch_frames(lpcn_batch_dev *b, const LaunchShape &sh, hipStream_t st, const float *d_feat, int feat_stride, size_t feat_stream_stride, int n_frames);
int lpcn_launch_frame_kernels(const LpcnFrameModel &M, hipStream_t st, int n, int n_frames, const float *d_feat,
                              int feat_stride, size_t feat_stream_stride, lpcn_stream_state *d_state, int *d_fc_base,
                              float *d_cond, float *d_cond_a, float *d_cond_b, float *d_lpc, char *err, size_t errlen);
// engine_plc.hip: the buffers of the compacted groups, with every stream's kept frame products
int group_alloc(lpcn_batch_dev *b);
// engine_dred.hip: the host copy of the blob's DRED decoder, taken when the engine is created
int dred_engine_init(lpcn_engine *e, const lpcn_model_host *m);
// engine_dred.hip: a FAST image packed from `F` (dred_fast_pack.h) and uploaded; `what` names the half in the messages ("DRED FAST", "DRED encoder FAST")
int dred_fast_image_upload(lpcn_engine *e, const DredFastHost &F, const lpcn::DredFastImage **dst, const char *what);
int dred_state_reset(lpcn_batch_dev *b, int first, int count);      // engine_dred.hip: the decoder's per-stream records of a range, zeroed (lpcn_batch_dev_reset)
// engine_dred_enc.hip: the same for the blob's DRED encoder
int denc_engine_init(lpcn_engine *e, const lpcn_model_host *m);
// engine_codec.hip (analysis_kernels.hip.h, encode_kernels.hip.h)
int lpcn_launch_analysis_kernels(const LpcnFrameModel &M, hipStream_t st, int n, int n_frames, const void *d_pcm, int is_float,
                                 size_t pcm_stream_stride, lpcn_analysis_state *d_state, float *d_feat, int feat_stride,
                                 size_t feat_stream_stride, float *d_resid, float *d_xc, float *d_fw, char *err, size_t errlen);
int lpcn_launch_encode_kernels(const LpcnFrameModel &M, const lpcn::EncodeTables &T, hipStream_t st, int n, int n_packets, const short *d_pcm,
                               size_t pcm_stream_stride, lpcn_analysis_state *d_state, float *d_feat, int feat_stride, size_t feat_stream_stride,
                               float *d_resid, float *d_xc, float *d_fw, float *d_vq_mem, float *d_qf3, int *d_pk, unsigned char *d_packets,
                               int packets_per_stream, char *err, size_t errlen);

// One stream's record of a per-stream device array, `per` elements at buf + s * per, to the host (down) or from it (up), after everything
// enqueued for the batch.  An array that exists only once its feature is enabled names the call that makes it.
template <typename T>
int stream_rec(lpcn_batch_dev *b, int s, const DevBuf<T> &buf, size_t per, void *down, const void *up, int (*enable)(lpcn_batch_dev *, int) = nullptr)
{
    if (s < 0 || s >= b->n || (!down && !up)) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    int rc = (!buf && enable) ? enable(b, 1) : 0;
    if (!rc) rc = wait_all(b);
    if (rc) return rc;
    if (up) HIP_TRY(hipMemcpy(buf + (size_t)s * per, up, sizeof(T) * per, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy(down, buf + (size_t)s * per, sizeof(T) * per, hipMemcpyDeviceToHost));
    return 0;
}
