// Device runtime of the LPCNet HIP engine: model upload, per-batch device buffers, kernel launches.
// Only the C ABI of lpcnet_engine.h is visible to the C host shell.
// Device and pinned memory is held by owning types (DevBuf, PinBuf): a buffer is freed when its owner goes and grows in one place
// (DevBuf::reserve, which first waits for the batch's enqueued work).  Kernels and launch helpers take raw pointers, filled from the owners.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "lpcnet_engine.h"
#include "lpcnet_tables_gen.h"
#include "sample_variants.h"
#include "sample_kernel.hip.h"
#include "frame_kernels.hip.h"
#include "decode_kernel.hip.h"
#include "analysis_kernels.hip.h"
#include "encode_kernels.hip.h"
#include "plc_kernels.hip.h"
#include "plc_plan.h"
#include <math.h>

static thread_local char g_err[512] = "";
extern "C" const char *lpcn_last_error(void) { return g_err; }

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
static int wait_all(lpcn_batch_dev *b);
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
    LpcnFrameModel fmodel{};
    lpcn::DecodeTables dec{};      // codec path: VQ codebooks + pitch table (set by lpcn_engine_set_codebooks)
    bool has_codebooks = false;
    lpcn::EncodeTables enc{};      // encoder: the same codebooks and their transposed copies, refreshed together
    lpcn::PlcNet plc{};            // packet-loss concealment: the blob's PLC network (float blobs; int8 blobs: its widths only)
    lpcn::PlcNetQ plcq{};          //   ... an int8 blob's (plc_pred_i8_kernel)
    int plc_present = 0;           //   ... lpcn_plc_model.present of the blob
    bool plc_servable = false;     //   ... and whether it is in the blob's own flavour (lpcn_plc_servable): uploaded only then
};

// packet-loss concealment of a batch (lpcn_batch_dev_plc_enable): the control state on the host, the data on the device
struct lpcn_plc_host {
    int options = 0;
    bool remove_dc = false;
    std::vector<lpcn_plc_ctl> ctl;
    DevBuf<short> q, lp;                            // the arrays of lpcn::PlcData (plc_kernels.hip.h) ...
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

struct lpcn_batch_dev {
    lpcn_engine *e = nullptr;
    int n = 0, max_chunk = 0, S = 0, frame_len = LPCN_FRAME_SIZE;
    bool S_auto = true;                // streams per workgroup are chosen by the engine (measured on this batch, see autotune_streams_per_wg)
    bool tuned = false;                // ... and have been measured for the current arithmetic flavour
    bool pack2 = false;                // 128-VGPR variant: two workgroups per CU (int8, <= 32 items per lane, more workgroups than CUs)
    bool no_x2 = false;                // LPCNET_HIP_NO_X2=1 when the batch was created (tools / tests): never the two-group kernel
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
    std::unique_ptr<lpcn_plc_host> plc;           // packet-loss concealment (lpcn_batch_dev_plc_enable): host control state and device data
    PinBuf h_pin;                      // pinned host staging of the single-stream fast path and the combined pass: each reserves what it lays out
    bool timing = false;
    float ms_sample = 0.f, ms_frame = 0.f;
};

// HIP-graph capture: a captured copy node re-reads its HOST source at every replay, so the argument block of a captured launch cannot come from the
// caller's stack -- it travels as the by-value parameter of a one-lane kernel instead, which the graph's kernel node owns (round 6, ADVICE r5: round 5's
// pinned pool of 32 slots leaked a slot per captured launch and ended every capture after the 32nd)
__global__ void lpcn_set_args_kernel(LpcnSampleArgs *dst, const LpcnSampleArgs a) { *dst = a; }
static bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return st != nullptr && hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
// (while the caller's stream is being captured into a HIP graph nothing is executed: the batch's event chain is left alone -- an event
// recorded inside a capture cannot be waited for from the host -- and ordering replays against other work on the batch is the caller's job)
static int order_begin(lpcn_batch_dev *b, hipStream_t st)
{
    if (stream_is_capturing(st)) return 0;
    if (b->pending && st != b->last_stream) HIP_TRY(hipStreamWaitEvent(st, b->ev_last, 0));
    return 0;
}
static int order_end(lpcn_batch_dev *b, hipStream_t st)
{
    if (stream_is_capturing(st)) return 0;
    HIP_TRY(hipEventRecord(b->ev_last, st));
    b->last_stream = st;
    b->pending = true;
    return 0;
}
// host-side wait for everything enqueued for this batch, whichever stream it went to
static int wait_all(lpcn_batch_dev *b)
{
    if (b->pending) { HIP_TRY(hipEventSynchronize(b->ev_last)); b->pending = false; }
    HIP_TRY(hipStreamSynchronize(b->e->stream));
    return 0;
}

template <typename T>
static int upload(lpcn_engine *e, const T **dst, const void *src, size_t count)
{
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, count * sizeof(T) ? count * sizeof(T) : 16));
    e->allocs.push_back(p);
    if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = (const T *)p;
    return 0;
}

// compiled item counts per lane (sample_variants.h), zero-terminated: fp32 items are 4 VGPRs each, int8 items 1 VGPR
#define LPCN_LIST_ITEM(n) n,
static const int variants_f32[] = {LPCN_VARIANTS_F32(LPCN_LIST_ITEM) 0};
static const int variants_i8[] = {LPCN_VARIANTS_I8(LPCN_LIST_ITEM) 0};
static const int variants_x2[] = {LPCN_VARIANTS_X2(LPCN_LIST_ITEM) 0};
#undef LPCN_LIST_ITEM
// the smallest compiled variant that holds nw items per lane (0: none does)
static int round_up_variant(const int *v, int nw) { for (; *v; ++v) if (nw <= *v) return *v; return 0; }

// the PLC network: the blob's arrays as they are, and for each sparse GRU input matrix the first block of every 8-row group plus the
// blocks' input positions (the index stream {count, pos...} of src/vec.h:347-360 without its counts)
static int plc_upload_net(lpcn_engine *e, const lpcn_plc_model *p)
{
    lpcn::PlcNet &n = e->plc;
    n.d1 = p->d1; n.g1 = p->g1; n.g2 = p->g2;
    int rc = 0;
#define UPP(field, src, count) if ((rc = upload<float>(e, &n.field, src, (size_t)(count)))) return rc
    UPP(dense1_w, p->dense1_w, LPCN_PLC_IN * p->d1); UPP(dense1_b, p->dense1_b, p->d1);
    UPP(gru1_w, p->gru1_w, 32 * (size_t)p->nb1); UPP(gru1_rec, p->gru1_rec, 3 * (size_t)p->g1 * p->g1); UPP(gru1_bias, p->gru1_bias, 6 * p->g1);
    UPP(gru2_w, p->gru2_w, 32 * (size_t)p->nb2); UPP(gru2_rec, p->gru2_rec, 3 * (size_t)p->g2 * p->g2); UPP(gru2_bias, p->gru2_bias, 6 * p->g2);
    UPP(out_w, p->out_w, LPCN_NB_FEAT * p->g2); UPP(out_b, p->out_b, LPCN_NB_FEAT);
    UPP(tansig, lpcn_tansig, 201);
#undef UPP
    for (int g = 0; g < 2; ++g) {
        const int *idx = g ? p->gru2_idx : p->gru1_idx;
        const int groups = 3 * (g ? p->g2 : p->g1) / 8;
        std::vector<int> start(groups + 1, 0), pos;
        for (int r = 0; r < groups; ++r) {
            const int cnt = *idx++;
            for (int k = 0; k < cnt; ++k) pos.push_back(*idx++);
            start[r + 1] = (int)pos.size();
        }
        if ((rc = upload<int>(e, g ? &n.gru2_start : &n.gru1_start, start.data(), start.size()))) return rc;
        if ((rc = upload<int>(e, g ? &n.gru2_pos : &n.gru1_pos, pos.data(), pos.size()))) return rc;
    }
    return 0;
}

// the int8 PLC network (plc_pred_i8_kernel): the float arrays as they are (`bias` -- the generic-C build never reads `subias`), the GRU input
// blocks as the blob has them -- [block][8 rows][4 cols] int8 is one dword per (row, block) already -- with the row groups' first blocks and the
// blocks' input dwords, and the recurrent weights block-major (model_pack.c: lpcn_plc_pack_rec_i8)
static int plc_upload_net_i8(lpcn_engine *e, const lpcn_plc_model *p)
{
    lpcn::PlcNetQ &n = e->plcq;
    n.d1 = e->plc.d1 = p->d1; n.g1 = e->plc.g1 = p->g1; n.g2 = e->plc.g2 = p->g2;
    int rc = 0;
#define UPP(field, src, count) if ((rc = upload<float>(e, &n.field, src, (size_t)(count)))) return rc
    UPP(dense1_w, p->dense1_w, LPCN_PLC_IN * p->d1); UPP(dense1_b, p->dense1_b, p->d1);
    UPP(gru1_bias, p->gru1_bias, 6 * p->g1); UPP(gru2_bias, p->gru2_bias, 6 * p->g2);
    UPP(out_w, p->out_w, LPCN_NB_FEAT * p->g2); UPP(out_b, p->out_b, LPCN_NB_FEAT);
    UPP(tansig, lpcn_tansig, 201);
#undef UPP
    for (int g = 0; g < 2; ++g) {
        const int *idx = g ? p->gru2_idx : p->gru1_idx;
        const int N = g ? p->g2 : p->g1, nb = g ? p->nb2 : p->nb1, groups = 3 * N / 8;
        std::vector<int> start(groups + 1, 0), pos;
        for (int r = 0; r < groups; ++r) {
            const int cnt = *idx++;
            for (int k = 0; k < cnt; ++k) pos.push_back(*idx++ >> 2);
            start[r + 1] = (int)pos.size();
        }
        std::vector<int32_t> rec((size_t)3 * N * N / 4);
        lpcn_plc_pack_rec_i8((const signed char *)(g ? p->gru2_rec : p->gru1_rec), N, rec.data());
        if ((rc = upload<int>(e, g ? &n.gru2_w : &n.gru1_w, g ? p->gru2_w : p->gru1_w, (size_t)8 * nb))) return rc;      // (32 bytes per block)
        if ((rc = upload<int>(e, g ? &n.gru2_rec : &n.gru1_rec, rec.data(), rec.size()))) return rc;
        if ((rc = upload<int>(e, g ? &n.gru2_start : &n.gru1_start, start.data(), start.size()))) return rc;
        if ((rc = upload<int>(e, g ? &n.gru2_pos : &n.gru1_pos, pos.data(), pos.size()))) return rc;
    }
    return 0;
}

extern "C" int lpcn_engine_create(lpcn_engine **out, int device, const lpcn_model_host *m)
{
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        snprintf(g_err, sizeof(g_err), "no HIP device visible: the LPCNet HIP engine has no CPU fallback");
        return LPCN_E_NODEVICE;
    }
    if (device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "bad device %d (have %d)", device, ndev); return LPCN_E_ARG; }
    const int nwv = round_up_variant(m->is_int8 ? variants_i8 : variants_f32, m->nw);
    if (!nwv) {
        snprintf(g_err, sizeof(g_err), "GRU-A does not fit the kernel's item variants (needs %d items on one lane, max 96: more than three full rows' worth of blocks on one wave)", m->nw);
        return LPCN_E_MODEL;
    }
    DeviceGuard guard(device);
    lpcn_engine *e = new lpcn_engine();
    e->device = device;
    e->nw = m->nw; e->nb_b = m->nb_b_padded; e->lpc_gamma = m->lpc_gamma;
    e->is_int8 = m->is_int8 != 0;
    int rc = 0;
    auto fail = [&](int code) { lpcn_engine_destroy(e); return code; };
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return fail(LPCN_E_HIP);

    LpcnSampleArgs &a = e->image[IMG_PARITY].args;
    // GRU-A as dealt to waves and lanes (model_pack.c) + the embedding tables in that lane order: everything that depends on the dealing
    auto upload_gru_a = [&](const lpcn_model_host *mm, GruAImage &img, int nwv_) -> int {
        LpcnSampleArgs &dst = img.args;
        dst = a;                                               // (what does not depend on the dealing is PARITY's)
        // re-pad the item arrays from the model's nw to the compiled variant
        const size_t item_dw = mm->is_int8 ? 1 : 4;            // dwords per (lane, item)
        const uint32_t *src = mm->is_int8 ? (const uint32_t *)mm->pk_a_wq : (const uint32_t *)mm->pk_a_w;
        std::vector<uint32_t> w((size_t)LPCN_WAVES * nwv_ * 64 * item_dw, 0u);
        std::vector<uint8_t> b((size_t)LPCN_WAVES * nwv_ * 64, 0);
        for (int wv = 0; wv < LPCN_WAVES; ++wv)
            for (int j = 0; j < mm->nw; ++j) {
                // the early head of slot 0, [nw - head, nw) in the model, stays end-aligned in the compiled variant's item array
                const int jd = j >= mm->nw - mm->pk_a_head[wv] ? j + (nwv_ - mm->nw) : j;
                memcpy(&w[((size_t)wv * nwv_ + jd) * 64 * item_dw], &src[((size_t)wv * mm->nw + j) * 64 * item_dw], 64 * item_dw * 4);
                memcpy(&b[((size_t)wv * nwv_ + jd) * 64], &mm->pk_a_blk[((size_t)wv * mm->nw + j) * 64], 64);
            }
        const uint32_t *d = nullptr;
        int rc_ = 0;
        if ((rc_ = upload<uint32_t>(e, &d, w.data(), w.size()))) return rc_;
        dst.a_w = (const float4 *)d;
        if ((rc_ = upload<uint8_t>(e, &dst.a_blk, b.data(), b.size()))) return rc_;
        int bound[LPCN_WAVES * 4], allh[LPCN_WAVES * 3];
        for (int wv = 0; wv < LPCN_WAVES; ++wv) {
            for (int k = 0; k < 4; ++k) bound[wv * 4 + k] = mm->pk_a_bound[wv][k];
            for (int k = 0; k < 3; ++k) allh[wv * 3 + k] = mm->pk_a_allh[wv][k];
        }
#define UPD(T, field, srcp, count) if ((rc_ = upload<T>(e, &dst.field, srcp, count))) return rc_
        UPD(int, a_row, mm->pk_a_row, LPCN_WAVES * 3 * 64);
        UPD(int, a_bound, bound, LPCN_WAVES * 4);
        UPD(int, a_allh, allh, LPCN_WAVES * 3);
        UPD(int, a_head, mm->pk_a_head, LPCN_WAVES);
        if (mm->pk_emb[0]) {                                  // (the two-group kernel's image has no lane-ordered tables)
            UPD(float, emb_sig, mm->pk_emb[0], (size_t)256 * LPCN_MAX_SLOTS * LPCN_WG_THREADS);
            UPD(float, emb_pred, mm->pk_emb[1], (size_t)256 * LPCN_MAX_SLOTS * LPCN_WG_THREADS);
            UPD(float, emb_exc, mm->pk_emb[2], (size_t)256 * LPCN_MAX_SLOTS * LPCN_WG_THREADS);
        }
#undef UPD
        img.nw_variant = nwv_; img.present = true;
        return 0;
    };
    if ((rc = upload_gru_a(m, e->image[IMG_PARITY], nwv))) return fail(rc);
#define UP(T, field, src, count) if ((rc = upload<T>(e, &a.field, src, count))) return fail(rc)
    UP(float, a_bias1, m->a_bias + LPCN_ROWS_A, LPCN_ROWS_A);
    UP(float, a_diag, m->a_diag, LPCN_ROWS_A);
    if (m->is_int8) {
        const uint32_t *d = nullptr;
        if ((rc = upload<uint32_t>(e, &d, m->pk_b_wq, (size_t)8 * m->nb_b_padded))) return fail(rc);
        a.b_w = (const float *)d;
        // recurrent matrix: blob layout [6 groups][4 column blocks][8 rows][4] -> [48 rows][4 blocks] dwords
        uint32_t rq[LPCN_ROWS_B * 4];
        const unsigned char *src = (const unsigned char *)m->b_rec;
        for (int r = 0; r < LPCN_ROWS_B; ++r)
            for (int jb = 0; jb < 4; ++jb) memcpy(&rq[r * 4 + jb], src + (((r >> 3) * 4 + jb) * 8 + (r & 7)) * 4, 4);
        if ((rc = upload<uint32_t>(e, &d, rq, LPCN_ROWS_B * 4))) return fail(rc);
        a.b_rec = (const float *)d;
    } else {
        UP(float, b_w, m->pk_b_w, (size_t)32 * m->nb_b_padded);
        UP(float, b_rec, m->b_rec, LPCN_N_B * LPCN_ROWS_B);
    }
    UP(int, b_start, m->pk_b_start, 7);
    UP(uint8_t, b_blk, m->pk_b_blk, m->nb_b_padded + 4);
    UP(float, b_bias, m->b_bias, 2 * LPCN_ROWS_B);
    UP(float, fc_w, m->fc_w, 256 * 2 * LPCN_N_B);
    UP(float, fc_b, m->fc_b, 512);
    UP(float, fc_f, m->fc_f, 512);
    {   // fp16 image of the dual-FC weights, packed in pairs (FAST sub-option)
        std::vector<uint32_t> wh(256 * 2 * LPCN_N_B / 2);
        for (size_t i = 0; i < wh.size(); ++i) {
            const _Float16 lo = (_Float16)m->fc_w[2 * i], hi = (_Float16)m->fc_w[2 * i + 1];
            uint16_t l, h;
            memcpy(&l, &lo, 2); memcpy(&h, &hi, 2);
            wh[i] = (uint32_t)l | ((uint32_t)h << 16);
        }
        UP(uint32_t, fc_wh, wh.data(), wh.size());
    }
    UP(float, tab_tansig, lpcn_tansig, 201);
    UP(float, tab_ulaw2lin, lpcn_ulaw2lin_tab, 256);
    UP(float, tab_logit, lpcn_logit_tab, 256);
#undef UP
    a.nb_b = m->nb_b_padded;
    a.b_dense = m->b_dense;
    if (!m->is_int8 && m->b_dense && !getenv("LPCNET_HIP_NO_X2_IMAGE")) {
        // the two-group kernel (eight float streams per workgroup) runs on its own dealing of GRU-A: chains on waves 0, 1, rows on waves 2..7
        lpcn_model_host mx;
        if (lpcn_model_pack_x2(m, &mx) == 0) {
            const int nwx = round_up_variant(variants_x2, mx.nw);
            mx.pk_b_w = m->pk_b_w; mx.pk_b_start = m->pk_b_start; mx.pk_b_blk = m->pk_b_blk;      // (the check reads GRU-B's packing too: shared)
            const int stx = lpcn_model_selftest(&mx);
            mx.pk_b_w = nullptr; mx.pk_b_start = nullptr; mx.pk_b_blk = nullptr;
            if (nwx && stx == 0) {
                LpcnSampleArgs &ax = e->image[IMG_X2].args;
                rc = upload_gru_a(&mx, e->image[IMG_X2], nwx);
                // ... and the tables in the blob's own [256][1152] order: the start-value pass of the two-group kernel, their only reader
                if (!rc) rc = upload<float>(e, &ax.emb_nat_sig, m->emb_sig, (size_t)256 * LPCN_ROWS_A);
                if (!rc) rc = upload<float>(e, &ax.emb_nat_pred, m->emb_pred, (size_t)256 * LPCN_ROWS_A);
                if (!rc) rc = upload<float>(e, &ax.emb_nat_exc, m->emb_exc, (size_t)256 * LPCN_ROWS_A);
            }
            lpcn_model_release(&mx);
            if (rc) return fail(rc);
        }
        // ... and its twelve-wave form on the image of lpcn_model_pack_x3, where the model has one (a model without keeps the eight-wave kernels)
        lpcn_x3_image im;
        if (e->image[IMG_X2].present && lpcn_model_pack_x3(m, &im) == 0) {
            if (lpcn_x3_image_selftest(m, &im) == 0) {
                GruAImage &img = e->image[IMG_X3];
                LpcnSampleArgs &ax = img.args;
                ax = e->image[IMG_X2].args;                    // (the natural-order tables and everything that does not depend on the dealing)
                int bound[LPCN_X3_WAVES * (1 + LPCN_X3_SEGS)], head[LPCN_X3_WAVES];
                for (int wv = 0; wv < LPCN_X3_WAVES; ++wv) {
                    int end = 0;
                    bound[wv * (1 + LPCN_X3_SEGS)] = 0;
                    for (int k = 1; k <= LPCN_X3_SEGS; ++k) {     // end of P1 segment k; an absent one ends where it starts
                        if (im.kind[wv][k] != LPCN_X3_NONE) end = im.first[wv][k] + im.count[wv][k];
                        bound[wv * (1 + LPCN_X3_SEGS) + k] = end;
                    }
                    head[wv] = im.kind[wv][0] != LPCN_X3_NONE ? im.count[wv][0] : 0;
                }
                const float *dw = nullptr;
                rc = upload<float>(e, &dw, im.w, (size_t)LPCN_X3_WAVES * LPCN_X3_NW * 64 * 4);
                ax.a_w = (const float4 *)dw;
                if (!rc) rc = upload<uint8_t>(e, &ax.a_blk, im.blk, (size_t)LPCN_X3_WAVES * LPCN_X3_NW * 64);
                if (!rc) rc = upload<int>(e, &ax.a_row, &im.row[0][0][0], (size_t)LPCN_X3_WAVES * (1 + LPCN_X3_SEGS) * 64);
                if (!rc) rc = upload<int>(e, &ax.a_bound, bound, LPCN_X3_WAVES * (1 + LPCN_X3_SEGS));
                if (!rc) rc = upload<int>(e, &ax.a_head, head, LPCN_X3_WAVES);
                img.nw_variant = LPCN_X3_NW; img.present = rc == 0;
            }
            lpcn_x3_image_release(&im);
            if (rc) return fail(rc);
        }
    }
    {   // the FAST arithmetic's own GRU-A image where its best dealing is not PARITY's (int8 blobs)
        lpcn_model_host mf;
        const int pf = getenv("LPCNET_HIP_NO_FAST_IMAGE") ? 1 : lpcn_model_pack_fast(m, &mf);
        if (pf < 0) { snprintf(g_err, sizeof(g_err), "packing the FAST image of GRU-A failed"); return fail(LPCN_E_MODEL); }
        if (pf == 0) {
            const int nwf = round_up_variant(variants_i8, mf.nw);
            if (nwf) rc = upload_gru_a(&mf, e->image[IMG_FAST], nwf);
            lpcn_model_release(&mf);
            if (rc) return fail(rc);
        }
    }

    LpcnFrameModel &fm = e->fmodel;
#define UPF(field, src, count) if ((rc = upload<float>(e, &fm.field, src, count))) return fail(rc)
    UPF(conv1_w, m->conv1_w, 3 * LPCN_FRAME_IN * LPCN_COND);
    UPF(conv1_b, m->conv1_b, LPCN_COND);
    UPF(conv2_w, m->conv2_w, 3 * LPCN_COND * LPCN_COND);
    UPF(conv2_b, m->conv2_b, LPCN_COND);
    UPF(pitch_emb, m->pitch_emb, 256 * LPCN_PITCH_EMB);
    UPF(dense1_w, m->dense1_w, LPCN_COND * LPCN_COND);
    UPF(dense1_b, m->dense1_b, LPCN_COND);
    UPF(dense2_w, m->dense2_w, LPCN_COND * LPCN_COND);
    UPF(dense2_b, m->dense2_b, LPCN_COND);
    UPF(a_dense_w, m->a_dense_w, LPCN_COND * LPCN_ROWS_A);
    UPF(a_dense_b, m->a_dense_b, LPCN_ROWS_A);
    UPF(b_dense_w, m->b_dense_w, LPCN_COND * LPCN_ROWS_B);
    UPF(b_dense_b, m->b_dense_b, LPCN_ROWS_B);
    UPF(tab_tansig, lpcn_tansig, 201);
    UPF(tab_idct, lpcn_idct_tab, 324);
    UPF(tab_tw, lpcn_fft_tw, 640);
#undef UPF
    {
        const short *src = lpcn_fft_bitrev;
        if ((rc = upload<short>(e, &fm.tab_bitrev, src, 320))) return fail(rc);
    }
    fm.lpc_gamma = m->lpc_gamma;
    fm.end2end = 0;
    e->plc_present = m->plc.present;
    e->plc_servable = lpcn_plc_servable(m) != 0;
    if (e->plc_servable && (rc = m->is_int8 ? plc_upload_net_i8(e, &m->plc) : plc_upload_net(e, &m->plc))) return fail(rc);
    *out = e;
    return 0;
}

extern "C" void lpcn_engine_destroy(lpcn_engine *e)
{
    if (!e) return;
    DeviceGuard guard(e->device);
    for (void *p : e->allocs) (void)hipFree(p);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}
extern "C" int lpcn_engine_device(const lpcn_engine *e) { return e->device; }

// VQ codebooks of the codec path (the reference's generated ceps_codebooks.c): cb1..3 [1024][17], cb_diff4 [4096][18]
extern "C" int lpcn_engine_set_codebooks(lpcn_engine *e, const float *cb1, const float *cb2, const float *cb3, const float *cb_diff4)
{
    DeviceGuard guard(e->device);
    int rc = 0;
    float pitch[64];
    for (int k = 0; k < 64; ++k) pitch[k] = (float)(pow(2.f, k / 21.) * 32);      // src/lpcnet_dec.c:107 (PITCH_MIN_PERIOD 32)
    // the encoder's searches read [dimension][entry]; ceps_codebook_diff4 by quarters of 1024 entries (encode_kernels.hip.h)
    std::vector<float> t1(17 * 1024), t2(17 * 1024), t3(17 * 1024), td(18 * 4096);
    for (int i = 0; i < 1024; ++i)
        for (int j = 0; j < 17; ++j) { t1[j * 1024 + i] = cb1[i * 17 + j]; t2[j * 1024 + i] = cb2[i * 17 + j]; t3[j * 1024 + i] = cb3[i * 17 + j]; }
    for (int i = 0; i < 4096; ++i)
        for (int j = 0; j < 18; ++j) td[((size_t)(i >> 10) * 18 + j) * 1024 + (i & 1023)] = cb_diff4[i * 18 + j];
    if (e->has_codebooks) {            // a newer codebook version replaces the contents of the buffers already on the device
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy((void *)e->enc.cb1_t, t1.data(), sizeof(float) * t1.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->enc.cb2_t, t2.data(), sizeof(float) * t2.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->enc.cb3_t, t3.data(), sizeof(float) * t3.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->enc.cbd_t, td.data(), sizeof(float) * td.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->dec.cb1, cb1, sizeof(float) * 1024 * 17, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->dec.cb2, cb2, sizeof(float) * 1024 * 17, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->dec.cb3, cb3, sizeof(float) * 1024 * 17, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)e->dec.cb_diff4, cb_diff4, sizeof(float) * 4096 * 18, hipMemcpyHostToDevice));
        return 0;
    }
    if ((rc = upload<float>(e, &e->dec.cb1, cb1, 1024 * 17))) return rc;
    if ((rc = upload<float>(e, &e->dec.cb2, cb2, 1024 * 17))) return rc;
    if ((rc = upload<float>(e, &e->dec.cb3, cb3, 1024 * 17))) return rc;
    if ((rc = upload<float>(e, &e->dec.cb_diff4, cb_diff4, 4096 * 18))) return rc;
    if ((rc = upload<float>(e, &e->dec.pitch, pitch, 64))) return rc;
    if ((rc = upload<float>(e, &e->enc.cb1_t, t1.data(), t1.size()))) return rc;
    if ((rc = upload<float>(e, &e->enc.cb2_t, t2.data(), t2.size()))) return rc;
    if ((rc = upload<float>(e, &e->enc.cb3_t, t3.data(), t3.size()))) return rc;
    if ((rc = upload<float>(e, &e->enc.cbd_t, td.data(), td.size()))) return rc;
    e->enc.cb1 = e->dec.cb1; e->enc.cb2 = e->dec.cb2; e->enc.cb3 = e->dec.cb3; e->enc.cb_diff4 = e->dec.cb_diff4;
    e->has_codebooks = true;
    return 0;
}
extern "C" int lpcn_engine_has_codebooks(const lpcn_engine *e) { return e->has_codebooks ? 1 : 0; }
// LPC_GAMMA is a compile-time constant of the reference's generated nnet_data.h (lpc_weighting, src/freq.c:299-308), not
// part of the weight blob: models trained with --lpc-gamma != 1 set it here.
// END2END is a compile-time switch of the reference (src/lpcnet.c:56-80,107-108), not part of the weight blob
extern "C" int lpcn_engine_set_end2end(lpcn_engine *e, int on)
{
    e->fmodel.end2end = on != 0;
    return 0;
}
// FAST arithmetic: what the reference's own SIMD builds do (src/vec_avx.h) -- fused multiply-add for float blobs, exact
// int32 block accumulation for int8 blobs -- instead of the generic-C order.  Not bit-exact; validated teacher-forced.
extern "C" int lpcn_engine_set_fast(lpcn_engine *e, int on)
{
    e->fast = on != 0;
    e->fc_f16 = on == 2;              // 2 = FAST with the dual FC in fp16 (BASELINE config 4's wording; weights converted at engine creation)
    return 0;
}
extern "C" int lpcn_engine_set_lpc_gamma(lpcn_engine *e, float gamma)
{
    if (!(gamma > 0.f && gamma <= 1.f)) { snprintf(g_err, sizeof(g_err), "lpc_gamma must be in (0, 1]"); return LPCN_E_ARG; }
    e->lpc_gamma = gamma;
    e->fmodel.lpc_gamma = gamma;
    return 0;
}

// ------------------------------------------------------------------------------------ batches --
// Streams per workgroup: one workgroup occupies a CU, so a batch runs in ceil(workgroups / CUs) rounds; a round with S
// interleaved streams costs step[S] (measured us per sample step, tests/tools/gpu_sweep.py).  Pick the cheapest.
static int device_cus(const lpcn_engine *e)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0) return prop.multiProcessorCount;
    return 256;
}
// The GRU-A image a launch at S streams per workgroup runs on: the two-group kernel's at eight; else FAST's own where the engine's
// current arithmetic is FAST and it has one; else PARITY's.
static const GruAImage &gru_a_image(const lpcn_engine *e, int S) { return e->image[S == 8 ? IMG_X2 : (e->fast && e->image[IMG_FAST].present) ? IMG_FAST : IMG_PARITY]; }
static bool pack2_available(const lpcn_engine *e) { return e->is_int8 && gru_a_image(e, 4).nw_variant <= 32; }
// Two groups of four float streams per workgroup, half a step apart (sample_kernel_x2.hip.h): float blobs, PARITY arithmetic, dense GRU-B input
// matrix, <= 32 items per lane.  Eight streams per workgroup select it.
static bool x2_available(const lpcn_batch_dev *b) { return !b->no_x2 && b->e->image[IMG_X2].present && !b->e->fast; }
// ... and its twelve-wave form (sample_kernel_x3.hip.h), where the model has the image for it
static bool x3_available(const lpcn_batch_dev *b) { return x2_available(b) && b->e->image[IMG_X3].present; }
static bool use_pack2(const lpcn_batch_dev *b, int n, int S)
{
    // (S = 4 needs ~92 KB of LDS per workgroup: two do not fit a CU, and the 128-VGPR code alone is slower -- measured 119 vs 137 M)
    if (S > 2 || !pack2_available(b->e)) return false;
    if (b->pack2_force >= 0) return b->pack2_force == 1;
    return (n + S - 1) / S > device_cus(b->e);
}
static int auto_streams_per_wg(const lpcn_batch_dev *b, int n)
{
    const lpcn_engine *e = b->e;
    const int cus = device_cus(e);
    static const float step_f32[3] = {6.5f, 7.6f, 9.9f}, step_i8[3] = {4.4f, 5.5f, 7.3f};
    static const float step_f32_fast[3] = {6.0f, 7.0f, 8.9f}, step_i8_fast[3] = {4.4f, 5.0f, 7.0f};
    // PACK2 (two int8 workgroups per CU): time of a round in which every CU carries two workgroups
    static const float pair_i8[3] = {5.8f, 7.3f, 8.6f}, pair_i8_fast[3] = {5.2f, 6.3f, 7.6f};
    const float *step = e->fast ? (e->is_int8 ? step_i8_fast : step_f32_fast) : (e->is_int8 ? step_i8 : step_f32);
    const float *pair = e->fast ? pair_i8_fast : pair_i8;
    int best = 1;
    float best_t = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int S = 1 << k, wgs = (n + S - 1) / S;
        float t;
        if (use_pack2(b, n, S)) t = (float)((wgs + 2 * cus - 1) / (2 * cus)) * pair[k];
        else t = (float)((wgs + cus - 1) / cus) * step[k];
        if (k == 0 || t < best_t) { best = S; best_t = t; }
    }
    if (x2_available(b)) {                                   // eight streams per workgroup: a round of the two-group kernel (us per sample step)
        static const float step_x2 = 13.9f;
        const int wgs = (n + 7) / 8;
        const float t = (float)((wgs + cus - 1) / cus) * step_x2;
        if (t < best_t) { best = 8; best_t = t; }
    }
    return best;
}

extern "C" int lpcn_batch_dev_create(lpcn_batch_dev **out, lpcn_engine *e, int n, int max_chunk)
{
    *out = nullptr;
    if (!e || n <= 0 || max_chunk <= 0) { snprintf(g_err, sizeof(g_err), "bad batch arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(e->device);
    lpcn_batch_dev *b = new lpcn_batch_dev();
    b->e = e; b->n = n; b->max_chunk = max_chunk;
    const char *off = getenv("LPCNET_HIP_NO_X2"), *force = getenv("LPCNET_HIP_PACK2");      // (read once per batch, never on the launch path)
    b->no_x2 = off && *off == '1'; b->pack2_force = (force && *force) ? *force == '1' : -1;
    const char *tw = getenv("LPCNET_HIP_X3");                // tools (profiles of one form under LPCNET_HIP_NO_AUTOTUNE): 1 = the twelve-wave form wherever the model has the image, 0 = never
    if (tw && *tw) { b->x3_mode = *tw == '1'; b->x3 = b->x3_mode == 1; }
    b->S = auto_streams_per_wg(b, n);
    b->pack2 = use_pack2(b, n, b->S);
    auto fail = [&](int code) { lpcn_batch_dev_destroy(b); return code; };
    const size_t rows = (size_t)n * max_chunk;
    int rc = 0;
    if ((rc = b->d_state.alloc(n)) || (rc = b->d_fc_base.alloc(n)) || (rc = b->d_cond_a.alloc(rows * LPCN_ROWS_A)) || (rc = b->d_cond_b.alloc(rows * LPCN_ROWS_B)) ||
        (rc = b->d_lpc.alloc(rows * LPCN_LPC_ORDER)) || (rc = b->d_cond.alloc((size_t)n * (max_chunk + 4) * LPCN_COND * 2)) || (rc = b->d_args.alloc((size_t)(n > PLC_MAX_GROUPS ? n : PLC_MAX_GROUPS))) ||
        (rc = b->d_vq_mem.alloc((size_t)n * LPCN_NB_BANDS))) return fail(rc);
    for (auto &ev : b->ev) if (hipEventCreate(&ev.e) != hipSuccess) return fail(LPCN_E_HIP);
    if (hipEventCreateWithFlags(&b->ev_last.e, hipEventDisableTiming) != hipSuccess) return fail(LPCN_E_HIP);
    *out = b;
    if ((rc = lpcn_batch_dev_reset(b, 0, n))) return fail(rc);
    return 0;
}

extern "C" void lpcn_batch_dev_destroy(lpcn_batch_dev *b)
{
    if (!b) return;
    DeviceGuard guard(b->e->device);
    (void)wait_all(b);
    delete b;                          // (inside the guard: the buffers, events and the PLC's data are freed on the batch's device)
}

// lpcnet_reset semantics (src/lpcnet.c:174-182): zero everything, last_exc = lin2ulaw(0) = 128,
// RNG seeded from the string "LPCNet" (src/kiss99.c:34-57, evaluated on the host).
static void host_reset_state(lpcn_stream_state *st)
{
    memset(st, 0, sizeof(*st));
    st->last_exc = 128;
    uint32_t c[4] = {362436069u, 521288629u, 123456789u, 380116160u};
    const unsigned char d[6] = {'L', 'P', 'C', 'N', 'e', 't'};
    c[0] ^= d[0]; c[1] ^= d[1]; c[2] ^= d[2]; c[3] ^= d[3];
    lpcn_kiss99(c);
    c[0] ^= d[4]; c[1] ^= d[5];
    if (c[0] == 0 || c[0] == 0x9068FFFFu) c[0]++;
    if (c[1] == 0 || c[1] == 0x464FFFFFu) c[1]++;
    if (c[2] == 0) c[2]++;
    memcpy(st->rng, c, sizeof(c));
}

// lpcn_batch_dev_step_host's per-stream frame products are stale after anything else has advanced or rewritten a stream
static void forget_keep(lpcn_batch_dev *b) { b->keep_ok.assign(b->keep_ok.size(), 0); }
static int check_range(const lpcn_batch_dev *b, int first, int count, const char *what)
{
    if (first < 0 || count < 0 || first + count > b->n) { snprintf(g_err, sizeof(g_err), "%s range", what); return LPCN_E_ARG; }
    return 0;
}
// One stream's record of a per-stream device array, `per` elements at buf + s * per, to the host (down) or from it (up), after everything
// enqueued for the batch.  An array that exists only once its feature is enabled names the call that makes it.
template <typename T>
static int stream_rec(lpcn_batch_dev *b, int s, const DevBuf<T> &buf, size_t per, void *down, const void *up, int (*enable)(lpcn_batch_dev *, int) = nullptr)
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

extern "C" int lpcn_batch_dev_reset(lpcn_batch_dev *b, int first, int count)
{
    forget_keep(b);
    if (check_range(b, first, count, "reset")) return LPCN_E_ARG;
    DeviceGuard guard(b->e->device);
    std::vector<lpcn_stream_state> h(count);
    for (auto &s : h) host_reset_state(&s);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    HIP_TRY(hipMemcpy(b->d_state + first, h.data(), sizeof(lpcn_stream_state) * count, hipMemcpyHostToDevice));
    if (count) HIP_TRY(hipMemset(b->d_vq_mem + (size_t)first * LPCN_NB_BANDS, 0, sizeof(float) * (size_t)count * LPCN_NB_BANDS));
    return 0;
}

extern "C" int lpcn_batch_dev_get_state(lpcn_batch_dev *b, int s, lpcn_stream_state *host) { return stream_rec(b, s, b->d_state, 1, host, nullptr); }
extern "C" int lpcn_batch_dev_set_state(lpcn_batch_dev *b, int s, const lpcn_stream_state *host)
{
    forget_keep(b);
    return stream_rec(b, s, b->d_state, 1, nullptr, host);
}
// the engine's arithmetic flavour changed: re-run the cost model unless the caller pinned the value
extern "C" int lpcn_batch_dev_retune(lpcn_batch_dev *b)
{
    if (b->S_auto) { b->S = auto_streams_per_wg(b, b->n); b->tuned = false; if (b->x3_mode < 0) b->x3 = false; }      // measured again at the next run
    b->pack2 = use_pack2(b, b->n, b->S);
    return 0;
}
extern "C" int lpcn_batch_dev_set_streams_per_wg(lpcn_batch_dev *b, int s)
{
    b->S_auto = s == 0;
    if (s == 0) { s = auto_streams_per_wg(b, b->n); b->tuned = false; }
    if (s == 8 && !x2_available(b)) { snprintf(g_err, sizeof(g_err), "eight streams per workgroup need a float blob with a dense GRU-B matrix and <= 32 items per lane, PARITY arithmetic"); return LPCN_E_ARG; }
    if (s != 1 && s != 2 && s != 4 && s != 8) { snprintf(g_err, sizeof(g_err), "streams per workgroup must be 1, 2, 4 or 8"); return LPCN_E_ARG; }
    b->S = s;
    b->pack2 = use_pack2(b, b->n, b->S);
    return 0;
}
extern "C" int lpcn_batch_dev_set_x3(lpcn_batch_dev *b, int mode)
{
    if (mode < -1 || mode > 1) { snprintf(g_err, sizeof(g_err), "twelve-wave mode must be -1, 0 or 1"); return LPCN_E_ARG; }
    if (mode == 1 && !x3_available(b)) { snprintf(g_err, sizeof(g_err), "the twelve-wave kernel needs a float blob that fits 12 waves x 16 items per lane (dense GRU-B matrix), PARITY arithmetic"); return LPCN_E_ARG; }
    b->x3_mode = mode;
    b->x3 = mode == 1;                                       // (-1: the eight-wave form until the batch is measured)
    if (mode < 0 && b->S_auto) b->tuned = false;
    return 0;
}
extern "C" int lpcn_batch_dev_set_frame_len(lpcn_batch_dev *b, int n)
{
    if (n < 1 || n > LPCN_FRAME_SIZE) { snprintf(g_err, sizeof(g_err), "frame length must be 1..160"); return LPCN_E_ARG; }
    b->frame_len = n;
    return 0;
}
extern "C" int lpcn_batch_dev_enable_timing(lpcn_batch_dev *b, int on) { b->timing = on != 0; return 0; }
extern "C" int lpcn_batch_dev_last_timing(lpcn_batch_dev *b, float *ms_sample, float *ms_frame)
{
    if (ms_sample) *ms_sample = b->ms_sample;
    if (ms_frame) *ms_frame = b->ms_frame;
    return 0;
}
extern "C" int lpcn_batch_dev_sync(lpcn_batch_dev *b)
{
    DeviceGuard guard(b->e->device);
    return wait_all(b);
}

// ------------------------------------------------------------------------------- launches -----
// The sample kernel's variants (streams per workgroup x items per lane x blob flavour x arithmetic) are compiled in
// separate translation units, one per streams-per-workgroup value (sample_variants.hip), so they build in parallel.
extern "C" int lpcn_launch_sample_s1(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);
extern "C" int lpcn_launch_sample_s2(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);
extern "C" int lpcn_launch_sample_s4(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);
extern "C" int lpcn_launch_sample_x2(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);      // sample_x2.hip: two groups of four streams
extern "C" int lpcn_x2_lds_bytes(int nb_b);
extern "C" int lpcn_launch_sample_x3(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);      // sample_x3.hip: the same on twelve waves (same LDS layout)

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
static LaunchShape whole_batch(const lpcn_batch_dev *b) { return {b->n, b->frame_len, b->d_state, b->S, b->pack2, b->x3}; }

// Which sample kernel a launch of n_frames frames per stream gets, on which GRU-A image.  No side effects.
struct SamplePlan {
    int S;                             // streams per workgroup the launch runs with
    bool pack2;
    bool x3;                           // eight streams per workgroup on twelve waves
    const GruAImage *image;            // (with its items-per-lane variant)
    int lds, grid;                     // dynamic LDS bytes per workgroup, workgroups
};
static SamplePlan plan_sample(const lpcn_batch_dev *b, const LaunchShape &sh, int n_frames)
{
    const lpcn_engine *e = b->e;
    SamplePlan p{sh.S, sh.pack2, false, nullptr, 0, 0};
    // Eight streams per workgroup become four (a) while the two-group kernel is unavailable (the arithmetic flavour changed under a pinned value) and
    // (b) for a launch with 4 GB or more of conditioning rows -- more than ~9 300 streams x 100 frames -- which the two-group kernel, addressing them
    // with 32-bit byte offsets, cannot reach
    if (sh.S == 8 && (!x2_available(b) || (unsigned long long)sh.n * (unsigned long long)n_frames * LPCN_ROWS_A * 4ull >= (1ull << 32))) { p.S = 4; p.pack2 = false; }
    p.x3 = p.S == 8 && sh.x3 && x3_available(b);
    p.image = p.x3 ? &e->image[IMG_X3] : &gru_a_image(e, p.S);
    p.lds = p.S == 8 ? lpcn_x2_lds_bytes(e->nb_b) : p.S == 1 ? lpcn::Lds<1>::total(e->nb_b, e->is_int8) : p.S == 2 ? lpcn::Lds<2>::total(e->nb_b, e->is_int8) : lpcn::Lds<4>::total(e->nb_b, e->is_int8);
    p.grid = (sh.n + p.S - 1) / p.S;
    return p;
}
// (what a whole-batch launch of one frame runs with: four while FAST arithmetic is on under a pinned eight)
extern "C" int lpcn_batch_dev_streams_per_wg(const lpcn_batch_dev *b) { return plan_sample(b, whole_batch(b), 1).S; }
extern "C" int lpcn_batch_dev_x3(const lpcn_batch_dev *b) { return plan_sample(b, whole_batch(b), 1).x3 ? 1 : 0; }

// one chunk of the per-sample kernel; cond_a/cond_b/lpc for the chunk are already in the batch buffers
static int launch_sample(lpcn_batch_dev *b, const LaunchShape &sh, hipStream_t st, short *d_pcm, size_t pcm_stride, int n_frames, int preload, bool fc_from_frames)
{
    const lpcn_engine *e = b->e;
    const SamplePlan p = plan_sample(b, sh, n_frames);
    const int nw = p.image->nw_variant;
    LpcnSampleArgs a = p.image->args;
    a.n_streams = sh.n; a.n_frames = n_frames; a.preload = preload; a.frame_len = sh.frame_len;
    a.fc_advance = fc_from_frames ? 1 : 0;
    a.cond_a = b->d_cond_a + (size_t)sh.slot * LPCN_ROWS_A; a.cond_b = b->d_cond_b + (size_t)sh.slot * LPCN_ROWS_B; a.lpc = b->d_lpc + (size_t)sh.slot * LPCN_LPC_ORDER;
    a.fc_base = fc_from_frames ? b->d_fc_base + sh.slot : nullptr;
    a.pcm = d_pcm; a.pcm_stride = (long long)pcm_stride;
    a.state = sh.d_state; a.dbg = b->d_dbg; a.prof = b->d_prof;
    a.fc_f16 = (e->fast && e->fc_f16) ? 1 : 0;
    if ((size_t)sh.arg >= b->d_args.cap) { snprintf(g_err, sizeof(g_err), "sample launch: the step's launches exceed their argument records"); return LPCN_E_HIP; }
    LpcnSampleArgs *d_args = b->d_args + sh.arg;
    // (d_dbg / d_prof are one buffer per batch: the trace and the phase profile are meaningful with one lane only)
    if (stream_is_capturing(st)) {
        hipLaunchKernelGGL(lpcn_set_args_kernel, dim3(1), dim3(1), 0, st, d_args, a);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpyAsync(d_args, &a, sizeof(a), hipMemcpyHostToDevice, st));
    }
    const int i8 = e->is_int8 ? 1 : 0;
    const int flags = (e->fast ? 1 : 0) | (p.pack2 ? 2 : 0);
    int rc = 0;
    switch (p.S) {
    case 8: rc = p.x3 ? lpcn_launch_sample_x3(p.grid, p.lds, st, d_args) : lpcn_launch_sample_x2(nw, p.grid, p.lds, st, d_args); break;
    case 1: rc = lpcn_launch_sample_s1(nw, i8, flags, p.grid, p.lds, st, d_args); break;
    case 2: rc = lpcn_launch_sample_s2(nw, i8, flags, p.grid, p.lds, st, d_args); break;
    default: rc = lpcn_launch_sample_s4(nw, i8, flags, p.grid, p.lds, st, d_args); break;
    }
    if (rc == LPCN_NO_SUCH_VARIANT) { snprintf(g_err, sizeof(g_err), "no compiled sample-kernel variant for %d items per lane at %d streams per workgroup", nw, p.S); return LPCN_E_HIP; }
    if (rc) { snprintf(g_err, sizeof(g_err), "sample kernel launch failed: %s", hipGetErrorString((hipError_t)rc)); return LPCN_E_HIP; }
    return 0;
}

static int launch_frames(lpcn_batch_dev *b, const LaunchShape &sh, hipStream_t st, const float *d_feat, int feat_stride, size_t feat_stream_stride, int n_frames)
{
    return lpcn_launch_frame_kernels(b->e->fmodel, st, sh.n, n_frames, d_feat, feat_stride, feat_stream_stride,
                                     sh.d_state, b->d_fc_base + sh.slot, b->d_cond + (size_t)sh.slot * LPCN_COND, b->d_cond_a + (size_t)sh.slot * LPCN_ROWS_A,
                                     b->d_cond_b + (size_t)sh.slot * LPCN_ROWS_B, b->d_lpc + (size_t)sh.slot * LPCN_LPC_ORDER, g_err, sizeof(g_err));
}

// Streams per workgroup, measured instead of looked up (the table in auto_streams_per_wg holds THIS model's step
// times; a denser / sparser blob or another item-count variant has other optima).  Before the first run of a batch whose
// value is not pinned, each candidate S runs live frames on the batch's own buffers -- zeroed frame products, the stream
// states saved and restored around it -- timed with HIP events: a warm-up launch, then one frame and five frames; the
// DIFFERENCE is the steady-state cost of four frames (a launch's prologue -- filling registers and LDS with the weights --
// is ~4 % of a two-frame launch and grows with the workgroup count, which biased a plain two-frame timing against the
// two-workgroups-per-CU form of the int8 kernel).  ~9 launches, ~12 ms, once per batch and arithmetic flavour;
// LPCNET_HIP_NO_AUTOTUNE=1 keeps the table value.
// Round 4: (a) the FAST flavour is never timed -- its float kernels switch GRU-B's algorithm with S (matrix-pipe GEMM at S >= 2,
// fused DPP chains at S = 1: different summation orders), so a measured S would make FAST output depend on timing noise;
// it takes the table's value, a pure function of (blob kind, stream count, device).  (b) the measurement is the best of
// three timing pairs.  (c) it never runs inside the enqueue-only device-pointer calls on a caller's stream (those take the
// table's value unless lpcnet_batch_tune() has been called): it allocates, synchronises and would break stream capture.
static int autotune_streams_per_wg(lpcn_batch_dev *b, hipStream_t st)
{
    b->tuned = true;
    const char *off = getenv("LPCNET_HIP_NO_AUTOTUNE");
    if ((off && *off == '1') || b->n < 2 || b->e->fast) return 0;     // (one stream: one workgroup whatever S is)
    const int nf = 5 < b->max_chunk ? 5 : b->max_chunk;
    int rc = 0;
    DevBuf<lpcn_stream_state> saved;
    DevBuf<short> pcm;                                       // (a buffer of its own: the caller may be holding the staging buffer's address)
    if ((rc = saved.alloc(b->n)) || (rc = pcm.alloc((size_t)b->n * nf * LPCN_FRAME_SIZE))) return rc;
    std::vector<int> fc((size_t)b->n, LPCN_FEATURES_DELAY + 3);                     // every stream live
    if (hipMemcpyAsync(saved, b->d_state, sizeof(lpcn_stream_state) * b->n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemsetAsync(b->d_cond_a, 0, sizeof(float) * (size_t)b->n * nf * LPCN_ROWS_A, st) != hipSuccess ||
        hipMemsetAsync(b->d_cond_b, 0, sizeof(float) * (size_t)b->n * nf * LPCN_ROWS_B, st) != hipSuccess ||
        hipMemsetAsync(b->d_lpc, 0, sizeof(float) * (size_t)b->n * nf * LPCN_LPC_ORDER, st) != hipSuccess ||
        hipMemcpyAsync(b->d_fc_base, fc.data(), sizeof(int) * b->n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { snprintf(g_err, sizeof(g_err), "auto-tune: buffer setup failed"); return LPCN_E_HIP; }
    int best = b->S;
    bool best_x3 = false;
    float best_ms = -1.f;
    // the candidates: S = 1, 2, 4, 8 and -- where the model has the image, the choice is the engine's and the batch has more than four streams per CU --
    // eight on twelve waves (both forms of the two-group kernel produce the same bits: the choice cannot change a result)
    const bool try_x3 = x3_available(b) && b->x3_mode < 0 && b->n > 4 * device_cus(b->e);
    for (int c = 0; c < 5; ++c) {
        const int S = c < 4 ? 1 << c : 8;
        if (S == 8 && (!x2_available(b) || b->n <= 4)) break;
        if (c == 4 && !try_x3) break;
        const LaunchShape sh = {b->n, b->frame_len, b->d_state, S, use_pack2(b, b->n, S), c == 4 || (S == 8 && b->x3_mode == 1)};
        float ms = -1.f, ms1 = 0.f;
        for (int pass = 0; pass < 7 && !rc; ++pass) {          // warm-up (1 frame), then three pairs of (1 frame, nf frames): the smallest difference
            const int k = (pass && !(pass & 1)) ? nf : 1;
            float t = 0.f;
            if (hipEventRecord(b->ev[1], st) != hipSuccess) rc = LPCN_E_HIP;
            if (!rc) rc = launch_sample(b, sh, st, pcm, (size_t)nf * LPCN_FRAME_SIZE, k, 0, true);
            if (!rc && (hipEventRecord(b->ev[2], st) != hipSuccess || hipEventSynchronize(b->ev[2]) != hipSuccess ||
                        hipEventElapsedTime(&t, b->ev[1], b->ev[2]) != hipSuccess)) rc = LPCN_E_HIP;
            if (pass & 1) ms1 = t;
            else if (pass) { const float d = nf > 1 ? t - ms1 : t; if (ms < 0.f || d < ms) ms = d; }      // nf - 1 frames in steady state
        }
        if (rc) break;
        if (best_ms < 0.f || ms < best_ms) { best_ms = ms; best = S; best_x3 = sh.x3; }
    }
    // the measurement ran on the real state: put it back
    if (hipMemcpyAsync(b->d_state, saved, sizeof(lpcn_stream_state) * b->n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) rc = rc ? rc : LPCN_E_HIP;
    if (rc) return rc;
    b->S = best; b->pack2 = use_pack2(b, b->n, best);
    if (b->x3_mode < 0) b->x3 = best_x3;
    return 0;
}

// lpcnet_batch_tune(): measure now, on the engine's own stream (e.g. right after lpcnet_batch_load_model), so that the first
// synthesize call -- in particular an enqueue-only one on a caller's stream -- carries no measurement
extern "C" int lpcn_batch_dev_tune(lpcn_batch_dev *b)
{
    DeviceGuard guard(b->e->device);
    if (!b->S_auto) return 0;
    hipStream_t st = b->e->stream;
    int rc = order_begin(b, st);
    if (rc) return rc;
    if ((rc = autotune_streams_per_wg(b, st))) return rc;
    return order_end(b, st);
}

// The measurement before the first run of a batch whose value is not pinned (allocates, synchronises, launches trial kernels).  Only the
// host-pointer entry points call it, on the engine's own stream, and BEFORE they make their launch shape, so that the measuring call itself
// runs on the measured value; the enqueue-only device-pointer entry points never do, whichever stream they name (a NULL hip_stream
// used to select the engine's own stream AND the measurement).
static int tune_if_due(lpcn_batch_dev *b, hipStream_t st) { return (b->S_auto && !b->tuned) ? autotune_streams_per_wg(b, st) : 0; }

static int run_impl(lpcn_batch_dev *b, const LaunchShape &sh, const float *d_features, int feat_stride, short *d_pcm, int n_frames, int preload, void *hip_stream)
{
    if (n_frames <= 0 || feat_stride < LPCN_NB_FEAT || preload < 0 || preload > LPCN_FRAME_SIZE) {
        snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG;
    }
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    float tf = 0.f, ts = 0.f;
    { int rco = order_begin(b, st); if (rco) return rco; }
    forget_keep(b);      // (the step call's per-stream frame products are stale now)
    for (int f0 = 0; f0 < n_frames; f0 += b->max_chunk) {
        const int nf = n_frames - f0 < b->max_chunk ? n_frames - f0 : b->max_chunk;
        if (b->timing) HIP_TRY(hipEventRecord(b->ev[0], st));
        int rc = launch_frames(b, sh, st, d_features + (size_t)f0 * feat_stride, feat_stride, (size_t)n_frames * feat_stride, nf);
        if (rc) return rc;
        if (b->timing) HIP_TRY(hipEventRecord(b->ev[1], st));
        rc = launch_sample(b, sh, st, d_pcm + (size_t)f0 * LPCN_FRAME_SIZE, (size_t)n_frames * LPCN_FRAME_SIZE, nf, preload, true);
        if (rc) return rc;
        if (b->timing) {
            HIP_TRY(hipEventRecord(b->ev[2], st));
            HIP_TRY(hipEventSynchronize(b->ev[2]));
            float a = 0.f, c = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, b->ev[0], b->ev[1]));
            HIP_TRY(hipEventElapsedTime(&c, b->ev[1], b->ev[2]));
            tf += a; ts += c;
        }
    }
    if (b->timing) { b->ms_frame = tf; b->ms_sample = ts; }
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_run(lpcn_batch_dev *b, const float *d_features, int feat_stride,
                                  short *d_pcm, int n_frames, int preload, void *hip_stream)
{
    return run_impl(b, whole_batch(b), d_features, feat_stride, d_pcm, n_frames, preload, hip_stream);
}

// the staging buffers of the host-pointer calls, for at least that many floats of features and samples of PCM
static int ensure_staging(lpcn_batch_dev *b, size_t feat_floats, size_t pcm_samples)
{
    const int rc = b->d_feat.reserve(b, feat_floats);
    return rc ? rc : b->d_pcm.reserve(b, pcm_samples);
}

extern "C" int lpcn_batch_dev_run_host(lpcn_batch_dev *b, const float *features, int feat_stride,
                                       short *pcm, int n_frames, int preload)
{
    if (n_frames <= 0) { snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t nfeat = (size_t)b->n * n_frames * feat_stride, npcm = (size_t)b->n * n_frames * LPCN_FRAME_SIZE;
    int rc = ensure_staging(b, nfeat, npcm);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(b->d_feat, features, nfeat * sizeof(float), hipMemcpyHostToDevice, st));
    if (preload > 0) HIP_TRY(hipMemcpyAsync(b->d_pcm, pcm, npcm * sizeof(short), hipMemcpyHostToDevice, st));
    if ((rc = tune_if_due(b, st))) return rc;
    rc = run_impl(b, whole_batch(b), b->d_feat, feat_stride, b->d_pcm, n_frames, preload, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, npcm * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// Single-stream fast path of the legacy per-frame API (a batch of one stream): one frame-network step + frame_len samples
// with ONE host synchronisation.  The caller's POD state is uploaded only when it differs from the device copy
// (st_in == NULL: the device copy is current); features, state and PCM travel through one pinned buffer.
extern "C" int lpcn_batch_dev_run_single(lpcn_batch_dev *b, const lpcn_stream_state *st_in, const float *feat, short *pcm,
                                         lpcn_stream_state *st_out)
{
    if (b->n != 1) { snprintf(g_err, sizeof(g_err), "run_single needs a batch of one stream"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t off_feat = sizeof(lpcn_stream_state), off_pcm = off_feat + LPCN_NB_FEAT * sizeof(float);
    int rc = ensure_staging(b, LPCN_NB_FEAT, LPCN_FRAME_SIZE);
    if (!rc) rc = b->h_pin.reserve(off_pcm + LPCN_FRAME_SIZE * sizeof(short));
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    unsigned char *pin = (unsigned char *)b->h_pin.p;
    if (st_in) {
        memcpy(pin, st_in, sizeof(*st_in));
        HIP_TRY(hipMemcpyAsync(b->d_state, pin, sizeof(*st_in), hipMemcpyHostToDevice, st));
    }
    memcpy(pin + off_feat, feat, LPCN_NB_FEAT * sizeof(float));
    HIP_TRY(hipMemcpyAsync(b->d_feat, pin + off_feat, LPCN_NB_FEAT * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = tune_if_due(b, st))) return rc;
    rc = run_impl(b, whole_batch(b), b->d_feat, LPCN_NB_FEAT, b->d_pcm, 1, 0, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pin, b->d_state, sizeof(lpcn_stream_state), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pin + off_pcm, b->d_pcm, LPCN_FRAME_SIZE * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    b->pending = false;
    memcpy(st_out, pin, sizeof(*st_out));
    memcpy(pcm, pin + off_pcm, (size_t)b->frame_len * sizeof(short));
    return 0;
}

// Combined pass of the legacy per-frame API (api.c: callers of one model that arrive while a pass is in flight are served together):
// k <= capacity independent streams, each with its caller's POD state -- states up, kernels, states and results down, ONE
// synchronisation.  The batch was created with the capacity as its stream count; a pass uses its first k slots.  `kind`:
//   LPCN_GROUP_FRAME_SAMPLES  frame network on feat[i] + frame_len samples (lpcnet_synthesize / lpcnet_synthesize_impl, src/lpcnet.c:273-281);
//                             the first `preload` samples of pcm[i] are imposed (teacher forcing); the frame products come back in
//                             ga[i] / gb[i] (the reference keeps them in the state for a later tail call; lpc is part of the state record)
//   LPCN_GROUP_TAIL           frame_len samples from the caller's products ga[i] / gb[i] / lpc[i] (lpcnet_synthesize_tail_impl, :235-271)
//   LPCN_GROUP_FRAMES         frame network only; products returned in ga[i] / gb[i] / lpc[i] (run_frame_network, :82-120)
// Nothing is written to the callers' memory unless the whole pass succeeded.
extern "C" int lpcn_batch_dev_run_group(lpcn_batch_dev *b, int k, int kind, int frame_len, int preload, const lpcn_stream_state *const *st_in,
                                        const float *const *feat, short *const *pcm, lpcn_stream_state *const *st_out,
                                        float *const *ga, float *const *gb, float *const *lpc)
{
    const bool samples = kind != LPCN_GROUP_FRAMES, frames = kind != LPCN_GROUP_TAIL;
    if (k < 1 || kind < 0 || kind > 2 || (samples && (frame_len < 1 || frame_len > LPCN_FRAME_SIZE || preload < 0 || preload > frame_len))) {
        snprintf(g_err, sizeof(g_err), "bad group arguments"); return LPCN_E_ARG;
    }
    DeviceGuard guard(b->e->device);
    const int cap = b->n;
    if (k > cap) { snprintf(g_err, sizeof(g_err), "group of %d exceeds the batch's %d streams", k, cap); return LPCN_E_ARG; }
    // pinned staging: states | features | pcm | cond_a | cond_b | lpc, each for `cap` streams
    const size_t sz_st = sizeof(lpcn_stream_state), off_feat = sz_st * cap, off_pcm = off_feat + sizeof(float) * LPCN_NB_FEAT * cap;
    const size_t off_ga = off_pcm + sizeof(short) * LPCN_FRAME_SIZE * cap, off_gb = off_ga + sizeof(float) * LPCN_ROWS_A * cap;
    const size_t off_lpc = off_gb + sizeof(float) * LPCN_ROWS_B * cap, pin_bytes = off_lpc + sizeof(float) * LPCN_LPC_ORDER * cap;
    int rc = ensure_staging(b, (size_t)cap * LPCN_NB_FEAT, (size_t)cap * LPCN_FRAME_SIZE);
    if (!rc) rc = b->h_pin.reserve(pin_bytes);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    unsigned char *pin = (unsigned char *)b->h_pin.p;
    for (int i = 0; i < k; ++i) {
        memcpy(pin + sz_st * i, st_in[i], sz_st);
        if (frames) memcpy(pin + off_feat + sizeof(float) * LPCN_NB_FEAT * i, feat[i], sizeof(float) * LPCN_NB_FEAT);
        if (samples && preload > 0) memcpy(pin + off_pcm + sizeof(short) * LPCN_FRAME_SIZE * i, pcm[i], sizeof(short) * (size_t)preload);
        if (kind == LPCN_GROUP_TAIL) {
            memcpy(pin + off_ga + sizeof(float) * LPCN_ROWS_A * i, ga[i], sizeof(float) * LPCN_ROWS_A);
            memcpy(pin + off_gb + sizeof(float) * LPCN_ROWS_B * i, gb[i], sizeof(float) * LPCN_ROWS_B);
            memcpy(pin + off_lpc + sizeof(float) * LPCN_LPC_ORDER * i, lpc[i], sizeof(float) * LPCN_LPC_ORDER);
        }
    }
    HIP_TRY(hipMemcpyAsync(b->d_state, pin, sz_st * k, hipMemcpyHostToDevice, st));
    if (frames) HIP_TRY(hipMemcpyAsync(b->d_feat, pin + off_feat, sizeof(float) * LPCN_NB_FEAT * k, hipMemcpyHostToDevice, st));
    if (samples && preload > 0) HIP_TRY(hipMemcpyAsync(b->d_pcm, pin + off_pcm, sizeof(short) * LPCN_FRAME_SIZE * k, hipMemcpyHostToDevice, st));
    if (kind == LPCN_GROUP_TAIL) {     // (one frame per stream: the chunk buffers are dense [stream][...])
        HIP_TRY(hipMemcpyAsync(b->d_cond_a, pin + off_ga, sizeof(float) * LPCN_ROWS_A * k, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_cond_b, pin + off_gb, sizeof(float) * LPCN_ROWS_B * k, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_lpc, pin + off_lpc, sizeof(float) * LPCN_LPC_ORDER * k, hipMemcpyHostToDevice, st));
    }
    const int S = auto_streams_per_wg(b, k);               // (the table's value for the group's size, never a measurement)
    const LaunchShape sh = {k, samples ? frame_len : b->frame_len, b->d_state, S, use_pack2(b, k, S), b->x3_mode == 1};
    forget_keep(b);
    if (kind == LPCN_GROUP_FRAME_SAMPLES) rc = run_impl(b, sh, b->d_feat, LPCN_NB_FEAT, b->d_pcm, 1, preload, st);
    else if (kind == LPCN_GROUP_TAIL) rc = launch_sample(b, sh, st, b->d_pcm, (size_t)LPCN_FRAME_SIZE, 1, preload, false);
    else rc = launch_frames(b, sh, st, b->d_feat, LPCN_NB_FEAT, (size_t)LPCN_NB_FEAT, 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pin, b->d_state, sz_st * k, hipMemcpyDeviceToHost, st));
    if (samples) HIP_TRY(hipMemcpyAsync(pin + off_pcm, b->d_pcm, sizeof(short) * LPCN_FRAME_SIZE * k, hipMemcpyDeviceToHost, st));
    if (frames) {
        HIP_TRY(hipMemcpyAsync(pin + off_ga, b->d_cond_a, sizeof(float) * LPCN_ROWS_A * k, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pin + off_gb, b->d_cond_b, sizeof(float) * LPCN_ROWS_B * k, hipMemcpyDeviceToHost, st));
        if (kind == LPCN_GROUP_FRAMES) HIP_TRY(hipMemcpyAsync(pin + off_lpc, b->d_lpc, sizeof(float) * LPCN_LPC_ORDER * k, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    b->pending = false;
    for (int i = 0; i < k; ++i) {
        memcpy(st_out[i], pin + sz_st * i, sz_st);
        // live frames return the imposed samples unchanged; start-up frames are cleared entirely (src/lpcnet.c:239-243)
        if (samples) memcpy(pcm[i], pin + off_pcm + sizeof(short) * LPCN_FRAME_SIZE * i, sizeof(short) * (size_t)frame_len);
        if (frames && ga[i]) {                               // (ga[i] == NULL: this caller does not take the frame products back)
            memcpy(ga[i], pin + off_ga + sizeof(float) * LPCN_ROWS_A * i, sizeof(float) * LPCN_ROWS_A);
            memcpy(gb[i], pin + off_gb + sizeof(float) * LPCN_ROWS_B * i, sizeof(float) * LPCN_ROWS_B);
            if (kind == LPCN_GROUP_FRAMES) memcpy(lpc[i], pin + off_lpc + sizeof(float) * LPCN_LPC_ORDER * i, sizeof(float) * LPCN_LPC_ORDER);
        }
    }
    return 0;
}

// Codec path: 8-byte packets [stream][packet][8] -> 4 frames each.  Device pointers, work only enqueued.
static int decode_impl(lpcn_batch_dev *b, const unsigned char *d_packets, short *d_pcm, int n_packets, void *hip_stream, bool may_tune)
{
    forget_keep(b);
    if (n_packets <= 0) { snprintf(g_err, sizeof(g_err), "bad decode arguments"); return LPCN_E_ARG; }
    if (!b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    const int T = 4 * n_packets;
    {   // (growing the staging buffer waits for the batch's outstanding work first; it happens once per size)
        int rc = ensure_staging(b, (size_t)b->n * T * LPCN_NB_FEAT, 0);
        if (rc) return rc;
        if ((rc = order_begin(b, st))) return rc;
    }
    hipLaunchKernelGGL(lpcn::decode_kernel, dim3((b->n + 1) / 2), dim3(64), 0, st, b->e->dec, d_packets, b->n, n_packets, b->d_vq_mem,
                       b->d_feat, LPCN_NB_FEAT);
    HIP_TRY(hipGetLastError());
    if (may_tune) { int rct = tune_if_due(b, st); if (rct) return rct; }      // (decode_host only: the engine's own stream)
    return run_impl(b, whole_batch(b), b->d_feat, LPCN_NB_FEAT, d_pcm, T, 0, st);
}
extern "C" int lpcn_batch_dev_decode(lpcn_batch_dev *b, const unsigned char *d_packets, short *d_pcm, int n_packets, void *hip_stream)
{
    return decode_impl(b, d_packets, d_pcm, n_packets, hip_stream, false);
}

extern "C" int lpcn_batch_dev_decode_host(lpcn_batch_dev *b, const unsigned char *packets, short *pcm, int n_packets)
{
    if (n_packets <= 0) { snprintf(g_err, sizeof(g_err), "bad decode arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t nbytes = (size_t)b->n * n_packets * 8, npcm = (size_t)b->n * n_packets * 4 * LPCN_FRAME_SIZE;
    int rc = b->d_packets.reserve(b, nbytes);
    if (rc) return rc;
    if ((rc = ensure_staging(b, 0, npcm))) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_packets, packets, nbytes, hipMemcpyHostToDevice, st));
    rc = decode_impl(b, b->d_packets, b->d_pcm, n_packets, nullptr, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, npcm * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ------------------------------------------------------------------------------- feature analysis -----
// (stream, frame) items per launch of the analysis kernels: bounds their scratch (2.7 KB per item) at 176 MB
#define LPCN_AN_ITEMS_MAX 65536
static int analysis_chunk_for(const lpcn_batch_dev *b, int n_frames)
{
    int cap = LPCN_AN_ITEMS_MAX / b->n;
    if (cap < 1) cap = 1;
    return n_frames < cap ? n_frames : cap;
}

// the analysis state (if absent) and the kernels' scratch for `chunk` frames per launch
static int analysis_alloc(lpcn_batch_dev *b, int chunk)
{
    int rc = 0;
    if (!b->d_an_state && (rc = b->d_an_state.alloc((size_t)b->n, true))) return rc;      // zeroed: lpcnet_encoder_init (src/lpcnet_enc.c:471-475)
    if (chunk <= b->an_chunk) return 0;
    const size_t items = (size_t)b->n * chunk;
    b->an_chunk = 0;                                         // (until all three have grown)
    if ((rc = b->d_an_resid.reserve(b, items * LPCN_FRAME_SIZE)) || (rc = b->d_an_xc.reserve(b, items * 2 * LPCN_PITCH_MAX_PERIOD)) ||
        (rc = b->d_an_fw.reserve(b, items * 2))) return rc;
    b->an_chunk = chunk;
    return 0;
}
extern "C" int lpcn_batch_dev_analysis_enable(lpcn_batch_dev *b, int max_frames)
{
    if (max_frames < 1) { snprintf(g_err, sizeof(g_err), "analysis: bad frame count"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    return analysis_alloc(b, analysis_chunk_for(b, max_frames));
}

extern "C" int lpcn_batch_dev_analyze(lpcn_batch_dev *b, const void *d_pcm, int pcm_is_float, float *d_features, int feat_stride, int n_frames,
                                      void *hip_stream)
{
    if (!d_pcm || !d_features || n_frames < 1 || feat_stride < LPCN_AN_NB_FEATURES) { snprintf(g_err, sizeof(g_err), "bad analysis arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (!b->d_an_state || analysis_chunk_for(b, n_frames) > b->an_chunk) {
        if (stream_is_capturing(st)) {      // (a capture executes nothing and allocates nothing)
            snprintf(g_err, sizeof(g_err), "analysis state / scratch for %d frames per call must exist before a capture: call lpcnet_batch_analysis_enable first", n_frames);
            return LPCN_E_ARG;
        }
        int rc = lpcn_batch_dev_analysis_enable(b, n_frames);
        if (rc) return rc;
    }
    { int rco = order_begin(b, st); if (rco) return rco; }
    const int is_float = pcm_is_float ? 1 : 0;
    const size_t pcm_stride = (size_t)n_frames * LPCN_FRAME_SIZE, feat_stream_stride = (size_t)n_frames * feat_stride;
    for (int f0 = 0; f0 < n_frames; f0 += b->an_chunk) {
        const int nf = n_frames - f0 < b->an_chunk ? n_frames - f0 : b->an_chunk;
        const void *p = is_float ? (const void *)((const float *)d_pcm + (size_t)f0 * LPCN_FRAME_SIZE) : (const void *)((const short *)d_pcm + (size_t)f0 * LPCN_FRAME_SIZE);
        int rc = lpcn_launch_analysis_kernels(b->e->fmodel, st, b->n, nf, p, is_float, pcm_stride, b->d_an_state, d_features + (size_t)f0 * feat_stride,
                                              feat_stride, feat_stream_stride, b->d_an_resid, b->d_an_xc, b->d_an_fw, g_err, sizeof(g_err));
        if (rc) return rc;
    }
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_analyze_host(lpcn_batch_dev *b, const void *pcm, int pcm_is_float, float *features, int feat_stride, int n_frames)
{
    if (!pcm || !features || n_frames < 1 || feat_stride < LPCN_AN_NB_FEATURES) { snprintf(g_err, sizeof(g_err), "bad analysis arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t npcm = (size_t)b->n * n_frames * LPCN_FRAME_SIZE * (pcm_is_float ? sizeof(float) : sizeof(short));
    const size_t nfeat = (size_t)b->n * n_frames * LPCN_AN_NB_FEATURES;      // (staged densely; the caller's stride is applied by the copy out)
    int rc = b->d_an_pcm.reserve(b, npcm);
    if (!rc) rc = b->d_an_feat.reserve(b, nfeat);
    if (rc) return rc;
    if ((rc = lpcn_batch_dev_analysis_enable(b, n_frames))) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(b->d_an_pcm, pcm, npcm, hipMemcpyHostToDevice, st));
    rc = lpcn_batch_dev_analyze(b, b->d_an_pcm.p, pcm_is_float, b->d_an_feat, LPCN_AN_NB_FEATURES, n_frames, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(features, (size_t)feat_stride * sizeof(float), b->d_an_feat, LPCN_AN_NB_FEATURES * sizeof(float),
                             LPCN_AN_NB_FEATURES * sizeof(float), (size_t)b->n * n_frames, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_analysis_reset(lpcn_batch_dev *b, int first, int count)
{
    if (check_range(b, first, count, "analysis reset")) return LPCN_E_ARG;
    DeviceGuard guard(b->e->device);
    if (!b->d_an_state) return lpcn_batch_dev_analysis_enable(b, 1);      // (a fresh state IS the reset state)
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (count) HIP_TRY(hipMemset(b->d_an_state + first, 0, sizeof(lpcn_analysis_state) * (size_t)count));
    if (count && b->d_enc_vq_mem) HIP_TRY(hipMemset(b->d_enc_vq_mem + (size_t)first * LPCN_NB_BANDS, 0, sizeof(float) * LPCN_NB_BANDS * (size_t)count));
    return 0;
}
extern "C" int lpcn_batch_dev_get_analysis_state(lpcn_batch_dev *b, int s, lpcn_analysis_state *host)
{
    return stream_rec(b, s, b->d_an_state, 1, host, nullptr, lpcn_batch_dev_analysis_enable);
}
extern "C" int lpcn_batch_dev_set_analysis_state(lpcn_batch_dev *b, int s, const lpcn_analysis_state *host)
{
    return stream_rec(b, s, b->d_an_state, 1, nullptr, host, lpcn_batch_dev_analysis_enable);
}

// ------------------------------------------------------------------------------- encoder -----
// lpcnet_encode / lpcnet_compute_features per stream and packet (encode_kernels.hip.h).  A chunk is a whole number of packets within the
// analysis scratch's item bound (at least one packet, whatever the batch size).
static int encode_chunk_for(const lpcn_batch_dev *b, int n_packets)
{
    int cap = LPCN_AN_ITEMS_MAX / b->n / 4;
    if (cap < 1) cap = 1;
    return n_packets < cap ? n_packets : cap;
}

extern "C" int lpcn_batch_dev_encoder_enable(lpcn_batch_dev *b, int max_packets)
{
    if (max_packets < 1) { snprintf(g_err, sizeof(g_err), "encoder: bad packet count"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const int chunk = encode_chunk_for(b, max_packets);
    int rc = analysis_alloc(b, 4 * chunk);
    if (rc) return rc;
    if (!b->d_enc_vq_mem && (rc = b->d_enc_vq_mem.alloc(LPCN_NB_BANDS * (size_t)b->n, true))) return rc;
    if (chunk <= b->enc_chunk) return 0;
    const size_t items = (size_t)b->n * chunk;
    b->enc_chunk = 0;                                        // (until all three have grown)
    if ((rc = b->d_enc_feat.reserve(b, items * 4 * LPCN_AN_NB_FEATURES)) || (rc = b->d_enc_qf3.reserve(b, (size_t)b->n * (chunk + 1) * LPCN_NB_BANDS)) ||
        (rc = b->d_enc_pk.reserve(b, items * lpcn::ENC_PK))) return rc;
    b->enc_chunk = chunk;
    return 0;
}

// d_packets != NULL: encode; else compute_features into d_features
static int encode_impl(lpcn_batch_dev *b, const short *d_pcm, unsigned char *d_packets, float *d_features, int feat_stride, int n_packets, void *hip_stream)
{
    if (!d_pcm || (!d_packets && !d_features) || n_packets < 1 || (!d_packets && feat_stride < LPCN_AN_NB_FEATURES)) {
        snprintf(g_err, sizeof(g_err), "bad encoder arguments");
        return LPCN_E_ARG;
    }
    if (d_packets && !b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    const int want = encode_chunk_for(b, n_packets);
    if (!b->d_an_state || !b->d_enc_vq_mem || want > b->enc_chunk || 4 * want > b->an_chunk) {
        if (stream_is_capturing(st)) {      // (a capture executes nothing and allocates nothing)
            snprintf(g_err, sizeof(g_err), "encoder state / scratch for %d packets per call must exist before a capture: call lpcnet_batch_encoder_enable first", n_packets);
            return LPCN_E_ARG;
        }
        int rc = lpcn_batch_dev_encoder_enable(b, n_packets);
        if (rc) return rc;
    }
    { int rco = order_begin(b, st); if (rco) return rco; }
    const int chunk = b->enc_chunk < b->an_chunk / 4 ? b->enc_chunk : b->an_chunk / 4;
    const size_t pcm_stride = (size_t)n_packets * 4 * LPCN_FRAME_SIZE;
    for (int p0 = 0; p0 < n_packets; p0 += chunk) {
        const int np = n_packets - p0 < chunk ? n_packets - p0 : chunk;
        const short *p = d_pcm + (size_t)p0 * 4 * LPCN_FRAME_SIZE;
        int rc;
        if (d_packets)
            rc = lpcn_launch_encode_kernels(b->e->fmodel, b->e->enc, st, b->n, np, p, pcm_stride, b->d_an_state, b->d_enc_feat, LPCN_AN_NB_FEATURES,
                                            (size_t)np * 4 * LPCN_AN_NB_FEATURES, b->d_an_resid, b->d_an_xc, b->d_an_fw, b->d_enc_vq_mem, b->d_enc_qf3, b->d_enc_pk,
                                            d_packets + (size_t)p0 * 8, n_packets, g_err, sizeof(g_err));
        else
            rc = lpcn_launch_encode_kernels(b->e->fmodel, b->e->enc, st, b->n, np, p, pcm_stride, b->d_an_state, d_features + (size_t)p0 * 4 * feat_stride, feat_stride,
                                            (size_t)n_packets * 4 * feat_stride, b->d_an_resid, b->d_an_xc, b->d_an_fw, b->d_enc_vq_mem, b->d_enc_qf3, b->d_enc_pk,
                                            nullptr, n_packets, g_err, sizeof(g_err));
        if (rc) return rc;
    }
    return order_end(b, st);
}
extern "C" int lpcn_batch_dev_encode(lpcn_batch_dev *b, const short *d_pcm, unsigned char *d_packets, int n_packets, void *hip_stream)
{
    if (!d_packets) { snprintf(g_err, sizeof(g_err), "bad encoder arguments"); return LPCN_E_ARG; }
    return encode_impl(b, d_pcm, d_packets, nullptr, 0, n_packets, hip_stream);
}
extern "C" int lpcn_batch_dev_compute_features(lpcn_batch_dev *b, const short *d_pcm, float *d_features, int feat_stride, int n_packets, void *hip_stream)
{
    if (!d_features) { snprintf(g_err, sizeof(g_err), "bad encoder arguments"); return LPCN_E_ARG; }
    return encode_impl(b, d_pcm, nullptr, d_features, feat_stride, n_packets, hip_stream);
}

// host pointers: copy in, run, copy out, synchronise.  packets != NULL: encode; else compute_features
extern "C" int lpcn_batch_dev_encode_host(lpcn_batch_dev *b, const short *pcm, unsigned char *packets, float *features, int feat_stride, int n_packets)
{
    if (!pcm || (!packets && !features) || n_packets < 1 || (!packets && feat_stride < LPCN_AN_NB_FEATURES)) {
        snprintf(g_err, sizeof(g_err), "bad encoder arguments");
        return LPCN_E_ARG;
    }
    if (packets && !b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    DeviceGuard guard(b->e->device);
    const size_t npcm = (size_t)b->n * n_packets * 4 * LPCN_FRAME_SIZE * sizeof(short);
    const size_t nfeat = packets ? 0 : (size_t)b->n * n_packets * 4 * LPCN_AN_NB_FEATURES, nbytes = packets ? (size_t)b->n * n_packets * 8 : 0;
    int rc = b->d_an_pcm.reserve(b, npcm);
    if (!rc) rc = b->d_an_feat.reserve(b, nfeat);
    if (!rc) rc = b->d_packets.reserve(b, nbytes);
    if (!rc) rc = lpcn_batch_dev_encoder_enable(b, n_packets);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(b->d_an_pcm, pcm, npcm, hipMemcpyHostToDevice, st));
    rc = encode_impl(b, (const short *)b->d_an_pcm.p, packets ? b->d_packets.p : nullptr, packets ? nullptr : b->d_an_feat.p, LPCN_AN_NB_FEATURES, n_packets, st);
    if (rc) return rc;
    if (packets)
        HIP_TRY(hipMemcpyAsync(packets, b->d_packets, nbytes, hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(hipMemcpy2DAsync(features, (size_t)feat_stride * sizeof(float), b->d_an_feat, LPCN_AN_NB_FEATURES * sizeof(float),
                                 LPCN_AN_NB_FEATURES * sizeof(float), (size_t)b->n * n_packets * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_get_encoder_vq_mem(lpcn_batch_dev *b, int s, float *out18)
{
    return stream_rec(b, s, b->d_enc_vq_mem, LPCN_NB_BANDS, out18, nullptr, lpcn_batch_dev_encoder_enable);
}
extern "C" int lpcn_batch_dev_set_encoder_vq_mem(lpcn_batch_dev *b, int s, const float *in18)
{
    return stream_rec(b, s, b->d_enc_vq_mem, LPCN_NB_BANDS, nullptr, in18, lpcn_batch_dev_encoder_enable);
}
extern "C" int lpcn_batch_dev_run_tail_host(lpcn_batch_dev *b, const float *cond_a, const float *cond_b,
                                            const float *lpc, short *pcm, int n_frames, int preload)
{
    forget_keep(b);
    if (n_frames <= 0 || preload < 0 || preload > LPCN_FRAME_SIZE) { snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t npcm = (size_t)b->n * n_frames * LPCN_FRAME_SIZE;
    int rc = ensure_staging(b, 0, npcm);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    if ((rc = tune_if_due(b, st))) return rc;
    if (preload > 0) HIP_TRY(hipMemcpyAsync(b->d_pcm, pcm, npcm * sizeof(short), hipMemcpyHostToDevice, st));
    for (int f0 = 0; f0 < n_frames; f0 += b->max_chunk) {
        const int nf = n_frames - f0 < b->max_chunk ? n_frames - f0 : b->max_chunk;
        // gather the chunk [stream][f0..f0+nf) into the dense chunk buffers
        HIP_TRY(hipMemcpy2DAsync(b->d_cond_a, (size_t)nf * LPCN_ROWS_A * 4, cond_a + (size_t)f0 * LPCN_ROWS_A, (size_t)n_frames * LPCN_ROWS_A * 4,
                                 (size_t)nf * LPCN_ROWS_A * 4, b->n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(b->d_cond_b, (size_t)nf * LPCN_ROWS_B * 4, cond_b + (size_t)f0 * LPCN_ROWS_B, (size_t)n_frames * LPCN_ROWS_B * 4,
                                 (size_t)nf * LPCN_ROWS_B * 4, b->n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(b->d_lpc, (size_t)nf * LPCN_LPC_ORDER * 4, lpc + (size_t)f0 * LPCN_LPC_ORDER, (size_t)n_frames * LPCN_LPC_ORDER * 4,
                                 (size_t)nf * LPCN_LPC_ORDER * 4, b->n, hipMemcpyHostToDevice, st));
        if (b->timing) HIP_TRY(hipEventRecord(b->ev[1], st));
        rc = launch_sample(b, whole_batch(b), st, b->d_pcm + (size_t)f0 * LPCN_FRAME_SIZE, (size_t)n_frames * LPCN_FRAME_SIZE, nf, preload, false);
        if (rc) return rc;
        if (b->timing) {
            HIP_TRY(hipEventRecord(b->ev[2], st));
            HIP_TRY(hipEventSynchronize(b->ev[2]));
            HIP_TRY(hipEventElapsedTime(&b->ms_sample, b->ev[1], b->ev[2]));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, npcm * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_run_frames_host(lpcn_batch_dev *b, const float *features, int feat_stride,
                                              float *cond_a, float *cond_b, float *lpc, int n_frames)
{
    forget_keep(b);
    if (n_frames <= 0 || feat_stride < LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t nfeat = (size_t)b->n * n_frames * feat_stride;
    int rc = ensure_staging(b, nfeat, 0);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_feat, features, nfeat * sizeof(float), hipMemcpyHostToDevice, st));
    for (int f0 = 0; f0 < n_frames; f0 += b->max_chunk) {
        const int nf = n_frames - f0 < b->max_chunk ? n_frames - f0 : b->max_chunk;
        rc = launch_frames(b, whole_batch(b), st, b->d_feat + (size_t)f0 * feat_stride, feat_stride, (size_t)n_frames * feat_stride, nf);
        if (rc) return rc;
        if (cond_a) HIP_TRY(hipMemcpy2DAsync(cond_a + (size_t)f0 * LPCN_ROWS_A, (size_t)n_frames * LPCN_ROWS_A * 4, b->d_cond_a, (size_t)nf * LPCN_ROWS_A * 4,
                                             (size_t)nf * LPCN_ROWS_A * 4, b->n, hipMemcpyDeviceToHost, st));
        if (cond_b) HIP_TRY(hipMemcpy2DAsync(cond_b + (size_t)f0 * LPCN_ROWS_B, (size_t)n_frames * LPCN_ROWS_B * 4, b->d_cond_b, (size_t)nf * LPCN_ROWS_B * 4,
                                             (size_t)nf * LPCN_ROWS_B * 4, b->n, hipMemcpyDeviceToHost, st));
        if (lpc) HIP_TRY(hipMemcpy2DAsync(lpc + (size_t)f0 * LPCN_LPC_ORDER, (size_t)n_frames * LPCN_LPC_ORDER * 4, b->d_lpc, (size_t)nf * LPCN_LPC_ORDER * 4,
                                          (size_t)nf * LPCN_LPC_ORDER * 4, b->n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

// ---- compacted groups: a subset of the batch's streams through the ordinary frame and sample kernels (the per-stream-arguments step below
// and the packet-loss concealment, whose streams take different branches in one step).  The streams of a group are named by an index map on
// the device; their states, their features or kept frame products and their imposed PCM are gathered into dense arrays by small kernels,
// the launch runs on those in the batch's form -- or, under the group schedule, the cost table's form for the group's size (group_shape) -- and
// the results are scattered back by the same map: the hot kernels stay untouched.  A group runs the sample kernel far below its throughput.
// the buffers every group uses: the compacted states, features and PCM, and every stream's most recent frame products (zero until a stream has some)
static int group_alloc(lpcn_batch_dev *b)
{
    if (b->d_keep_lpc) return 0;      // (the last one allocated)
    const size_t n = (size_t)b->n;
    int rc = 0;
    if ((rc = b->d_state_tmp.alloc(n)) || (rc = b->d_gfeat.alloc(n * LPCN_NB_FEAT)) || (rc = b->d_gpcm.alloc(n * LPCN_FRAME_SIZE)) || (rc = b->d_map.alloc(n)) ||
        (rc = b->d_keep_a.alloc(n * LPCN_ROWS_A, true)) || (rc = b->d_keep_b.alloc(n * LPCN_ROWS_B, true))) return rc;
    return b->d_keep_lpc.alloc(n * LPCN_LPC_ORDER, true);
}

// What one group runs (PLC_G_*): FRAMES the frame network alone, FRAME_SAMPLES the frame network and N samples (lpcnet_synthesize_impl,
// src/lpcnet.c:273-277), TAIL N samples from the products of each stream's most recent kept frame (lpcnet_synthesize_tail_impl, :235-271).
// Per-stream rows are given as (pointer, stride in elements): stream s's row starts at pointer + s * stride.
struct GroupRun {
    const int *map;                    // device: the group's stream indices
    int cnt, kind, N, preload;         // streams; PLC_G_*; samples per frame and how many of them are imposed
    const float *feat;                 // kinds with a frame step: every stream's feature vector
    size_t feat_stride;
    const short *pcm_src;              // the samples to impose (NULL: none are gathered)
    size_t pcm_src_stride;
    short *pcm_dst;                    // where the N samples go (NULL: they stay in the compacted d_gpcm, e.g. for a cross-fade)
    size_t pcm_dst_stride;
    bool keep;                         // remember the frame products per stream (lpcnet->gru_a_condition, gru_b_condition, lpc of the reference's state)
    bool scatter;                      // write the states back (false: a trial run)
    int slot = 0, lane = 0;            // the group's rows of the group buffers: [slot, slot + cnt); the lane it was dealt to (for lpcn_batch_dev_last_groups)
};
// The form a compacted group of cnt streams launches in.  Under the group schedule's `form`, with the batch's streams per workgroup chosen by
// the engine and PARITY arithmetic (every form gives the same bits there; FAST's output depends on the form), the cost table's form for cnt
// streams -- a table look-up, never a measurement -- and the twelve-wave form only where the batch already runs it at eight; else the batch's.
static LaunchShape group_shape(const lpcn_batch_dev *b, int cnt, int N, int slot)
{
    if (b->sched_form && b->S_auto && !b->e->fast) {
        const int S = auto_streams_per_wg(b, cnt);
        return {cnt, N, b->d_state_tmp + slot, S, use_pack2(b, cnt, S), S == 8 && b->S == 8 && b->x3, slot, 0};
    }
    return {cnt, N, b->d_state_tmp + slot, b->S, b->pack2, b->x3, slot, 0};
}
static bool aligned16(const void *p, size_t stride_bytes) { return ((uintptr_t)p | (uintptr_t)stride_bytes) % 16 == 0; }
// Enqueues only; the caller checks hipGetLastError() after its groups.  One gather launch, the frame and sample kernels on rows
// [slot, slot + cnt) of the group buffers, one scatter launch.
static int run_group(lpcn_batch_dev *b, hipStream_t st, const GroupRun &g)
{
    const int cnt = g.cnt;
    if (g.slot < 0 || cnt < 1 || g.slot + cnt > b->n) { snprintf(g_err, sizeof(g_err), "group rows [%d, %d) outside the batch", g.slot, g.slot + cnt); return LPCN_E_ARG; }
    LaunchShape sh = group_shape(b, cnt, g.N, g.slot);
    sh.arg = b->args_next;
    const SamplePlan sp = plan_sample(b, sh, 1);
    b->last_groups.push_back({{g.lane, g.slot, cnt, g.kind, g.N, g.preload, sp.S, sp.grid}});
    const bool frames = g.kind != PLC_G_TAIL, samples = g.kind != PLC_G_FRAMES;
    short *gpcm = b->d_gpcm + (size_t)g.slot * LPCN_FRAME_SIZE;
    lpcn::GroupRows r{};
    r.map = g.map; r.cnt = cnt;
    r.states = b->d_state; r.gstates = sh.d_state;
    r.gfeat = b->d_gfeat + (size_t)g.slot * LPCN_NB_FEAT;
    r.keep_a = b->d_keep_a; r.keep_b = b->d_keep_b; r.keep_lpc = b->d_keep_lpc;
    r.cond_a = b->d_cond_a + (size_t)g.slot * LPCN_ROWS_A; r.cond_b = b->d_cond_b + (size_t)g.slot * LPCN_ROWS_B; r.lpc = b->d_lpc + (size_t)g.slot * LPCN_LPC_ORDER;
    r.gpcm = gpcm; r.N = g.N;
    lpcn::GroupRows in = r;
    if (frames) { in.feat = g.feat; in.feat_stride = g.feat_stride; in.feat_vec = aligned16(g.feat, g.feat_stride * sizeof(float)); }
    in.keep = frames ? 0 : 1;
    if (samples && g.pcm_src) { in.pcm = const_cast<short *>(g.pcm_src); in.pcm_stride = g.pcm_src_stride; in.pcm_vec = aligned16(g.pcm_src, g.pcm_src_stride * sizeof(short)); }
    hipLaunchKernelGGL(lpcn::group_gather_kernel, dim3(cnt), dim3(lpcn::PLC_GROUP_THREADS), 0, st, in);
    int rc = 0;
    if (frames && (rc = launch_frames(b, sh, st, r.gfeat, LPCN_NB_FEAT, (size_t)LPCN_NB_FEAT, 1))) return rc;
    if (samples) {
        if ((rc = launch_sample(b, sh, st, gpcm, (size_t)LPCN_FRAME_SIZE, 1, g.preload, frames))) return rc;
        b->args_next++;
    }
    lpcn::GroupRows out = r;
    if (samples && g.pcm_dst) { out.pcm = g.pcm_dst; out.pcm_stride = g.pcm_dst_stride; out.pcm_vec = aligned16(g.pcm_dst, g.pcm_dst_stride * sizeof(short)); }
    out.keep = frames && g.keep ? 1 : 0;
    out.state_back = g.scatter ? 1 : 0;
    if (out.pcm || out.keep || out.state_back)
        hipLaunchKernelGGL(lpcn::group_scatter_kernel, dim3(cnt), dim3(lpcn::PLC_GROUP_THREADS), 0, st, out);
    return 0;
}
// The lanes of a step: lane 0 is the caller's stream, lanes 1 .. are the batch's own streams.  lanes_fork lets them start after what the caller's
// stream holds so far (the step's uploads); lanes_join makes the caller's stream wait for every lane that was given work.
struct Lanes {
    hipStream_t st[PLC_MAX_LANES];
    bool used[PLC_MAX_LANES] = {false, false, false, false};
    bool forked = false;
};
static int lanes_use(lpcn_batch_dev *b, Lanes &ln, int lane, hipStream_t *out)
{
    if (lane < 0 || lane >= b->sched_lanes) { snprintf(g_err, sizeof(g_err), "lane %d of %d", lane, b->sched_lanes); return LPCN_E_ARG; }
    if (lane > 0 && !ln.used[lane]) {
        if (!ln.forked) { HIP_TRY(hipEventRecord(b->ev_fork, ln.st[0])); ln.forked = true; }
        HIP_TRY(hipStreamWaitEvent(ln.st[lane], b->ev_fork, 0));
        ln.used[lane] = true;
    }
    *out = ln.st[lane];
    return 0;
}
static Lanes lanes_begin(lpcn_batch_dev *b, hipStream_t st)
{
    Lanes ln;
    ln.st[0] = st;
    for (int l = 1; l < PLC_MAX_LANES; ++l) ln.st[l] = b->side[l - 1];
    return ln;
}
static int lanes_join(lpcn_batch_dev *b, Lanes &ln)
{
    for (int l = 1; l < PLC_MAX_LANES; ++l)
        if (ln.used[l]) {
            HIP_TRY(hipEventRecord(b->ev_join[l - 1], ln.st[l]));
            HIP_TRY(hipStreamWaitEvent(ln.st[0], b->ev_join[l - 1], 0));
            ln.used[l] = false;
        }
    ln.forked = false;
    return 0;
}

extern "C" int lpcn_batch_dev_set_group_schedule(lpcn_batch_dev *b, int form, int lanes)
{
    if (form < 0 || form > 1 || lanes < 1 || lanes > PLC_MAX_LANES) { snprintf(g_err, sizeof(g_err), "group schedule: form must be 0 or 1 and lanes 1 .. %d", PLC_MAX_LANES); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (lanes > 1 && !b->ev_fork.e) {
        // (each handle is made once: a call that failed part-way is completed by the next one)
        for (auto &sd : b->side) if (!sd.s && hipStreamCreateWithFlags(&sd.s, hipStreamNonBlocking) != hipSuccess) { snprintf(g_err, sizeof(g_err), "group schedule: hipStreamCreate failed"); return LPCN_E_HIP; }
        for (auto &ev : b->ev_join) if (!ev.e && hipEventCreateWithFlags(&ev.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "group schedule: hipEventCreate failed"); return LPCN_E_HIP; }
        if (hipEventCreateWithFlags(&b->ev_fork.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "group schedule: hipEventCreate failed"); return LPCN_E_HIP; }
    }
    b->sched_form = form; b->sched_lanes = lanes;
    return 0;
}
extern "C" int lpcn_batch_dev_get_group_schedule(const lpcn_batch_dev *b, int *form, int *lanes)
{
    if (form) *form = b->sched_form;
    if (lanes) *lanes = b->sched_lanes;
    return 0;
}
extern "C" int lpcn_batch_dev_group_form(const lpcn_batch_dev *b, int cnt)
{
    if (cnt < 1 || cnt > b->n) { snprintf(g_err, sizeof(g_err), "group form: 1 .. %d streams", b->n); return LPCN_E_ARG; }
    return plan_sample(b, group_shape(b, cnt, LPCN_FRAME_SIZE, 0), 1).S;
}
extern "C" int lpcn_batch_dev_last_groups(const lpcn_batch_dev *b, int *rec, int cap)
{
    const int k = (int)b->last_groups.size();
    for (int i = 0; rec && i < k && i < cap; ++i) memcpy(rec + (size_t)i * 8, b->last_groups[(size_t)i].v, sizeof(int) * 8);
    return k;
}

// ---- one frame step with PER-STREAM arguments (src/lpcnet_plc.c calls lpcnet_synthesize_impl(N = TRAINING_OFFSET, preload),
// lpcnet_synthesize_tail_impl(N, preload) and plain frames per stream, depending on which of its streams lost a packet).  mode[s]: 0 = leave
// the stream alone, 1 = frame network on features[s] + n_samples[s] samples, 2 = n_samples[s] samples from the products of the stream's most
// recent frame; the first preload[s] samples of pcm[s] are imposed (teacher forcing).  Streams with equal (mode, n_samples, preload) form a
// group.  The call's features and PCM go up once, the groups run one after the other (run_group), the PCM comes back once.
extern "C" int lpcn_batch_dev_step_host(lpcn_batch_dev *b, const float *features, int feat_stride, short *pcm,
                                        const int *n_samples, const int *preload, const int *mode)
{
    if (!features || !pcm || !n_samples || !preload || !mode || feat_stride < LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "bad step arguments"); return LPCN_E_ARG; }
    for (int s = 0; s < b->n; ++s) {
        if (mode[s] < 0 || mode[s] > 2) { snprintf(g_err, sizeof(g_err), "stream %d: mode must be 0, 1 or 2", s); return LPCN_E_ARG; }
        if (mode[s] && (n_samples[s] < 1 || n_samples[s] > LPCN_FRAME_SIZE || preload[s] < 0 || preload[s] > n_samples[s])) {
            snprintf(g_err, sizeof(g_err), "stream %d: n_samples must be 1..160 and preload 0..n_samples", s); return LPCN_E_ARG;
        }
    }
    // a tail-only step continues the frame of the stream's last mode-1 step: the reference's lpcnet_synthesize_tail_impl uses
    // whatever the last run_frame_network left in the state, but this engine keeps frame products per stream only for
    // steps that went through this call -- a stream advanced by the ordinary synthesize / decode calls has none
    if (b->keep_ok.size() != (size_t)b->n) b->keep_ok.assign((size_t)b->n, 0);
    for (int s = 0; s < b->n; ++s)
        if (mode[s] == 2 && !b->keep_ok[s]) {
            snprintf(g_err, sizeof(g_err), "stream %d: a tail-only step (mode 2) needs a preceding frame step (mode 1) of lpcnet_batch_synthesize_step", s);
            return LPCN_E_ARG;
        }
    DeviceGuard guard(b->e->device);
    const size_t nfeat = (size_t)(b->n - 1) * feat_stride + LPCN_NB_FEAT, npcm = (size_t)b->n * LPCN_FRAME_SIZE;
    int rc = ensure_staging(b, nfeat, npcm);
    if (!rc) rc = group_alloc(b);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    if ((rc = tune_if_due(b, st))) return rc;
    struct Group { int off, cnt, mode, N, preload; };      // (off: the group's place in `map`, which holds every group's streams)
    std::vector<Group> groups;
    std::vector<int> map;
    std::vector<char> done((size_t)b->n, 0);
    for (int s0 = 0; s0 < b->n; ++s0) {
        if (done[s0] || mode[s0] == 0) continue;
        const int off = (int)map.size();
        for (int s = s0; s < b->n; ++s)
            if (!done[s] && mode[s] == mode[s0] && n_samples[s] == n_samples[s0] && preload[s] == preload[s0]) { map.push_back(s); done[s] = 1; }
        groups.push_back({off, (int)map.size() - off, mode[s0], n_samples[s0], preload[s0]});
    }
    if (groups.empty()) return 0;
    HIP_TRY(hipMemcpyAsync(b->d_map, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_feat, features, sizeof(float) * nfeat, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_pcm, pcm, sizeof(short) * npcm, hipMemcpyHostToDevice, st));
    b->args_next = 0; b->last_groups.clear();
    Lanes ln = lanes_begin(b, st);
    int next_lane = 0;
    for (const Group &g : groups) {
        // (only the first N samples of a stream's frame are written: the rest of d_pcm, and the streams of mode 0, go back as they came)
        // The groups hold disjoint streams: with more than one lane they are dealt round-robin, each in the rows of its own place in the map.
        const int lane = next_lane, slot = b->sched_lanes > 1 ? g.off : 0;
        next_lane = (next_lane + 1) % b->sched_lanes;
        hipStream_t lst = st;
        if ((rc = lanes_use(b, ln, lane, &lst))) return rc;
        const GroupRun r = {b->d_map + g.off, g.cnt, g.mode == 1 ? PLC_G_FRAME_SAMPLES : PLC_G_TAIL, g.N, g.preload, b->d_feat, (size_t)feat_stride,
                            g.preload > 0 ? b->d_pcm.p : nullptr, (size_t)LPCN_FRAME_SIZE, b->d_pcm, (size_t)LPCN_FRAME_SIZE, g.mode == 1, true, slot, lane};
        if ((rc = run_group(b, lst, r))) { (void)lanes_join(b, ln); return rc; }
    }
    if ((rc = lanes_join(b, ln))) return rc;
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "per-stream step: kernel launch failed"); return LPCN_E_HIP; }
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, sizeof(short) * npcm, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // only now do the streams of the mode-1 groups own frame products a later tail-only step may continue from (the flag used to
    // be set before the sample launch and the state scatter had succeeded)
    for (const Group &g : groups)
        if (g.mode == 1) for (int i = 0; i < g.cnt; ++i) b->keep_ok[(size_t)map[(size_t)g.off + i]] = 1;
    return 0;
}

// ------------------------------------------------------------------------------- packet-loss concealment -----
// lpcnet_plc_update / lpcnet_plc_conceal in causal mode for every stream (src/lpcnet_plc.c:188-340).  The host keeps the control
// state and plans every step (plc_plan.h: no device needed); the data stays on the device.  A step is one upload of the planner's lists and
// a fixed order of launches with no host synchronisation between them.
extern "C" int lpcn_plc_plan(int options, int n, lpcn_plc_ctl *ctl, const unsigned char *lost, int *summary)
{
    if (n < 1 || !ctl || !lost || (options & 3) == 1 || (options & 3) == 3 || (options & ~7)) { snprintf(g_err, sizeof(g_err), "bad PLC plan arguments"); return LPCN_E_ARG; }
    PlcPlan P;
    return plc_plan(options, n, ctl, lost, P, summary, g_err, sizeof(g_err));
}

extern "C" int lpcn_engine_plc_present(const lpcn_engine *e) { return e->plc_present; }
extern "C" int lpcn_batch_dev_plc_enabled(const lpcn_batch_dev *b) { return b->plc ? 1 : 0; }
extern "C" int lpcn_batch_dev_plc_flavour(const lpcn_batch_dev *b)
{
    if (!b->plc) { snprintf(g_err, sizeof(g_err), "packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; }
    return b->e->is_int8 ? 1 : 0;
}
// compute_plc_pred in the flavour of the engine's blob: the same records and data, the float or the int8 network
static void launch_plc_pred(lpcn_batch_dev *b, hipStream_t st, const int *ctl, int cnt, float *raw_out)
{
    if (b->e->is_int8) hipLaunchKernelGGL(lpcn::plc_pred_i8_kernel, dim3(cnt), dim3(lpcn::PLC_PRED_THREADS), 0, st, b->e->plcq, ctl, cnt, b->plc->D, raw_out);
    else hipLaunchKernelGGL(lpcn::plc_pred_kernel, dim3(cnt), dim3(lpcn::PLC_PRED_THREADS), 0, st, b->e->plc, ctl, cnt, b->plc->D, raw_out);
}
static size_t plc_net_floats(const lpcn_batch_dev *b) { return 4 * (size_t)(b->e->plc.g1 + b->e->plc.g2); }
// lpcnet_plc_reset (src/lpcnet_plc.c:46-60) on streams [first, first + count): the PLC's own fields, the synthesis state, the analysis state
static int plc_reset_range(lpcn_batch_dev *b, int first, int count)
{
    lpcn_plc_host *p = b->plc.get();
    int rc = lpcn_batch_dev_reset(b, first, count);      // (waits for everything enqueued)
    if (!rc) rc = lpcn_batch_dev_analysis_reset(b, first, count);
    if (rc || !count) return rc;
    const size_t G4 = plc_net_floats(b);
#define ZR(buf, per) HIP_TRY(hipMemset((buf).p + (size_t)first * (per), 0, sizeof(*(buf).p) * (size_t)count * (per)))
    ZR(p->q, LPCN_PLC_QUEUE); ZR(p->feat, LPCN_NB_FEAT); ZR(p->net, G4); ZR(p->dc, 2); ZR(p->delta, 1);
    ZR(p->fec, LPCN_PLC_MAX_FEC * LPCN_NB_FEAT); ZR(p->fbuf, LPCN_PLC_FBUF * LPCN_NB_FEAT); ZR(p->lp, LPCN_FRAME_SIZE);
    ZR(p->burg, 2 * LPCN_NB_BANDS); ZR(p->an, LPCN_AN_NB_FEATURES);
    ZR(b->d_keep_a, LPCN_ROWS_A); ZR(b->d_keep_b, LPCN_ROWS_B); ZR(b->d_keep_lpc, LPCN_LPC_ORDER);
#undef ZR
    for (int s = first; s < first + count; ++s) lpcn_plc_ctl_reset(&p->ctl[s]);
    return 0;
}

extern "C" int lpcn_batch_dev_plc_enable(lpcn_batch_dev *b, int options)
{
    if ((options & 3) == 1 || (options & 3) == 3 || (options & ~7)) { snprintf(g_err, sizeof(g_err), "PLC options: LPCNET_PLC_CAUSAL or LPCNET_PLC_CODEC, optionally | LPCNET_PLC_DC_FILTER (the non-causal mode needs a model without feature delay)"); return LPCN_E_ARG; }
    if (b->e->plc_present == 0) { snprintf(g_err, sizeof(g_err), "the model blob has no PLC network (plc_dense1_*, plc_gru1_*, plc_gru2_*, plc_out_*)"); return LPCN_E_MODEL; }
    if (b->e->plc_present != 1 && b->e->plc_present != 2) { snprintf(g_err, sizeof(g_err), "the blob's PLC arrays are incomplete or do not fit together"); return LPCN_E_MODEL; }
    if (b->e->plc_present == 2 && !b->e->plc_servable) { snprintf(g_err, sizeof(g_err), "the blob's PLC network is int8 but its LPCNet model is float: a PLC network is served in its blob's own flavour"); return LPCN_E_MODEL; }
    if (!b->e->plc_servable) { snprintf(g_err, sizeof(g_err), "the blob's PLC network is float but its LPCNet model is int8: a PLC network is served in its blob's own flavour"); return LPCN_E_MODEL; }
    DeviceGuard guard(b->e->device);
    int rc = lpcn_batch_dev_analysis_enable(b, 1);
    if (rc) return rc;
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (!b->plc) {
        auto p = std::make_unique<lpcn_plc_host>();      // (a failure below frees what it holds; the batch stays without PLC)
        const size_t n = (size_t)b->n;
        if ((rc = p->q.alloc(n * LPCN_PLC_QUEUE)) || (rc = p->feat.alloc(n * LPCN_NB_FEAT)) || (rc = p->net.alloc(n * plc_net_floats(b))) || (rc = p->dc.alloc(n * 2)) ||
            (rc = p->delta.alloc(n)) || (rc = p->fec.alloc(n * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT)) || (rc = p->fbuf.alloc(n * LPCN_PLC_FBUF * LPCN_NB_FEAT)) ||
            (rc = p->lp.alloc(n * LPCN_FRAME_SIZE)) || (rc = p->burg.alloc(n * 2 * LPCN_NB_BANDS)) || (rc = p->an.alloc(n * LPCN_AN_NB_FEATURES)) ||
            (rc = p->d_pcm.alloc(n * LPCN_FRAME_SIZE)) || (rc = p->d_ident.alloc(n)) || (rc = p->d_ctl.alloc(64 * n + 64)) ||
            (rc = p->d_feed.alloc(lpcn::PLC_FEED_REC * n)) || (rc = p->h_ctl.reserve(sizeof(int) * (p->d_ctl.cap + p->d_feed.cap))) || (rc = group_alloc(b))) return rc;
        p->D = {p->q, p->feat, p->net, p->dc, p->delta, p->fec, p->fbuf, p->lp, p->burg, p->an};
        if (hipEventCreateWithFlags(&p->ev_ctl.e, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&p->ev_feed.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "PLC: hipEventCreate failed"); return LPCN_E_HIP; }
        std::vector<int> ident(n);
        for (size_t i = 0; i < n; ++i) ident[i] = (int)i;
        if (hipMemcpy(p->d_ident, ident.data(), sizeof(int) * n, hipMemcpyHostToDevice) != hipSuccess) { snprintf(g_err, sizeof(g_err), "PLC: upload failed"); return LPCN_E_HIP; }
        p->ctl.resize(n);
        b->plc = std::move(p);
    }
    b->plc->options = options; b->plc->remove_dc = (options & 4) != 0;
    return plc_reset_range(b, 0, b->n);
}
#define NEED_PLC(b) do { if (!(b)->plc) { snprintf(g_err, sizeof(g_err), "packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; } } while (0)

extern "C" int lpcn_batch_dev_plc_reset(lpcn_batch_dev *b, int first, int count)
{
    NEED_PLC(b);
    if (check_range(b, first, count, "PLC reset")) return LPCN_E_ARG;
    DeviceGuard guard(b->e->device);
    return plc_reset_range(b, first, count);
}

// a group of the plan: its sources and destinations among the PLC's arrays and the call's frame
static GroupRun plc_group(lpcn_plc_host *p, const PlcLaunch &L, short *d_pcm)
{
    const bool queued = L.feat_src != 0;      // the features are entry feat_src - 1 of the deferred queue, else st->features
    return {p->d_ctl + L.off, L.cnt, L.kind, L.N, L.preload,
            queued ? p->fbuf + (size_t)(L.feat_src - 1) * LPCN_NB_FEAT : p->feat.p, queued ? (size_t)LPCN_PLC_FBUF * LPCN_NB_FEAT : (size_t)LPCN_NB_FEAT,
            L.pcm_src == 1 ? p->q.p : L.pcm_src == 2 ? d_pcm + L.pcm_off : nullptr, L.pcm_src == 1 ? (size_t)LPCN_PLC_QUEUE : (size_t)LPCN_FRAME_SIZE,
            L.pcm_dst == 1 ? d_pcm + L.pcm_off : nullptr, (size_t)LPCN_FRAME_SIZE, L.keep, L.scatter, L.slot, L.lane};
}
extern "C" int lpcn_batch_dev_plc_step(lpcn_batch_dev *b, short *d_pcm, const unsigned char *lost, void *hip_stream)
{
    NEED_PLC(b);
    if (!d_pcm || !lost) { snprintf(g_err, sizeof(g_err), "bad PLC step arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) {
        snprintf(g_err, sizeof(g_err), "a PLC step cannot be captured: its launch sequence depends on the loss flags"); return LPCN_E_ARG;
    }
    { int rco = order_begin(b, st); if (rco) return rco; }
    if (p->ctl_pending) { HIP_TRY(hipEventSynchronize(p->ev_ctl)); p->ctl_pending = false; }      // (the previous step's lists have left the pinned buffer: long done)
    int rc = plc_plan(p->options, b->n, p->ctl.data(), lost, p->plan, nullptr, g_err, sizeof(g_err), b->sched_lanes);
    if (rc) return rc;
    const PlcPlan &P = p->plan;
    if (P.ctl.size() > p->d_ctl.cap) { snprintf(g_err, sizeof(g_err), "PLC step: control lists exceed their buffer"); return LPCN_E_HIP; }
    if (!P.ctl.empty()) {
        memcpy(p->h_ctl.p, P.ctl.data(), sizeof(int) * P.ctl.size());
        HIP_TRY(hipMemcpyAsync(p->d_ctl, p->h_ctl.p, sizeof(int) * P.ctl.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(p->ev_ctl, st));
        p->ctl_pending = true;
    }
    forget_keep(b);      // (lpcn_batch_dev_step_host's products are the PLC's now)
    b->args_next = 0; b->last_groups.clear();
    // Lanes run side by side from here -- the lists are up -- to the join in front of the analysis; from there on everything is on the caller's stream.
    Lanes ln = lanes_begin(b, st);
    const hipStream_t caller = st;
    for (const PlcLaunch &L : P.launches) {
        const int *ctl = p->d_ctl + L.off;
        if (L.type == PLC_T_ANALYSIS) rc = lanes_join(b, ln);
        if (!rc) rc = lanes_use(b, ln, L.lane, &st);      // (st: the launch's lane from here on)
        if (rc) { (void)lanes_join(b, ln); return rc; }
        switch (L.type) {
        case PLC_T_BURG:
            hipLaunchKernelGGL(lpcn::plc_burg_kernel, dim3(L.cnt), dim3(lpcn::PLC_BURG_THREADS), 0, st, b->e->fmodel, ctl, L.cnt, d_pcm, p->D, p->remove_dc ? 1 : 0);
            break;
        case PLC_T_PRED:
            launch_plc_pred(b, st, ctl, L.cnt, nullptr);
            break;
        case PLC_T_MIX:
            hipLaunchKernelGGL(lpcn::plc_mix_kernel, dim3(L.cnt), dim3(lpcn::PLC_MIX_THREADS), 0, st, L.op, ctl, L.cnt, d_pcm, (const short *)b->d_gpcm + (size_t)L.slot * LPCN_FRAME_SIZE, p->D, b->d_state);
            break;
        case PLC_T_GROUP:
            if ((rc = run_group(b, st, plc_group(p, L, d_pcm)))) { (void)lanes_join(b, ln); return rc; }
            break;
        case PLC_T_ANALYSIS:
            if ((rc = lpcn_launch_analysis_kernels(b->e->fmodel, st, b->n, 1, d_pcm, 0, (size_t)LPCN_FRAME_SIZE, b->d_an_state, p->D.an, LPCN_AN_NB_FEATURES,
                                                   (size_t)LPCN_AN_NB_FEATURES, b->d_an_resid, b->d_an_xc, b->d_an_fw, g_err, sizeof(g_err)))) return rc;
            break;
        }
    }
    if ((rc = lanes_join(b, ln))) return rc;      // (a plan always has its analysis launch: nothing is left to join)
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "PLC step: kernel launch failed"); return LPCN_E_HIP; }
    return order_end(b, caller);
}

extern "C" int lpcn_batch_dev_plc_step_host(lpcn_batch_dev *b, short *pcm, const unsigned char *lost)
{
    NEED_PLC(b);
    if (!pcm || !lost) { snprintf(g_err, sizeof(g_err), "bad PLC step arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    int rc = order_begin(b, st);
    if (rc) return rc;
    if ((rc = tune_if_due(b, st))) return rc;
    const size_t bytes = sizeof(short) * (size_t)b->n * LPCN_FRAME_SIZE;
    HIP_TRY(hipMemcpyAsync(p->d_pcm, pcm, bytes, hipMemcpyHostToDevice, st));
    if ((rc = lpcn_batch_dev_plc_step(b, p->d_pcm, lost, st))) return rc;
    HIP_TRY(hipMemcpyAsync(pcm, p->d_pcm, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_plc_fec_add(lpcn_batch_dev *b, int s, const float *features20)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    lpcn_plc_host *p = b->plc.get();
    lpcn_plc_ctl &c = p->ctl[s];
    const int keep = c.fec_keep, fill = c.fec_fill;
    const int r = lpcn_plc_ctl_fec_add(&c, features20 == nullptr);
    if (!features20) return 0;
    if (r == 1) { snprintf(g_err, sizeof(g_err), "stream %d: FEC buffer full", s); return 1; }      // (the reference prints this and drops the vector)
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    float *ring = p->fec + (size_t)s * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT;
    if (r == 2) {
        hipLaunchKernelGGL(lpcn::plc_fec_move_kernel, dim3(1), dim3(256), 0, b->e->stream, ring, keep, fill - keep);
        HIP_TRY(hipStreamSynchronize(b->e->stream));
    }
    HIP_TRY(hipMemcpy(ring + (size_t)(c.fec_fill - 1) * LPCN_NB_FEAT, features20, sizeof(float) * LPCN_NB_FEAT, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int lpcn_batch_dev_plc_fec_clear(lpcn_batch_dev *b, int s)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    lpcn_plc_ctl &c = b->plc->ctl[s];
    c.fec_keep = c.fec_read = c.fec_fill = c.fec_skip = 0;      // src/lpcnet_plc.c:129-131
    return 0;
}

// lpcnet_plc_fec_clear / lpcnet_plc_fec_add for every stream in one call (plc_plan.h: plc_fec_feed_plan): the host plans every ring's rows from
// the control state, the records go up through the pinned list buffer and one launch moves the vectors.  Enqueue only; count, skip, clear and
// dropped are host arrays, d_features the packed vectors on the device.  Returns 1 when a vector was dropped ("FEC buffer full").
extern "C" int lpcn_plc_fec_feed_plan(int n, lpcn_plc_ctl *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped)
{
    if (n < 1 || !ctl || !count || !rec) { snprintf(g_err, sizeof(g_err), "bad FEC feed plan arguments"); return LPCN_E_ARG; }
    return plc_fec_feed_plan(n, ctl, count, skip, clear, rec, dropped, nullptr, g_err, sizeof(g_err));
}

extern "C" int lpcn_batch_dev_plc_fec_feed(lpcn_batch_dev *b, const float *d_features, const int *count, const int *skip, const unsigned char *clear,
                                           int *dropped, void *hip_stream)
{
    NEED_PLC(b);
    bool vectors = false;
    for (int s = 0; count && s < b->n; ++s) vectors |= count[s] > 0;
    if (!count || (vectors && !d_features)) { snprintf(g_err, sizeof(g_err), "bad FEC feed arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    if (stream_is_capturing(st)) {
        snprintf(g_err, sizeof(g_err), "an FEC feed cannot be captured: its launch depends on the rings' positions"); return LPCN_E_ARG;
    }
    if (p->feed_pending) { HIP_TRY(hipEventSynchronize(p->ev_feed)); p->feed_pending = false; }      // (the previous feed's records have left the pinned buffer)
    int *h_rec = (int *)p->h_ctl.p + p->d_ctl.cap, any = 0;
    const int n_rec = plc_fec_feed_plan(b->n, p->ctl.data(), count, skip, clear, h_rec, dropped, &any, g_err, sizeof(g_err));
    if (n_rec < 0) return n_rec;
    if (any) snprintf(g_err, sizeof(g_err), "FEC buffer full");      // (the reference prints this and drops the vector)
    if (n_rec == 0) return any;
    { int rco = order_begin(b, st); if (rco) return rco; }
    HIP_TRY(hipMemcpyAsync(p->d_feed, h_rec, sizeof(int) * lpcn::PLC_FEED_REC * (size_t)n_rec, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->ev_feed, st));
    p->feed_pending = true;
    hipLaunchKernelGGL(lpcn::plc_fec_feed_kernel, dim3(n_rec), dim3(lpcn::PLC_FEED_THREADS), 0, st, (const int *)p->d_feed, n_rec, d_features, p->D.fec);
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "FEC feed: kernel launch failed"); return LPCN_E_HIP; }
    { int rco = order_end(b, st); if (rco) return rco; }
    return any;
}

extern "C" int lpcn_batch_dev_plc_fec_feed_host(lpcn_batch_dev *b, const float *features, const int *count, const int *skip, const unsigned char *clear, int *dropped)
{
    NEED_PLC(b);
    if (!count) { snprintf(g_err, sizeof(g_err), "bad FEC feed arguments"); return LPCN_E_ARG; }
    size_t total = 0;
    for (int s = 0; s < b->n; ++s) {
        if (count[s] < 0) { snprintf(g_err, sizeof(g_err), "FEC feed: stream %d has a negative count", s); return LPCN_E_ARG; }
        total += (size_t)count[s];
    }
    if (total && !features) { snprintf(g_err, sizeof(g_err), "bad FEC feed arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    int rc = p->d_feed_src.reserve(b, total * LPCN_NB_FEAT);
    if (rc) return rc;
    if (total) HIP_TRY(hipMemcpyAsync(p->d_feed_src, features, sizeof(float) * total * LPCN_NB_FEAT, hipMemcpyHostToDevice, st));
    if ((rc = lpcn_batch_dev_plc_fec_feed(b, p->d_feed_src, count, skip, clear, dropped, st)) < 0) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// one stream's record, both halves: the device arrays' part field by field, down into *h or up from it
static int plc_state_copy(lpcn_batch_dev *b, int s, lpcn_plc_state_rec *h, bool up)
{
    lpcn_plc_host *p = b->plc.get();
    const size_t i = (size_t)s, G = (size_t)(b->e->plc.g1 + b->e->plc.g2);
    const struct { void *dev, *host; size_t bytes; } fields[] = {
        {p->delta + i, &h->delta, sizeof(int)}, {p->dc + 2 * i, h->dc, sizeof(h->dc)}, {p->q + i * LPCN_PLC_QUEUE, h->q, sizeof(h->q)},
        {p->feat + i * LPCN_NB_FEAT, h->feat, sizeof(h->feat)},
        {p->net + (4 * i + 0) * G, h->net[0], sizeof(float) * G}, {p->net + (4 * i + 1) * G, h->net[1], sizeof(float) * G},
        {p->net + (4 * i + 2) * G, h->net[2], sizeof(float) * G}, {p->net + (4 * i + 3) * G, h->net[3], sizeof(float) * G},
        {p->fec + i * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT, h->fec, sizeof(h->fec)}, {p->fbuf + i * LPCN_PLC_FBUF * LPCN_NB_FEAT, h->fbuf, sizeof(h->fbuf)},
        {b->d_keep_a + i * LPCN_ROWS_A, h->keep_a, sizeof(h->keep_a)}, {b->d_keep_b + i * LPCN_ROWS_B, h->keep_b, sizeof(h->keep_b)},
        {b->d_keep_lpc + i * LPCN_LPC_ORDER, h->keep_lpc, sizeof(h->keep_lpc)}};
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (up) p->ctl[i] = h->ctl;
    for (const auto &f : fields) HIP_TRY(up ? hipMemcpy(f.dev, f.host, f.bytes, hipMemcpyHostToDevice) : hipMemcpy(f.host, f.dev, f.bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lpcn_batch_dev_get_plc_state(lpcn_batch_dev *b, int s, lpcn_plc_state_rec *h)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n || !h) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    memset(h, 0, sizeof(*h));
    h->ctl = b->plc->ctl[s]; h->g1 = b->e->plc.g1; h->g2 = b->e->plc.g2;
    return plc_state_copy(b, s, h, false);
}

extern "C" int lpcn_batch_dev_set_plc_state(lpcn_batch_dev *b, int s, const lpcn_plc_state_rec *h)
{
    NEED_PLC(b);
    if (s < 0 || s >= b->n || !h) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    const int g1 = b->e->plc.g1, g2 = b->e->plc.g2;
    if (h->g1 != g1 || h->g2 != g2) { snprintf(g_err, sizeof(g_err), "PLC state of a %d / %d network on a %d / %d network", h->g1, h->g2, g1, g2); return LPCN_E_ARG; }
    {   // (the planner's own consistency check, on a copy)
        lpcn_plc_ctl c = h->ctl;
        const unsigned char one = 1;
        PlcPlan P;
        int rc = plc_plan(b->plc->options, 1, &c, &one, P, nullptr, g_err, sizeof(g_err));
        if (rc) return rc;
    }
    return plc_state_copy(b, s, const_cast<lpcn_plc_state_rec *>(h), true);      // (up: *h is only read)
}

// parity seam: burg_cepstral_analysis on one frame per stream.  x holds PCM values as the PLC feeds them (x[i] = pcm[i], src/lpcnet_plc.c:206):
// integers of the int16 range.
extern "C" int lpcn_batch_dev_plc_burg_host(lpcn_batch_dev *b, const float *x, float *ceps36)
{
    NEED_PLC(b);
    if (!x || !ceps36) { snprintf(g_err, sizeof(g_err), "bad arguments"); return LPCN_E_ARG; }
    const size_t count = (size_t)b->n * LPCN_FRAME_SIZE;
    std::vector<short> pc(count);
    for (size_t i = 0; i < count; ++i) {
        if (!(x[i] >= -32768.f && x[i] <= 32767.f) || x[i] != (float)(int)x[i]) { snprintf(g_err, sizeof(g_err), "plc_burg: samples must be integers of the int16 range"); return LPCN_E_ARG; }
        pc[i] = (short)(int)x[i];
    }
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    HIP_TRY(hipMemcpy(p->d_pcm, pc.data(), sizeof(short) * count, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(lpcn::plc_burg_kernel, dim3(b->n), dim3(lpcn::PLC_BURG_THREADS), 0, st, b->e->fmodel, (const int *)p->d_ident, b->n, p->d_pcm, p->D, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(ceps36, p->burg, sizeof(float) * (size_t)b->n * 2 * LPCN_NB_BANDS, hipMemcpyDeviceToHost));
    return 0;
}

// parity seam: compute_plc_pred on every stream's network state (which advances), any 57 inputs
extern "C" int lpcn_batch_dev_plc_pred_host(lpcn_batch_dev *b, const float *in57, float *out20)
{
    NEED_PLC(b);
    if (!in57 || !out20) { snprintf(g_err, sizeof(g_err), "bad arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    lpcn_plc_host *p = b->plc.get();
    hipStream_t st = b->e->stream;
    std::vector<int> recs((size_t)b->n * lpcn::PLC_PRED_REC, 0);
    if (recs.size() > p->d_ctl.cap) { snprintf(g_err, sizeof(g_err), "plc_pred: control buffer"); return LPCN_E_HIP; }
    for (int s = 0; s < b->n; ++s) {
        const float *in = in57 + (size_t)s * LPCN_PLC_IN;
        int *r = &recs[(size_t)s * lpcn::PLC_PRED_REC];
        r[0] = s; r[1] = lpcn::PLC_F_COMPUTE | lpcn::PLC_F_RAW; r[3] = float_bits(in[LPCN_PLC_IN - 1]);
        HIP_TRY(hipMemcpy(p->burg + (size_t)s * 2 * LPCN_NB_BANDS, in, sizeof(float) * 2 * LPCN_NB_BANDS, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(p->an + (size_t)s * LPCN_AN_NB_FEATURES, in + 2 * LPCN_NB_BANDS, sizeof(float) * LPCN_NB_FEAT, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(p->d_ctl, recs.data(), sizeof(int) * recs.size(), hipMemcpyHostToDevice));
    launch_plc_pred(b, st, p->d_ctl, b->n, b->d_gfeat.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out20, b->d_gfeat, sizeof(float) * (size_t)b->n * LPCN_NB_FEAT, hipMemcpyDeviceToHost));
    return 0;
}

// debug trace (tests only): allocate / fetch the per-sample trace of workgroup 0, stream 0
extern "C" int lpcn_batch_dev_debug_trace(lpcn_batch_dev *b, int n_samples, float *host_out)
{
    DeviceGuard guard(b->e->device);
    if (host_out == nullptr) {
        { int rcw = wait_all(b); if (rcw) return rcw; }
        b->d_dbg.release();
        return n_samples > 0 ? b->d_dbg.alloc((size_t)n_samples * LPCN_DBG_STRIDE, true) : 0;
    }
    if (!b->d_dbg) { snprintf(g_err, sizeof(g_err), "trace not enabled"); return LPCN_E_ARG; }
    { int rcw = wait_all(b); if (rcw) return rcw; }
    HIP_TRY(hipMemcpy(host_out, b->d_dbg, sizeof(float) * (size_t)n_samples * LPCN_DBG_STRIDE, hipMemcpyDeviceToHost));
    return 0;
}

// per-phase shader-clock totals of workgroup 0 / wave 0 (out == NULL: enable + zero; else fetch 8 values)
extern "C" int lpcn_batch_dev_profile(lpcn_batch_dev *b, unsigned long long *out)
{
    DeviceGuard guard(b->e->device);
    if (!b->d_prof) { int rca = b->d_prof.alloc(96); if (rca) return rca; }
    { int rcw = wait_all(b); if (rcw) return rcw; }
    if (!out) { HIP_TRY(hipMemset(b->d_prof, 0, 96 * sizeof(unsigned long long))); return 0; }
    HIP_TRY(hipMemcpy(out, b->d_prof, 96 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

// test seam: the device's 10^x (lpcnet_exp10.h) for host arrays
extern "C" int lpcn_debug_exp10(int device, const float *x, double *out, size_t n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "no such HIP device"); return LPCN_E_NODEVICE; }
    DeviceGuard guard(device);
    DevBuf<float> dx;
    DevBuf<double> dy;
    int rc = 0;
    if ((rc = dx.alloc(n)) || (rc = dy.alloc(n))) return rc;
    if (hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = LPCN_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(lpcn::exp10_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const float *)dx, dy.p, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dy, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = LPCN_E_HIP;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "exp10 test kernel failed");
    return rc;
}

// test seam: the arithmetic identities PARITY rests on, evaluated with THIS library's compile flags and float mode.
//   * v_mfma_f32_4x4x1(A, B, C = -0.0): register k of lane j of a quad == v_mul_f32(A of lane k, B of lane j), bit for bit
//     (the GRU-A items of the float PARITY kernels form their products there, sample_kernel.hip.h: mac());
//   * each half of v_pk_mul_f32 / v_pk_add_f32 == v_mul_f32 / v_add_f32 (GRU-B's block loop, the items' sums).
// n lanes (a multiple of 64).  out_mfma / out_mul: [n][4] bit patterns (k = 0..3: A from lane 4*(i/4) + k, B from lane i);
// out_pk / out_sc: [n][4] = {pk_mul half 0, half 1, pk_add half 0, half 1} and the scalar instructions' results on the same operands
// (half 0: (a[i], b[i]), half 1: (a[i^1], b[i^1])).
__global__ void lpcn_arith_identity_kernel(const float *a, const float *b, uint32_t *out_mfma, uint32_t *out_mul, uint32_t *out_pk, uint32_t *out_sc)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    f4 negz = {-0.f, -0.f, -0.f, -0.f};
    asm volatile("" : "+v"(negz));                         // (the same guard as the kernel's: the addend must reach the instruction as -0.0)
    const float av = a[i], bv = b[i];
    const f4 p = __builtin_amdgcn_mfma_f32_4x4x1f32(av, bv, negz, 0, 0, 0);
    // (element-wise copies first: hipcc's __builtin_bit_cast of an ext-vector ELEMENT reads element 0 whatever the index)
    const float pe[4] = {p[0], p[1], p[2], p[3]};
    const size_t q = i & ~(size_t)3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ak = a[q + k], m;
        asm volatile("v_mul_f32 %0, %1, %2" : "=v"(m) : "v"(ak), "v"(bv));
        out_mfma[i * 4 + k] = __float_as_uint(pe[k]);
        out_mul[i * 4 + k] = __float_as_uint(m);
    }
    const float a2 = a[i ^ 1], b2 = b[i ^ 1];
    f2 x = {av, a2}, y = {bv, b2}, pm, pa;
    asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(pm) : "v"(x), "v"(y));
    asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(pa) : "v"(x), "v"(y));
    float m0, m1, s0, s1;
    asm volatile("v_mul_f32 %0, %1, %2" : "=v"(m0) : "v"(av), "v"(bv));
    asm volatile("v_mul_f32 %0, %1, %2" : "=v"(m1) : "v"(a2), "v"(b2));
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(s0) : "v"(av), "v"(bv));
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(s1) : "v"(a2), "v"(b2));
    const float pk0 = pm[0], pk1 = pm[1], pk2 = pa[0], pk3 = pa[1];
    out_pk[i * 4 + 0] = __float_as_uint(pk0); out_pk[i * 4 + 1] = __float_as_uint(pk1);
    out_pk[i * 4 + 2] = __float_as_uint(pk2); out_pk[i * 4 + 3] = __float_as_uint(pk3);
    out_sc[i * 4 + 0] = __float_as_uint(m0); out_sc[i * 4 + 1] = __float_as_uint(m1);
    out_sc[i * 4 + 2] = __float_as_uint(s0); out_sc[i * 4 + 3] = __float_as_uint(s1);
}

extern "C" int lpcn_debug_arith_identities(int device, const float *a, const float *b, uint32_t *out_mfma, uint32_t *out_mul,
                                           uint32_t *out_pk, uint32_t *out_sc, size_t n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "no such HIP device"); return LPCN_E_NODEVICE; }
    if (!n || n % 64) { snprintf(g_err, sizeof(g_err), "operand count must be a positive multiple of 64"); return LPCN_E_ARG; }
    DeviceGuard guard(device);
    DevBuf<float> d_in;
    DevBuf<uint32_t> d_out;
    int rc = 0;
    if ((rc = d_in.alloc(2 * n)) || (rc = d_out.alloc(16 * n))) return rc;
    if (hipMemcpy(d_in, a, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in + n, b, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = LPCN_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(lpcn_arith_identity_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, 0, (const float *)d_in, (const float *)(d_in + n),
                           d_out, d_out + 4 * n, d_out + 8 * n, d_out + 12 * n);
        uint32_t *const dst[4] = {out_mfma, out_mul, out_pk, out_sc};
        if (hipGetLastError() != hipSuccess) rc = LPCN_E_HIP;
        for (int k = 0; k < 4 && !rc; ++k)
            if (hipMemcpy(dst[k], d_out + (size_t)k * 4 * n, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = LPCN_E_HIP;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "arithmetic identity test kernel failed");
    return rc;
}

// test seam: the state re-quantisation of the int8 kernels.  The reference computes (int)floor(.5 + t) with t = 127 x rounded to float and the
// sum in DOUBLE (src/vec.h:311-316: exact, 0.5 + t needs at most 31 bits); the kernels use ONE instruction, v_cvt_rpi_i32_f32 ("round to
// nearest, ties toward +infinity" = floor(t + 0.5) evaluated exactly), when LPCN_QUANT_RPI is set.  This sweep compares both on ALL 2^32 bit
// patterns: out[0] = mismatches among the finite t with |t| < 2^31, out[1] = mismatches inside the reachable range |t| <= 127.5 (|x| <= 1),
// out[2] = one mismatching bit pattern (if any).
__global__ void lpcn_quant_sweep_kernel(unsigned long long *out)
{
    const uint32_t base = (blockIdx.x * blockDim.x + threadIdx.x) * 256u;
    unsigned bad = 0, bad_in = 0;
    for (uint32_t k = 0; k < 256u; ++k) {
        const uint32_t u = base + k;
        const float t = __uint_as_float(u);
        if (!(fabsf(t) < 2147483648.f)) continue;            // NaN, infinities and |t| >= 2^31: the C conversion is undefined there
        const int want = (int)floor(.5 + (double)t);
        int got;
        asm volatile("v_cvt_rpi_i32_f32 %0, %1" : "=v"(got) : "v"(t));
        if (got != want) { ++bad; if (fabsf(t) <= 127.5f) ++bad_in; out[2] = u; }
    }
    if (bad) atomicAdd(&out[0], (unsigned long long)bad);
    if (bad_in) atomicAdd(&out[1], (unsigned long long)bad_in);
}

extern "C" int lpcn_debug_quant_sweep(int device, unsigned long long *out3)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { snprintf(g_err, sizeof(g_err), "no such HIP device"); return LPCN_E_NODEVICE; }
    DeviceGuard guard(device);
    DevBuf<unsigned long long> d;
    int rc = d.alloc(3);
    if (rc) return rc;
    if (hipMemset(d, 0, 3 * sizeof(unsigned long long)) != hipSuccess) rc = LPCN_E_HIP;
    if (!rc) {
        hipLaunchKernelGGL(lpcn_quant_sweep_kernel, dim3(65536), dim3(256), 0, 0, d.p);      // 2^16 x 2^8 threads x 2^8 patterns
        if (hipGetLastError() != hipSuccess || hipMemcpy(out3, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) rc = LPCN_E_HIP;
    }
    if (rc) snprintf(g_err, sizeof(g_err), "quantisation sweep kernel failed");
    return rc;
}
