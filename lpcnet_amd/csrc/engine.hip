// Device runtime of the LPCNet HIP engine, first unit: model upload, batch lifetime, ordering across caller streams, the cost table.  The launches
// are in engine_synth.hip, engine_codec.hip, engine_plc.hip and engine_probe.hip; what the units share is in engine_core.h.
// Only the C ABI of lpcnet_engine.h is visible to the C host shell.
// Device and pinned memory is held by owning types (DevBuf, PinBuf; engine_core.h): a buffer is freed when its owner goes and grows in one place
// (DevBuf::reserve, which first waits for the batch's enqueued work).  Kernels and launch helpers take raw pointers, filled from the owners.
#include "engine_core.h"
#include "lpcnet_tables_gen.h"
#include "sample_variants.h"
#include <math.h>

__thread char g_err[512] = "";
extern "C" const char *lpcn_last_error(void) { return g_err; }

bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return st != nullptr && hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
// (while the caller's stream is being captured into a HIP graph nothing is executed: the batch's event chain is left alone -- an event
// recorded inside a capture cannot be waited for from the host -- and ordering replays against other work on the batch is the caller's job)
int order_begin(lpcn_batch_dev *b, hipStream_t st)
{
    if (stream_is_capturing(st)) return 0;
    if (b->pending && st != b->last_stream) HIP_TRY(hipStreamWaitEvent(st, b->ev_last, 0));
    return 0;
}
int order_end(lpcn_batch_dev *b, hipStream_t st)
{
    if (stream_is_capturing(st)) return 0;
    HIP_TRY(hipEventRecord(b->ev_last, st));
    b->last_stream = st;
    b->pending = true;
    return 0;
}
// host-side wait for everything enqueued for this batch, whichever stream it went to
int wait_all(lpcn_batch_dev *b)
{
    if (b->pending) { HIP_TRY(hipEventSynchronize(b->ev_last)); b->pending = false; }
    HIP_TRY(hipStreamSynchronize(b->e->stream));
    return 0;
}

// compiled item counts per lane (sample_variants.h), zero-terminated: fp32 items are 4 VGPRs each, int8 items 1 VGPR
#define LPCN_LIST_ITEM(n) n,
static const int variants_f32[] = {LPCN_VARIANTS_F32(LPCN_LIST_ITEM) 0};
static const int variants_i8[] = {LPCN_VARIANTS_I8(LPCN_LIST_ITEM) 0};
static const int variants_x2[] = {LPCN_VARIANTS_X2(LPCN_LIST_ITEM) 0};
static const int variants_x2w[] = {LPCN_VARIANTS_X2W(LPCN_LIST_ITEM) 0};
#undef LPCN_LIST_ITEM
// the smallest compiled variant that holds nw items per lane (0: none does)
static int round_up_variant(const int *v, int nw) { for (; *v; ++v) if (nw <= *v) return *v; return 0; }

// the PLC network in the blob's flavour: the dense layers as they are, the two GRUs through upload_gru (engine_core.h)
template <typename W>
static int plc_upload_net(lpcn_engine *e, const lpcn_plc_model *p, lpcn::PlcNetT<W> &n)
{
    n.d1 = p->dense1.n_out;
    int rc = 0;
#define UPP(field, src, count) if ((rc = upload<float>(e, &n.field, src, (size_t)(count)))) return rc
    UPP(dense1_w, p->dense1.w, LPCN_PLC_IN * n.d1); UPP(dense1_b, p->dense1.b, n.d1);
    UPP(out_w, p->out.w, LPCN_NB_FEAT * p->out.n_in); UPP(out_b, p->out.b, LPCN_NB_FEAT);
    UPP(tansig, lpcn_tansig, 201);
#undef UPP
    for (int g = 0; g < 2; ++g) if ((rc = upload_gru(e, n.gru[g], p->gru[g]))) return rc;
    return 0;
}

// GRU-A as dealt to waves and lanes (model_pack.c) + the embedding tables in that lane order: everything that depends on the dealing.  `a`: the
// PARITY image's block, for what does not
static int upload_gru_a(lpcn_engine *e, const LpcnSampleArgs &a, const lpcn_model_host *mm, GruAImage &img, int nwv_)
{
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
}

// the embedding tables in the blob's own [256][1152] order: the start-value pass of the two-group kernel, their only reader
static int upload_nat_tables(lpcn_engine *e, LpcnSampleArgs &ax, const float *sig, const float *pred, const float *exc)
{
    int rc = upload<float>(e, &ax.emb_nat_sig, sig, (size_t)256 * LPCN_ROWS_A);
    if (!rc) rc = upload<float>(e, &ax.emb_nat_pred, pred, (size_t)256 * LPCN_ROWS_A);
    if (!rc) rc = upload<float>(e, &ax.emb_nat_exc, exc, (size_t)256 * LPCN_ROWS_A);
    return rc;
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
    if ((rc = upload_gru_a(e, a, m, e->image[IMG_PARITY], nwv))) return fail(rc);
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
                rc = upload_gru_a(e, a, &mx, e->image[IMG_X2], nwx);
                if (!rc) rc = upload_nat_tables(e, e->image[IMG_X2].args, m->emb_sig, m->emb_pred, m->emb_exc);
            }
            lpcn_model_release(&mx);
            if (rc) return fail(rc);
        } else {
            // more than 32 items per lane: the STREAMED variants' image (lpcn_model_pack_x2_wide) is dealt and checked here, on the host, and kept
            // with a copy of the tables; the first batch that asks (lpcn_batch_dev_set_x2_streamed) uploads it as IMG_X2
            auto wh = std::make_unique<X2WideHost>();
            if (lpcn_model_pack_x2_wide(m, &wh->mx) == 0) {
                wh->packed = true;
                wh->mx.pk_b_w = m->pk_b_w; wh->mx.pk_b_start = m->pk_b_start; wh->mx.pk_b_blk = m->pk_b_blk;
                const int stw = lpcn_model_selftest(&wh->mx);
                wh->mx.pk_b_w = nullptr; wh->mx.pk_b_start = nullptr; wh->mx.pk_b_blk = nullptr;
                if (stw == 0 && round_up_variant(variants_x2w, wh->mx.nw)) {
                    const float *src[3] = {m->emb_sig, m->emb_pred, m->emb_exc};
                    for (int t = 0; t < 3; ++t) wh->emb[t].assign(src[t], src[t] + (size_t)256 * LPCN_ROWS_A);
                    e->x2w_host = std::move(wh);
                }
            }
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
            if (nwf) rc = upload_gru_a(e, a, &mf, e->image[IMG_FAST], nwf);
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
    if (e->plc_servable && (rc = m->is_int8 ? plc_upload_net(e, &m->plc, e->plcq) : plc_upload_net(e, &m->plc, e->plc))) return fail(rc);
    if ((rc = dred_engine_init(e, m))) return fail(rc);
    if ((rc = denc_engine_init(e, m))) return fail(rc);
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
int device_cus(const lpcn_engine *e)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0) return prop.multiProcessorCount;
    return 256;
}
static bool pack2_available(const lpcn_engine *e) { return e->is_int8 && gru_a_image(e, 4).nw_variant <= 32; }
bool use_pack2(const lpcn_batch_dev *b, int n, int S)
{
    // (S = 4 needs ~92 KB of LDS per workgroup: two do not fit a CU, and the 128-VGPR code alone is slower -- measured 119 vs 137 M)
    if (S > 2 || !pack2_available(b->e)) return false;
    if (b->pack2_force >= 0) return b->pack2_force == 1;
    return (n + S - 1) / S > device_cus(b->e);
}
int auto_streams_per_wg(const lpcn_batch_dev *b, int n)
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
    // (a wide image -- the streamed variants, a batch's opt-in -- is never the table's choice: at 2 048 streams eight against four was +17.3 % on
    // the 36-item model and -2.8 % at skew 0.1, EXPERIMENTS.md round 11 -- one sign per model; lpcnet_batch_tune and a pinned value select it)
    if (x2_available(b) && !e->x2_wide) {                    // eight streams per workgroup: a round of the two-group kernel (us per sample step)
        static const float step_x2 = 13.9f;
        const int wgs = (n + 7) / 8;
        const float t = (float)((wgs + cus - 1) / cus) * step_x2;
        // (FAST, a batch that opted in -- lpcn_batch_dev_set_x2_fast: eight at exactly the stream counts where PARITY gets eight, so the comparison is
        // PARITY's; the FAST form of the kernel has no step time of its own in this table)
        if (e->fast) {
            float t_par = 0.f;
            for (int k = 0; k < 3; ++k) {
                const int S = 1 << k, w = (n + S - 1) / S;
                const float tk = (float)((w + cus - 1) / cus) * step_f32[k];
                if (k == 0 || tk < t_par) t_par = tk;
            }
            if (t < t_par) best = 8;
        } else
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
    b->e = e; b->n = n; b->active = n; b->max_chunk = max_chunk;
    const char *off = getenv("LPCNET_HIP_NO_X2"), *force = getenv("LPCNET_HIP_PACK2");      // (read once per batch, never on the launch path)
    b->no_x2 = off && *off == '1'; b->pack2_force = (force && *force) ? *force == '1' : -1;
    const char *tw = getenv("LPCNET_HIP_X3");                // tools (profiles of one form under LPCNET_HIP_NO_AUTOTUNE): 1 = the twelve-wave form wherever the model has the image, 0 = never
    if (tw && *tw) { b->x3_mode = *tw == '1'; b->x3 = b->x3_mode == 1; }
    b->S = auto_streams_per_wg(b, n);
    b->pack2 = use_pack2(b, n, b->S);
    auto fail = [&](int code) { lpcn_batch_dev_destroy(b); return code; };
    const char *xs = getenv("LPCNET_HIP_X2_STREAMED");       // tools (bench.py on a trained-like model): the streamed two-group variants where the model allows, silently not where it does not
    if (xs && *xs == '1' && (e->x2w_host || e->x2_wide)) { const int rcs = lpcn_batch_dev_set_x2_streamed(b, 1); if (rcs) return fail(rcs); }
    const char *xf = getenv("LPCNET_HIP_X2_FAST");           // tools (bench.py --fast): the two-group kernel under FAST fp32 arithmetic where the model allows, silently not where it does not
    if (xf && *xf == '1' && x2_fast_servable(e)) { const int rcf = lpcn_batch_dev_set_x2_fast(b, 1); if (rcf) return fail(rcf); }
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
// (an inactive stream keeps its products and their flag: nothing advanced it)
void forget_keep(lpcn_batch_dev *b) { for (size_t s = 0; s < b->keep_ok.size() && s < (size_t)b->active; ++s) b->keep_ok[s] = 0; }
void forget_keep_all(lpcn_batch_dev *b) { b->keep_ok.assign(b->keep_ok.size(), 0); }
int check_range(const lpcn_batch_dev *b, int first, int count, const char *what)
{
    if (first < 0 || count < 0 || first + count > b->n) { snprintf(g_err, sizeof(g_err), "%s range", what); return LPCN_E_ARG; }
    return 0;
}

extern "C" int lpcn_batch_dev_reset(lpcn_batch_dev *b, int first, int count)
{
    forget_keep_all(b);
    if (check_range(b, first, count, "reset")) return LPCN_E_ARG;
    DeviceGuard guard(b->e->device);
    std::vector<lpcn_stream_state> h(count);
    for (auto &s : h) host_reset_state(&s);
    { int rcw = wait_all(b); if (rcw) return rcw; }
    HIP_TRY(hipMemcpy(b->d_state + first, h.data(), sizeof(lpcn_stream_state) * count, hipMemcpyHostToDevice));
    if (count) HIP_TRY(hipMemset(b->d_vq_mem + (size_t)first * LPCN_NB_BANDS, 0, sizeof(float) * (size_t)count * LPCN_NB_BANDS));
    if (count && b->denc) {            // (DRED_rdovae_init_encoder; done before the call returns: the next encode may go to any stream)
        HIP_TRY(hipMemsetAsync(b->denc->state + (size_t)first * b->denc->rec, 0, sizeof(float) * (size_t)count * b->denc->rec, b->e->stream));
        HIP_TRY(hipStreamSynchronize(b->e->stream));
    }
    return dred_state_reset(b, first, count);      // (DRED_rdovae_init_decoder, where the batch keeps the decoder's states)
}

extern "C" int lpcn_batch_dev_get_state(lpcn_batch_dev *b, int s, lpcn_stream_state *host) { return stream_rec(b, s, b->d_state, 1, host, nullptr); }
extern "C" int lpcn_batch_dev_set_state(lpcn_batch_dev *b, int s, const lpcn_stream_state *host)
{
    forget_keep_all(b);
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
    if (s == 8 && !x2_available(b)) { snprintf(g_err, sizeof(g_err), "eight streams per workgroup need a float blob with a dense GRU-B matrix and <= 32 items per lane (33 .. 96: lpcnet_batch_set_two_group_streaming first), PARITY arithmetic (FAST fp32: lpcnet_batch_set_fast_two_group first)"); return LPCN_E_ARG; }
    if (s != 1 && s != 2 && s != 4 && s != 8) { snprintf(g_err, sizeof(g_err), "streams per workgroup must be 1, 2, 4 or 8"); return LPCN_E_ARG; }
    b->S = s;
    b->pack2 = use_pack2(b, b->n, b->S);
    return 0;
}
// The streamed variants of the two-group kernel for THIS batch (float blobs of 33 .. 96 items per lane; off by default).  On: the engine's wide image
// is uploaded once, as IMG_X2, and the batch treats eight streams per workgroup like any two-group model -- pinned, measured, or the group
// schedule's answer; off: the batch is back on the four-stream kernel (the image stays).  A model with an ordinary two-group image: nothing to do.
extern "C" int lpcn_batch_dev_set_x2_streamed(lpcn_batch_dev *b, int on)
{
    lpcn_engine *e = b->e;
    if (e->image[IMG_X2].present && !e->x2_wide) return 0;
    if (e->is_int8) { snprintf(g_err, sizeof(g_err), "two-group streaming: int8 blobs have no two-group kernel"); return LPCN_E_MODEL; }
    if (!e->image[IMG_PARITY].args.b_dense) { snprintf(g_err, sizeof(g_err), "two-group streaming: the two-group kernel needs a dense GRU-B input matrix"); return LPCN_E_MODEL; }
    if (!e->x2_wide && !e->x2w_host) { snprintf(g_err, sizeof(g_err), "two-group streaming: the model has no two-group image (more than %d items per lane, or switched off when the engine was created)", LPCN_X2W_NW_MAX); return LPCN_E_MODEL; }
    if (!on && b->x2_streamed && !b->S_auto && b->S == 8) { snprintf(g_err, sizeof(g_err), "two-group streaming: eight streams per workgroup are pinned; pin another value first"); return LPCN_E_ARG; }
    if ((on != 0) == b->x2_streamed) return 0;
    DeviceGuard guard(e->device);
    { const int rcw = wait_all(b); if (rcw) return rcw; }
    if (on && !e->x2_wide) {
        X2WideHost &wh = *e->x2w_host;
        GruAImage img;
        int rc = upload_gru_a(e, e->image[IMG_PARITY].args, &wh.mx, img, round_up_variant(variants_x2w, wh.mx.nw));
        if (!rc) rc = upload_nat_tables(e, img.args, wh.emb[0].data(), wh.emb[1].data(), wh.emb[2].data());
        if (rc) return rc;                                   // (what was uploaded goes with the engine)
        e->image[IMG_X2] = img;
        e->x2_wide = true;
        e->x2w_host.reset();
    }
    b->x2_streamed = on != 0;
    return lpcn_batch_dev_retune(b);                         // (the engine's choice is made again, and measured again at the next run; a pinned value stays)
}
extern "C" int lpcn_batch_dev_x2_streamed(const lpcn_batch_dev *b) { return b->x2_streamed ? 1 : 0; }
// The two-group kernel under FAST fp32 arithmetic for THIS batch (off by default).  On: while the engine's flavour is FAST without the fp16 dual FC,
// eight streams per workgroup are available to the batch -- pinned, or the cost table's answer at the stream counts where PARITY gets eight (never a
// measurement: FAST is not timed); under PARITY and under the fp16 dual FC nothing that runs changes.  Needs the ordinary two-group image.
extern "C" int lpcn_batch_dev_set_x2_fast(lpcn_batch_dev *b, int on)
{
    lpcn_engine *e = b->e;
    if (e->is_int8) { snprintf(g_err, sizeof(g_err), "FAST two-group: int8 blobs have no two-group kernel"); return LPCN_E_MODEL; }
    if (!e->image[IMG_PARITY].args.b_dense) { snprintf(g_err, sizeof(g_err), "FAST two-group: the two-group kernel needs a dense GRU-B input matrix"); return LPCN_E_MODEL; }
    if (!x2_fast_servable(e)) { snprintf(g_err, sizeof(g_err), "FAST two-group: the model has no register-resident two-group image (more than %d items per lane, or switched off when the engine was created)", LPCN_X2_NW_MAX); return LPCN_E_MODEL; }
    if (!on && b->x2_fast && x2_fast_active(b) && !b->S_auto && b->S == 8) { snprintf(g_err, sizeof(g_err), "FAST two-group: eight streams per workgroup are pinned under FAST arithmetic; pin another value first"); return LPCN_E_ARG; }
    if ((on != 0) == b->x2_fast) return 0;
    DeviceGuard guard(e->device);
    { const int rcw = wait_all(b); if (rcw) return rcw; }
    b->x2_fast = on != 0;
    return lpcn_batch_dev_retune(b);                         // (the table's choice is made again; a pinned value stays)
}
extern "C" int lpcn_batch_dev_x2_fast(const lpcn_batch_dev *b) { return b->x2_fast ? 1 : 0; }
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
// The active prefix: host-only, no wait, no device work.  Calls enqueued before keep the count they were enqueued with (every launch takes its
// size as a value when it is enqueued); what follows works on streams [0, active).
extern "C" int lpcn_batch_dev_set_active(lpcn_batch_dev *b, int active)
{
    if (active < 0 || active > b->n) { snprintf(g_err, sizeof(g_err), "active streams: 0 .. %d", b->n); return LPCN_E_ARG; }
    b->active = active;
    return 0;
}
extern "C" int lpcn_batch_dev_active(const lpcn_batch_dev *b) { return b->active; }
extern "C" int lpcn_batch_dev_sync(lpcn_batch_dev *b)
{
    DeviceGuard guard(b->e->device);
    return wait_all(b);
}
