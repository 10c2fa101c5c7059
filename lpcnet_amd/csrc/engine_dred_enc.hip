// Device runtime, DRED encoder unit: the encoder's upload, a batch's per-stream state records and the one launch that encodes every active stream's
// double frames of a call (rdovae_enc_kernels.hip.h).  The records are a per-stream array of the batch: resets (engine.hip) and stream
// copies (engine_roster.hip) treat them like the others.
#include "engine_core.h"
#include "rdovae_enc_kernels.hip.h"
#include "rdovae_enc_fast_kernels.hip.h"
#include "lpcnet_tables_gen.h"

static constexpr size_t DENC_LDS_MAX = 160 * 1024;

// ---- the engine's part: a host copy of the blob's arrays now, the upload when a batch first enables the encoder
int denc_engine_init(lpcn_engine *e, const lpcn_model_host *m)
{
    e->denc_present = m->dred_enc.present;
    e->denc_servable = lpcn_dred_enc_servable(m) != 0;
    if (!e->denc_servable) return 0;
    auto h = std::make_unique<DredEncHostModel>();
    h->m = m->dred_enc;
    lpcn_dred_enc_model &d = h->m;
    h->a.take({&d.dense[0], &d.dense[1], &d.dense[2], &d.dense[3], &d.dense[4], &d.bits, &d.gdense[0], &d.gdense[1]}, d.gru, 3, m->dred_enc.present == 2);
    e->denc_host = std::move(h);
    return 0;
}

// the arrays as they are, the GRUs through upload_gru (engine_core.h) in the blob's flavour (W = int: an int8 blob's); then the block itself, which the
// kernel reads from device memory
template <typename W>
static int denc_upload_net(lpcn_engine *e, lpcn::DredEncNetT<W> &net, const lpcn::DredEncNetT<W> **d_net)
{
    const lpcn_dred_enc_model &d = e->denc_host->m;
    lpcn::DredEncNetT<W> n{};
    int rc = 0, off[9] = {0};
    n.latent_dim = d.latent_dim; n.state_dim = d.state_dim; n.taps = d.taps; n.gd1 = d.gdense1;
    for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + d.width[k];
    n.total = off[8];
    auto up_dense = [&](const lpcn_dense_layer &s, lpcn::DredStepT<W> &o, int x, int out) {
        o.gru = 0; o.n_in = s.n_in; o.n_out = s.n_out; o.x = x; o.out = out;
        int r = upload<float>(e, &o.w, s.w, (size_t)s.n_in * s.n_out);
        return r ? r : upload<float>(e, &o.b, s.b, s.n_out);
    };
    static const int dense_at[5] = {0, 2, 4, 6, 7}, gru_at[3] = {1, 3, 5};
    for (int k = 0; k < 5; ++k) if ((rc = up_dense(d.dense[k], n.step[dense_at[k]], dense_at[k] ? off[dense_at[k] - 1] : -1, off[dense_at[k]]))) return rc;
    for (int g = 0; g < 3; ++g) {
        const lpcn_gru_layer &G = d.gru[g];
        lpcn::DredStepT<W> &o = n.step[gru_at[g]];
        lpcn::GruLayer<W> L{};
        if ((rc = upload_gru(e, L, G))) return rc;
        o.gru = 1; o.n_in = L.n_in; o.n_out = L.n; o.x = off[gru_at[g] - 1]; o.out = off[gru_at[g]];
        o.gw = L.w; o.rec = L.rec; o.b = L.bias; o.start = L.start; o.pos = L.pos;
        n.max_gru = G.n > n.max_gru ? G.n : n.max_gru;
        n.gru_off[g] = off[gru_at[g]]; n.gru_n[g] = G.n; n.gru_floats += G.n;
    }
    if ((rc = up_dense(d.gdense[0], n.step[8], 0, n.total))) return rc;
    if ((rc = upload<float>(e, &n.bits_w, d.bits.w, (size_t)d.bits.n_in * d.bits.n_out)) || (rc = upload<float>(e, &n.bits_b, d.bits.b, d.bits.n_out)) ||
        (rc = upload<float>(e, &n.g2_w, d.gdense[1].w, (size_t)d.gdense1 * d.state_dim)) || (rc = upload<float>(e, &n.g2_b, d.gdense[1].b, d.state_dim)) ||
        (rc = upload<float>(e, &n.tansig, lpcn_tansig, 201))) return rc;
    if ((rc = upload<lpcn::DredEncNetT<W>>(e, d_net, &n, 1))) return rc;
    net = n;
    if constexpr (std::is_same<W, float>::value) {       // (what the FAST image is packed from outlives the host copy: denc_fast_upload)
        auto f = std::make_unique<DredFastHost>();
        for (int g = 0; g < 3; ++g) {
            const lpcn_gru_layer &G = d.gru[g];
            f->w[g].assign(G.w, G.w + 32 * (size_t)G.nb);
            f->idx[g].assign(G.idx, G.idx + 3 * G.n / 8 + G.nb);
            f->n_in[g] = G.n_in; f->n[g] = G.n;
        }
        e->denc_fast_host = std::move(f);
    }
    e->denc_host.reset();
    return 0;
}

// the uploaded block's figures, whichever flavour it is (a served encoder is in the blob's own): everything but the weights is the same in both
static size_t denc_lds_bytes(const lpcn_engine *e, int S) { return (size_t)(e->is_int8 ? lpcn::rdovae_enc_lds_floats(e->dencq, S) : lpcn::rdovae_enc_lds_floats(e->denc, S)) * sizeof(float); }
struct DencDims { int latent_dim, state_dim, taps, total, gru_floats, rec; };
static DencDims denc_dims(const lpcn_engine *e)
{
    if (e->is_int8) return {e->dencq.latent_dim, e->dencq.state_dim, e->dencq.taps, e->dencq.total, e->dencq.gru_floats, lpcn::rdovae_enc_rec_floats(e->dencq)};
    return {e->denc.latent_dim, e->denc.state_dim, e->denc.taps, e->denc.total, e->denc.gru_floats, lpcn::rdovae_enc_rec_floats(e->denc)};
}
static bool denc_form_fits(const lpcn_engine *e, int S) { return denc_lds_bytes(e, S) <= DENC_LDS_MAX; }
template <int S, typename W>
static auto denc_kernel() { if constexpr (std::is_same<W, float>::value) return lpcn::rdovae_enc_kernel<S>; else return lpcn::rdovae_enc_i8_kernel<S>; }

// the dynamic-LDS limit of a form, raised when a batch enables the encoder: a launch sets nothing, so it can be captured
template <int S>
static int denc_prepare_form(const lpcn_engine *e)
{
    if (!denc_form_fits(e, S)) return 0;
    const void *kernel = e->is_int8 ? (const void *)denc_kernel<S, int>() : (const void *)denc_kernel<S, float>();
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)denc_lds_bytes(e, S)));
    return 0;
}

extern "C" int lpcn_batch_dev_dred_enc_enabled(const lpcn_batch_dev *b) { return b->denc ? b->denc->max_dframes : 0; }

extern "C" int lpcn_batch_dev_dred_enc_enable(lpcn_batch_dev *b, int max_dframes)
{
    lpcn_engine *e = b->e;
    if (e->denc_present == 0) { snprintf(g_err, sizeof(g_err), "the model blob has no DRED encoder (enc_dense1..8_*, bits_dense_*, gdense1_*, gdense2_*)"); return LPCN_E_MODEL; }
    if (e->denc_present != 1 && e->denc_present != 2) { snprintf(g_err, sizeof(g_err), "the blob's DRED encoder arrays are incomplete, mix float and int8, or do not fit together (widths up to %d, enc_dense1 with %d inputs, 1 to %d taps of bits_dense)", LPCN_DRED_MAX_UNITS, LPCN_DRED_ENC_IN, LPCN_DRED_ENC_MAX_TAPS); return LPCN_E_MODEL; }
    if (!e->denc_servable && e->denc_present == 2) { snprintf(g_err, sizeof(g_err), "the blob's DRED encoder is int8 (DOT_PROD) but its LPCNet model is float: int8 encoder arrays are served beside an int8 model"); return LPCN_E_MODEL; }
    if (!e->denc_servable) { snprintf(g_err, sizeof(g_err), "the blob's DRED encoder is float but its LPCNet model is int8: float encoder arrays are served beside a float model"); return LPCN_E_MODEL; }
    if (max_dframes < 1 || (long long)max_dframes * 2 * b->n > 0x7fffffffLL / 256) { snprintf(g_err, sizeof(g_err), "DRED encoder: max_dframes must be at least 1 (and the batch's rows fit an int)"); return LPCN_E_ARG; }
    DeviceGuard guard(e->device);
    int rc = wait_all(b);
    if (rc) return rc;
    if (e->denc_host && (rc = e->is_int8 ? denc_upload_net<int>(e, e->dencq, &e->d_dencq) : denc_upload_net<float>(e, e->denc, &e->d_denc))) return rc;
    if (!denc_form_fits(e, 1)) { snprintf(g_err, sizeof(g_err), "DRED encoder: the encoder's buffers do not fit the LDS"); return LPCN_E_MODEL; }
    if ((rc = denc_prepare_form<1>(e)) || (rc = denc_prepare_form<2>(e)) || (rc = denc_prepare_form<4>(e)) || (rc = denc_prepare_form<8>(e))) return rc;
    if (!b->denc) {
        auto p = std::make_unique<lpcn_denc_host>();
        p->rec = (size_t)denc_dims(e).rec;
        if ((rc = p->state.alloc(p->rec * b->n)) || (rc = p->d_cnt.alloc((size_t)b->n)) || (rc = p->h_cnt.reserve(sizeof(int) * (size_t)b->n))) return rc;
        HIP_TRY(hipMemsetAsync(p->state, 0, sizeof(float) * p->rec * b->n, e->stream));      // (DRED_rdovae_init_encoder; done before the call returns: the first
        HIP_TRY(hipStreamSynchronize(e->stream));                                            //  encode may go to any stream)
        if (hipEventCreateWithFlags(&p->ev_cnt.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED encoder: hipEventCreate failed"); return LPCN_E_HIP; }
        b->denc = std::move(p);
    }
    b->denc->max_dframes = max_dframes;
    b->denc->cus = device_cus(e);
    return 0;
}
#define NEED_DENC(b) do { if (!(b)->denc) { snprintf(g_err, sizeof(g_err), "the DRED encoder is not enabled on this batch (lpcnet_batch_dred_enc_enable)"); return LPCN_E_MODEL; } } while (0)

extern "C" int lpcn_batch_dev_dred_enc_flavour(const lpcn_batch_dev *b)
{
    NEED_DENC(b);
    return b->e->is_int8 ? 1 : 0;
}

extern "C" int lpcn_batch_dev_dred_enc_info(const lpcn_batch_dev *b, int *info)
{
    NEED_DENC(b);
    const DencDims P = denc_dims(b->e);
    info[0] = b->denc->max_dframes; info[1] = LPCN_DRED_ENC_IN; info[2] = P.latent_dim; info[3] = P.state_dim; info[4] = P.taps; info[5] = P.total;
    info[6] = P.gru_floats + (P.taps - 1) * P.total;
    return 0;
}

// ---- streams per workgroup.  The table is the decoder's (engine_dred.hip): a workgroup's time per double frame is set by its dependent add chains, not
// by how many streams it carries, so the fewest streams per workgroup that still put the streams on the CUs in one round, eight beyond that -- among
// the forms whose buffers fit the LDS.  Measured in profiles/dred_enc_rate.json, and for an int8 blob's encoder, which shares the
// table, in profiles/dred_enc_i8_rate.json (§4.8).
extern "C" int lpcn_batch_dev_dred_enc_form(const lpcn_batch_dev *b, int n)
{
    NEED_DENC(b);
    int S = b->denc->form;
    if (!S) {
        const int cus = b->denc->cus;
        for (S = 1; S < 8 && (n + S - 1) / S > cus; S *= 2) {}
        while (S > 1 && !denc_form_fits(b->e, S)) S /= 2;      // (widths the widest form's buffers do not fit)
    }
    return S;
}
extern "C" int lpcn_batch_dev_dred_enc_set_form(lpcn_batch_dev *b, int S)
{
    NEED_DENC(b);
    if (S != 0 && S != 1 && S != 2 && S != 4 && S != 8) { snprintf(g_err, sizeof(g_err), "DRED encoder form: 1, 2, 4 or 8 streams per workgroup, 0 = the table's choice"); return LPCN_E_ARG; }
    if (S && !denc_form_fits(b->e, S)) { snprintf(g_err, sizeof(g_err), "DRED encoder form: the buffers of %d streams (%zu bytes) do not fit a workgroup's LDS", S, denc_lds_bytes(b->e, S)); return LPCN_E_ARG; }
    b->denc->form = S;
    return 0;
}

// ---- the FAST flavour (rdovae_enc_fast_kernels.hip.h): the float encoder in the arithmetic of the reference's AVX2+FMA build, the
// streams of a workgroup on the columns of an fp32 MFMA.  Its image of the GRUs' sparse input matrices is the decoder's format, packed on the host
// (dred_fast_pack.h) and uploaded when a batch first asks for FAST; the host copy of those matrices goes then.  The other arrays are the PARITY block's.
static int denc_fast_upload(lpcn_engine *e)
{
    if (e->d_denc_fast) return 0;
    if (!e->denc_fast_host) { snprintf(g_err, sizeof(g_err), "DRED encoder FAST: the encoder's host arrays are gone"); return LPCN_E_MODEL; }
    const int rc = dred_fast_image_upload(e, *e->denc_fast_host, &e->d_denc_fast, "DRED encoder FAST");
    if (rc) return rc;
    e->denc_fast_host.reset();
    return 0;
}
// (a kilobyte is left to the kernel's static LDS)
static bool denc_fast_fits(const lpcn_engine *e, int T)
{
    return lpcn::rdovae_enc_fast_tiles_fit(e->denc) && (size_t)lpcn::rdovae_enc_fast_lds_floats(e->denc, T) * sizeof(float) <= DENC_LDS_MAX - 1024;
}
// The tile a FAST launch over n streams runs with: the pinned one, or the engine's choice (mode 1).  The rule is read off
// profiles/dred_enc_fast_rate.json, and it is the decoder's: a tile's chain takes the same time whether it carries 16 or 32 streams,
// so T = 16 while its tiles fit the CUs in one round and T = 32 beyond -- among the tiles whose buffers fit the LDS.  The bits of a stream are the
// same in both
static int denc_fast_tile(const lpcn_batch_dev *b, int n)
{
    const lpcn_denc_host *p = b->denc.get();
    if (p->fast != 1) return p->fast;
    const int T = (n + 15) / 16 <= p->cus ? 16 : 32;
    return denc_fast_fits(b->e, T) ? T : 16;
}
template <int T, int U>
static int denc_fast_prepare(const lpcn_engine *e)
{
    if (!denc_fast_fits(e, T)) return 0;
    HIP_TRY(hipFuncSetAttribute((const void *)lpcn::rdovae_enc_fast_kernel<T, U>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lpcn::rdovae_enc_fast_lds_floats(e->denc, T) * (int)sizeof(float)));
    return 0;
}
extern "C" int lpcn_batch_dev_dred_enc_get_fast(const lpcn_batch_dev *b)
{
    NEED_DENC(b);
    return b->denc->fast;
}
extern "C" int lpcn_batch_dev_dred_enc_set_fast(lpcn_batch_dev *b, int mode)
{
    NEED_DENC(b);
    lpcn_engine *e = b->e;
    if (mode != 0 && mode != 1 && mode != 16 && mode != 32) { snprintf(g_err, sizeof(g_err), "DRED encoder FAST: 0 = off, 1 = the engine's tile, 16 or 32 = that many streams per workgroup (the tiles that are built)"); return LPCN_E_ARG; }
    if (e->is_int8 && mode) { snprintf(g_err, sizeof(g_err), "DRED encoder FAST: the int8 encoder has no FAST form yet"); return LPCN_E_MODEL; }
    if (mode) {
        // a pinned tile must fit; mode 1 falls back to 16 streams where 32 do not fit
        if (!denc_fast_fits(e, mode == 32 ? 32 : 16)) {
            snprintf(g_err, sizeof(g_err), "DRED encoder FAST: the encoder's tile of %d streams (%zu bytes, bits_dense and gdense1 in at most %d tiles of 32 rows) does not fit a workgroup",
                     mode == 32 ? 32 : 16, (size_t)lpcn::rdovae_enc_fast_lds_floats(e->denc, mode == 32 ? 32 : 16) * sizeof(float), lpcn::ENC_FAST_TRAIL_WAVES * lpcn::ENC_FAST_SLOTS);
            return LPCN_E_MODEL;
        }
        DeviceGuard guard(e->device);
        int rc = wait_all(b);
        // (the dynamic-LDS limits are raised here, not at a launch: a launch sets nothing, so it can be captured)
        if (rc || (rc = denc_fast_upload(e)) || (rc = denc_fast_prepare<16, 16>(e)) || (rc = denc_fast_prepare<32, 8>(e))) return rc;
    }
    b->denc->fast = mode;
    return 0;
}
template <int T, int U>
static void denc_fast_launch(const lpcn_batch_dev *b, hipStream_t st, const int *d_cnt, int uniform, const float *d_feat, int stride, float *d_lat, float *d_init)
{
    const int lds = lpcn::rdovae_enc_fast_lds_floats(b->e->denc, T) * (int)sizeof(float);
    hipLaunchKernelGGL((lpcn::rdovae_enc_fast_kernel<T, U>), dim3((b->active + T - 1) / T), dim3(lpcn::ENC_FAST_THREADS), lds, st, b->e->d_denc, b->e->d_denc_fast, b->active,
                       b->denc->max_dframes, d_cnt, uniform, d_feat, stride, (float *)b->denc->state, d_lat, d_init);
}

// count in 0 .. max_dframes and zero beyond the active prefix (count == NULL: n_dframes for every active stream); stride >= 20
extern "C" int lpcn_batch_dev_dred_enc_check(const lpcn_batch_dev *b, const int *count, int n_dframes, int stride)
{
    NEED_DENC(b);
    if (stride < LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "DRED encode: the feature stride must be at least %d", LPCN_NB_FEAT); return LPCN_E_ARG; }
    if (!count) {
        if (n_dframes < 0 || n_dframes > b->denc->max_dframes) { snprintf(g_err, sizeof(g_err), "DRED encode: a count outside 0 .. %d", b->denc->max_dframes); return LPCN_E_ARG; }
        return 0;
    }
    for (int s = 0; s < b->n; ++s) {
        if (count[s] < 0 || count[s] > b->denc->max_dframes) { snprintf(g_err, sizeof(g_err), "DRED encode: stream %d has a count outside 0 .. %d", s, b->denc->max_dframes); return LPCN_E_ARG; }
        if (s >= b->active && count[s] != 0) { snprintf(g_err, sizeof(g_err), "DRED encode: stream %d is not active and has a count", s); return LPCN_E_ARG; }
    }
    return 0;
}

template <int S>
static void denc_launch_form(const lpcn_batch_dev *b, hipStream_t st, const int *d_cnt, int uniform, const float *d_feat, int stride, float *d_lat, float *d_init)
{
    const int grid = (b->active + S - 1) / S, lds = (int)denc_lds_bytes(b->e, S);
    if (b->e->is_int8)
        hipLaunchKernelGGL(lpcn::rdovae_enc_i8_kernel<S>, dim3(grid), dim3(lpcn::DRED_THREADS), lds, st, b->e->d_dencq, b->active, b->denc->max_dframes, d_cnt,
                           uniform, d_feat, stride, (float *)b->denc->state, d_lat, d_init);
    else
        hipLaunchKernelGGL(lpcn::rdovae_enc_kernel<S>, dim3(grid), dim3(lpcn::DRED_THREADS), lds, st, b->e->d_denc, b->active, b->denc->max_dframes, d_cnt, uniform,
                           d_feat, stride, (float *)b->denc->state, d_lat, d_init);
}

// checks, the counts' upload through the pinned buffer (none for the uniform form), one launch
static int denc_enqueue(lpcn_batch_dev *b, const float *d_feat, int stride, const int *count, int n_dframes, float *d_lat, float *d_init, hipStream_t st)
{
    int rc = lpcn_batch_dev_dred_enc_check(b, count, n_dframes, stride);
    if (rc) return rc;
    bool any = !count && n_dframes > 0 && b->active > 0;
    for (int s = 0; count && s < b->active; ++s) any |= count[s] > 0;
    if (!any) return 0;
    if (!d_feat || !d_lat || !d_init) { snprintf(g_err, sizeof(g_err), "bad DRED encode arguments"); return LPCN_E_ARG; }
    lpcn_denc_host *p = b->denc.get();
    if (count && stream_is_capturing(st)) { snprintf(g_err, sizeof(g_err), "a DRED encode with a count array cannot be captured: its launch depends on the host's array (count = NULL with n_dframes can)"); return LPCN_E_ARG; }
    if ((rc = order_begin(b, st))) return rc;
    if (count) {
        if (p->cnt_pending) { HIP_TRY(hipEventSynchronize(p->ev_cnt)); p->cnt_pending = false; }      // (the previous call's counts have left the pinned buffer)
        memcpy(p->h_cnt.p, count, sizeof(int) * (size_t)b->active);
        HIP_TRY(hipMemcpyAsync(p->d_cnt, p->h_cnt.p, sizeof(int) * (size_t)b->active, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(p->ev_cnt, st));
        p->cnt_pending = true;
    }
    const int *d_cnt = count ? (const int *)p->d_cnt : nullptr;
    if (p->fast) {
        if (denc_fast_tile(b, b->active) == 16) denc_fast_launch<16, 16>(b, st, d_cnt, n_dframes, d_feat, stride, d_lat, d_init);
        else denc_fast_launch<32, 8>(b, st, d_cnt, n_dframes, d_feat, stride, d_lat, d_init);
    } else switch (lpcn_batch_dev_dred_enc_form(b, b->active)) {
    case 1: denc_launch_form<1>(b, st, d_cnt, n_dframes, d_feat, stride, d_lat, d_init); break;
    case 2: denc_launch_form<2>(b, st, d_cnt, n_dframes, d_feat, stride, d_lat, d_init); break;
    case 4: denc_launch_form<4>(b, st, d_cnt, n_dframes, d_feat, stride, d_lat, d_init); break;
    default: denc_launch_form<8>(b, st, d_cnt, n_dframes, d_feat, stride, d_lat, d_init); break;
    }
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED encode: kernel launch failed"); return LPCN_E_HIP; }
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_dred_encode(lpcn_batch_dev *b, const float *d_features, int stride, const int *count, int n_dframes, float *d_latents,
                                          float *d_initial, void *hip_stream)
{
    NEED_DENC(b);
    DeviceGuard guard(b->e->device);
    return denc_enqueue(b, d_features, stride, count, n_dframes, d_latents, d_initial, hip_stream ? (hipStream_t)hip_stream : b->e->stream);
}

// host pointers: the active streams' rows in, one launch, the outputs down whole and out to the caller row by row
extern "C" int lpcn_batch_dev_dred_encode_host(lpcn_batch_dev *b, const float *features, int stride, const int *count, float *latents, float *initial)
{
    NEED_DENC(b);
    if (!count) { snprintf(g_err, sizeof(g_err), "bad DRED encode arguments"); return LPCN_E_ARG; }
    int rc = lpcn_batch_dev_dred_enc_check(b, count, 0, stride);
    if (rc) return rc;
    if (!features || !latents || !initial) { snprintf(g_err, sizeof(g_err), "bad DRED encode arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    lpcn_denc_host *p = b->denc.get();
    const DencDims P = denc_dims(b->e);
    hipStream_t st = b->e->stream;
    const size_t n = (size_t)b->active, per_f = 2 * (size_t)p->max_dframes * stride, per_l = (size_t)p->max_dframes * P.latent_dim,
                 per_i = (size_t)p->max_dframes * P.state_dim;
    if ((rc = p->d_feat.reserve(b, (size_t)b->n * per_f)) || (rc = p->d_lat.reserve(b, (size_t)b->n * per_l)) || (rc = p->d_init.reserve(b, (size_t)b->n * per_i)) ||
        (rc = p->h_out.reserve(sizeof(float) * (size_t)b->n * (per_l + per_i)))) return rc;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(p->d_feat, features, sizeof(float) * n * per_f, hipMemcpyHostToDevice, st));
    if ((rc = denc_enqueue(b, p->d_feat, stride, count, 0, p->d_lat, p->d_init, st))) return rc;
    float *h_lat = (float *)p->h_out.p, *h_init = h_lat + n * per_l;
    HIP_TRY(hipMemcpyAsync(h_lat, p->d_lat, sizeof(float) * n * per_l, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_init, p->d_init, sizeof(float) * n * per_i, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t s = 0; s < n; ++s) {
        memcpy(latents + s * per_l, h_lat + s * per_l, sizeof(float) * P.latent_dim * (size_t)count[s]);
        memcpy(initial + s * per_i, h_init + s * per_i, sizeof(float) * P.state_dim * (size_t)count[s]);
    }
    return 0;
}

// ---- one stream's state in the reference's member order (RDOVAEEncState: dense2_state, dense4_state, dense6_state, bits_dense_state -- the oldest tap
// first): the record with its ring turned so that the head is slot 0
extern "C" int lpcn_batch_dev_dred_enc_get_state(lpcn_batch_dev *b, int s, float *out)
{
    NEED_DENC(b);
    lpcn_denc_host *p = b->denc.get();
    const DencDims P = denc_dims(b->e);
    if (!out) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    std::vector<float> r(p->rec);
    int rc = stream_rec(b, s, p->state, p->rec, r.data(), nullptr);
    if (rc) return rc;
    int head = 0;
    memcpy(&head, &r[p->rec - 1], sizeof(int));
    memcpy(out, r.data(), sizeof(float) * P.gru_floats);
    for (int i = 0; i < P.taps - 1; ++i)
        memcpy(out + P.gru_floats + (size_t)i * P.total, &r[P.gru_floats + (size_t)((head + i) % (P.taps - 1)) * P.total], sizeof(float) * P.total);
    return 0;
}
extern "C" int lpcn_batch_dev_dred_enc_set_state(lpcn_batch_dev *b, int s, const float *in)
{
    NEED_DENC(b);
    lpcn_denc_host *p = b->denc.get();
    if (!in) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    std::vector<float> r(p->rec, 0.f);      // (head 0: the ring as the caller gave it)
    memcpy(r.data(), in, sizeof(float) * (p->rec - 1));
    return stream_rec(b, s, p->state, p->rec, nullptr, r.data());
}
