// Device runtime, DRED unit: the decoder's upload, a batch's scratch and the one launch that decodes every active stream's latent chain
// (dred_kernels.hip.h).  That call keeps nothing per stream between calls.  The init / step pair at the end of the file does
// (DESIGN.md §4.6b): its record is one of the batch's per-stream arrays, which resets, stream copies and snapshots carry.
#include "engine_core.h"
#include "dred_kernels.hip.h"
#include "dred_fast_kernels.hip.h"
#include "dred_fast_pack.h"
#include "lpcnet_tables_gen.h"
#include <mutex>

// ---- the engine's part: a host copy of the blob's arrays now, the upload when a batch first enables the decoder
int dred_engine_init(lpcn_engine *e, const lpcn_model_host *m)
{
    e->dred_present = m->dred.present;
    e->dred_servable = lpcn_dred_servable(m) != 0;
    if (!e->dred_servable) return 0;
    auto h = std::make_unique<DredHostModel>();
    h->m = m->dred;
    lpcn_dred_model &d = h->m;
    h->a.take({&d.state[0], &d.state[1], &d.state[2], &d.dense[0], &d.dense[1], &d.dense[2], &d.dense[3], &d.dense[4], &d.final}, d.gru, 3, m->dred.present == 2);
    e->dred_host = std::move(h);
    return 0;
}

// the arrays as they are, the GRUs through upload_gru (engine_core.h) like the PLC network's, in the blob's flavour (W = int: an int8 blob's); then
// the block itself, which the kernel reads from device memory
template <typename W>
static int dred_upload_net(lpcn_engine *e, lpcn::DredNetT<W> &net, const lpcn::DredNetT<W> **d_net)
{
    const lpcn_dred_model &d = e->dred_host->m;
    lpcn::DredNetT<W> n{};
    int rc = 0, off[9] = {0};
    n.latent_dim = d.latent_dim; n.state_dim = d.state_dim;
    for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + d.width[k];
    n.total = off[8];
    auto up_dense = [&](const lpcn_dense_layer &s, lpcn::DredStepT<W> &o, int x, int out) {
        o.gru = 0; o.n_in = s.n_in; o.n_out = s.n_out; o.x = x; o.out = out;
        int r = upload<float>(e, &o.w, s.w, (size_t)s.n_in * s.n_out);
        return r ? r : upload<float>(e, &o.b, s.b, s.n_out);
    };
    static const int dense_at[5] = {0, 2, 4, 6, 7}, gru_at[3] = {1, 3, 5};
    for (int k = 0; k < 3; ++k) if ((rc = up_dense(d.state[k], n.init[k], -1, off[gru_at[k]]))) return rc;
    for (int k = 0; k < 5; ++k) if ((rc = up_dense(d.dense[k], n.step[dense_at[k]], dense_at[k] ? off[dense_at[k] - 1] : -1, off[dense_at[k]]))) return rc;
    for (int g = 0; g < 3; ++g) {
        const lpcn_gru_layer &G = d.gru[g];
        lpcn::DredStepT<W> &o = n.step[gru_at[g]];
        lpcn::GruLayer<W> L{};
        if ((rc = upload_gru(e, L, G))) return rc;
        o.gru = 1; o.n_in = L.n_in; o.n_out = L.n; o.x = off[gru_at[g] - 1]; o.out = off[gru_at[g]];
        o.gw = L.w; o.rec = L.rec; o.b = L.bias; o.start = L.start; o.pos = L.pos;
        n.max_gru = G.n > n.max_gru ? G.n : n.max_gru;
    }
    if ((rc = upload<float>(e, &n.final_w, d.final.w, (size_t)n.total * LPCN_DRED_OUT)) || (rc = upload<float>(e, &n.final_b, d.final.b, LPCN_DRED_OUT)) ||
        (rc = upload<float>(e, &n.tansig, lpcn_tansig, 201))) return rc;
    if ((rc = upload<lpcn::DredNetT<W>>(e, d_net, &n, 1))) return rc;
    net = n;
    if constexpr (std::is_same<W, float>::value) {       // (what the FAST image is packed from outlives the host copy: dred_fast_upload)
        auto f = std::make_unique<DredFastHost>();
        for (int g = 0; g < 3; ++g) {
            const lpcn_gru_layer &G = d.gru[g];
            f->w[g].assign(G.w, G.w + 32 * (size_t)G.nb);
            f->idx[g].assign(G.idx, G.idx + 3 * G.n / 8 + G.nb);
            f->n_in[g] = G.n_in; f->n[g] = G.n;
        }
        e->dred_fast_host = std::move(f);
    }
    e->dred_host.reset();
    return 0;
}
// the uploaded block's figures, whichever flavour it is (a served decoder is in the blob's own)
static int dred_lds_bytes(const lpcn_engine *e, int S) { return (e->is_int8 ? lpcn::dred_lds_floats(e->dredq, S) : lpcn::dred_lds_floats(e->dred, S)) * (int)sizeof(float); }
static int dred_latent_dim(const lpcn_engine *e) { return e->is_int8 ? e->dredq.latent_dim : e->dred.latent_dim; }
static int dred_state_dim(const lpcn_engine *e) { return e->is_int8 ? e->dredq.state_dim : e->dred.state_dim; }

extern "C" int lpcn_engine_dred_present(const lpcn_engine *e) { return e->dred_present; }
extern "C" int lpcn_batch_dev_dred_enabled(const lpcn_batch_dev *b) { return b->dred ? b->dred->max_latents : 0; }

extern "C" int lpcn_batch_dev_dred_enable(lpcn_batch_dev *b, int max_latents)
{
    lpcn_engine *e = b->e;
    if (e->dred_present == 0) { snprintf(g_err, sizeof(g_err), "the model blob has no DRED decoder (state1..3_*, dec_dense1..8_*, dec_final_*)"); return LPCN_E_MODEL; }
    if (e->dred_present != 1 && e->dred_present != 2) { snprintf(g_err, sizeof(g_err), "the blob's DRED decoder arrays are incomplete, mix float and int8, or do not fit together (widths up to %d, dec_final with %d outputs)", LPCN_DRED_MAX_UNITS, LPCN_DRED_OUT); return LPCN_E_MODEL; }
    if (!e->dred_servable && e->dred_present == 2) { snprintf(g_err, sizeof(g_err), "the blob's DRED decoder is int8 (DOT_PROD) but its LPCNet model is float: int8 decoder arrays are served beside an int8 model"); return LPCN_E_MODEL; }
    if (!e->dred_servable) { snprintf(g_err, sizeof(g_err), "the blob's DRED decoder is float but its LPCNet model is int8: float decoder arrays are served beside a float model"); return LPCN_E_MODEL; }
    if (max_latents < 1 || (long long)max_latents * LPCN_DRED_FRAMES * b->n > 0x7fffffffLL / LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "DRED: max_latents must be at least 1 (and the batch's rows fit an int)"); return LPCN_E_ARG; }
    DeviceGuard guard(e->device);
    int rc = wait_all(b);
    if (rc) return rc;
    if (e->dred_host && (rc = e->is_int8 ? dred_upload_net<int>(e, e->dredq, &e->d_dredq) : dred_upload_net<float>(e, e->dred, &e->d_dred))) return rc;
    if ((size_t)dred_lds_bytes(e, 1) > 160 * 1024) { snprintf(g_err, sizeof(g_err), "DRED: the decoder's buffers do not fit the LDS"); return LPCN_E_MODEL; }
    if (!b->dred) {
        auto p = std::make_unique<lpcn_dred_host>();
        if ((rc = p->d_rec.alloc((size_t)lpcn::DRED_REC * b->n)) || (rc = p->h_rec.reserve(sizeof(int) * lpcn::DRED_REC * (size_t)b->n))) return rc;
        if (hipEventCreateWithFlags(&p->ev_rec.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED: hipEventCreate failed"); return LPCN_E_HIP; }
        b->dred = std::move(p);
    }
    b->dred->max_latents = max_latents;
    b->dred->cus = device_cus(e);
    return 0;
}
#define NEED_DRED(b) do { if (!(b)->dred) { snprintf(g_err, sizeof(g_err), "the DRED decoder is not enabled on this batch (lpcnet_batch_dred_enable)"); return LPCN_E_MODEL; } } while (0)

extern "C" int lpcn_batch_dev_dred_dims(const lpcn_batch_dev *b, int *latent_dim, int *state_dim)
{
    NEED_DRED(b);
    if (latent_dim) *latent_dim = dred_latent_dim(b->e);
    if (state_dim) *state_dim = dred_state_dim(b->e);
    return 0;
}
extern "C" int lpcn_batch_dev_dred_flavour(const lpcn_batch_dev *b)
{
    NEED_DRED(b);
    return b->e->is_int8 ? 1 : 0;
}

// ---- streams per workgroup.  A workgroup's time per latent is set by its dependent add chains, not by how many streams it carries: measured on one
// MI355X at width 256 and 25 latents (profiles/dred_rate.json), 256 streams take 6.61 / 6.71 / 6.92 / 7.67 ms at 1 / 2 / 4 / 8 streams per
// workgroup -- one workgroup per CU or fewer, so the fewest streams win -- and 2 048 streams 52.8 / 27.3 / 14.2 / 7.78 ms, 8 192 streams 210.9 / 109.1 /
// 56.4 / 31.0 ms: the time follows the number of workgroups.  The table: the fewest streams per workgroup that still put the streams on the CUs in one
// round, eight beyond that.  An int8 blob's decoder shares the table: measured beside the float one (profiles/dred_i8_rate.json) it
// takes 2.78 / 2.82 / 3.11 / 4.86 ms at 256 streams, 21.1 / 10.9 / 6.25 / 4.91 ms at 2 048 and 83.7 / 43.0 / 24.4 / 19.3 ms at 8 192, and the table's
// form is within the run's spread of the best pinned one in every row.
static bool dred_form_fits(const lpcn_engine *e, int S) { return (size_t)dred_lds_bytes(e, S) <= 160 * 1024; }
extern "C" int lpcn_batch_dev_dred_form(const lpcn_batch_dev *b, int n)
{
    NEED_DRED(b);
    int S = b->dred->form;
    if (!S) {
        const int cus = b->dred->cus;
        for (S = 1; S < 8 && (n + S - 1) / S > cus; S *= 2) {}
    }
    while (S > 1 && !dred_form_fits(b->e, S)) S /= 2;      // (widths the widest form's buffers do not fit)
    return S;
}
extern "C" int lpcn_batch_dev_dred_set_form(lpcn_batch_dev *b, int S)
{
    NEED_DRED(b);
    if (S != 0 && S != 1 && S != 2 && S != 4 && S != 8) { snprintf(g_err, sizeof(g_err), "DRED form: 1, 2, 4 or 8 streams per workgroup, 0 = the table's choice"); return LPCN_E_ARG; }
    b->dred->form = S;
    return 0;
}

// ---- the FAST flavour (dred_fast_kernels.hip.h): the float decoder in the arithmetic of the reference's AVX2+FMA build, the streams of a workgroup on
// the columns of an fp32 MFMA.  Its image of the GRUs' sparse input matrices is packed on the host (dred_fast_pack.h) and uploaded when a batch first
// asks for FAST; the host copy of those matrices goes then.  The other arrays are the PARITY block's.
int dred_fast_image_upload(lpcn_engine *e, const DredFastHost &F, const lpcn::DredFastImage **dst, const char *what)
{
    lpcn::DredFastImage im{};
    for (int g = 0; g < 3; ++g) {
        lpcn_dred_fast_gru pk;
        const int prc = lpcn_dred_fast_pack(F.w[g].data(), F.idx[g].data(), F.n_in[g], F.n[g], &pk);
        if (prc) {
            if (prc == -1) snprintf(g_err, sizeof(g_err), "%s: out of memory", what);
            else snprintf(g_err, sizeof(g_err), "%s: GRU %d's block lists are not ascending: no FAST image", what, g);
            return prc == -1 ? LPCN_E_HIP : LPCN_E_MODEL;
        }
        const size_t blocks = (size_t)pk.start[3 * pk.tiles];
        int rc = upload<int>(e, &im.gru[g].start, pk.start, 3 * (size_t)pk.tiles + 1);
        if (!rc) rc = upload<int>(e, &im.gru[g].pos, pk.pos, blocks);
        if (!rc) rc = upload<float>(e, &im.gru[g].w, pk.w, blocks * 128);
        lpcn_dred_fast_release(&pk);
        if (rc) return rc;
    }
    return upload<lpcn::DredFastImage>(e, dst, &im, 1);
}
static int dred_fast_upload(lpcn_engine *e)
{
    if (e->d_dred_fast) return 0;
    if (!e->dred_fast_host) { snprintf(g_err, sizeof(g_err), "DRED FAST: the decoder's host arrays are gone"); return LPCN_E_MODEL; }
    const int rc = dred_fast_image_upload(e, *e->dred_fast_host, &e->d_dred_fast, "DRED FAST");
    if (rc) return rc;
    e->dred_fast_host.reset();
    return 0;
}
// The tile a FAST launch over n streams runs with: the pinned one, or the engine's choice (mode 1).  The rule is read off
// profiles/dred_fast_rate.json (one MI355X, width 256, 25 latents): a tile's chain takes the same time however many tiles run in
// one round -- T = 16: 4.68 / 4.28 ms for 16 / 128 tiles and 8.62 ms for 512 (two rounds); T = 32: 8.31 / 7.79 / 7.54 ms for 8 / 64 / 256 tiles;
// PARITY's table form 6.66 / 7.87 / 30.90 ms at those 256 / 2 048 / 8 192 streams -- so T = 16 while its tiles fit the CUs in one round, 32 beyond.
// The bits of a stream are the same in both
static int dred_fast_tile(const lpcn_dred_host *p, int n)
{
    if (p->fast != 1) return p->fast;
    return (n + 15) / 16 <= p->cus ? 16 : 32;
}
extern "C" int lpcn_batch_dev_dred_get_fast(const lpcn_batch_dev *b)
{
    NEED_DRED(b);
    return b->dred->fast;
}
extern "C" int lpcn_batch_dev_dred_set_fast(lpcn_batch_dev *b, int mode)
{
    NEED_DRED(b);
    lpcn_engine *e = b->e;
    if (mode != 0 && mode != 1 && mode != 16 && mode != 32) { snprintf(g_err, sizeof(g_err), "DRED FAST: 0 = off, 1 = the engine's tile, 16 or 32 = that many streams per workgroup (the tiles that are built)"); return LPCN_E_ARG; }
    if (e->is_int8 && mode) { snprintf(g_err, sizeof(g_err), "DRED FAST: the int8 decoder has no FAST form yet"); return LPCN_E_MODEL; }
    if (mode) {
        if ((size_t)lpcn::dred_fast_lds_floats(e->dred, mode == 16 ? 16 : 32) * sizeof(float) > 160 * 1024 - 1024) { snprintf(g_err, sizeof(g_err), "DRED FAST: the decoder's tile does not fit the LDS"); return LPCN_E_MODEL; }
        DeviceGuard guard(e->device);
        int rc = wait_all(b);
        if (rc || (rc = dred_fast_upload(e))) return rc;
    }
    b->dred->fast = mode;
    return 0;
}

// count in 0 .. max_latents and zero beyond the active prefix; the packed form's first / take inside the decoded rows
extern "C" int lpcn_batch_dev_dred_check(const lpcn_batch_dev *b, const int *count, const int *first, const int *take, long long *rows)
{
    NEED_DRED(b);
    if (!count || (first != nullptr) != (take != nullptr)) { snprintf(g_err, sizeof(g_err), "bad DRED decode arguments"); return LPCN_E_ARG; }
    long long total = 0;
    for (int s = 0; s < b->n; ++s) {
        if (count[s] < 0 || count[s] > b->dred->max_latents) { snprintf(g_err, sizeof(g_err), "DRED decode: stream %d has a count outside 0 .. %d", s, b->dred->max_latents); return LPCN_E_ARG; }
        if (s >= b->active && count[s] != 0) { snprintf(g_err, sizeof(g_err), "DRED decode: stream %d is not active and has a count", s); return LPCN_E_ARG; }
        if (first && s < b->active) {
            if (first[s] < 0 || take[s] < 0 || (long long)first[s] + take[s] > (long long)LPCN_DRED_FRAMES * count[s]) { snprintf(g_err, sizeof(g_err), "DRED decode: stream %d selects rows outside its %d decoded ones", s, LPCN_DRED_FRAMES * count[s]); return LPCN_E_ARG; }
            total += take[s];
        }
    }
    if (total > 0x7fffffffLL / LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "DRED decode: too many packed rows"); return LPCN_E_ARG; }
    if (rows) *rows = total;
    return 0;
}

template <int S, typename W>
static int dred_launch_form(const lpcn::DredNetT<W> *P, int grid, int lds, hipStream_t st, int n, int max_latents, const int *d_rec, const float *d_state,
                            const float *d_latents, float *d_out)
{
    // the dynamic-LDS limit of a form is raised once per (device, size), not at every launch
    static std::mutex mu;
    static int limit[64];
    const auto kernel = [] { if constexpr (std::is_same<W, float>::value) return lpcn::dred_decode_kernel<S>; else return lpcn::dred_decode_i8_kernel<S>; }();
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> g(mu);
        if (dev < 0 || dev >= 64 || limit[dev] < lds) {
            HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            if (dev >= 0 && dev < 64) limit[dev] = lds;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(lpcn::DRED_THREADS), lds, st, P, n, max_latents, d_rec, d_state, d_latents, d_out);
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED decode: kernel launch failed"); return LPCN_E_HIP; }
    return 0;
}

// the FAST launch: T streams per workgroup, U steps of weights in flight per wave (the smaller tile's accumulators leave registers for twice as many)
template <int T, int U>
static int dred_fast_launch(const lpcn_engine *e, hipStream_t st, int n, int max_latents, const int *d_rec, const float *d_state, const float *d_latents, float *d_out)
{
    static std::mutex mu;
    static int limit[64];
    const auto kernel = lpcn::dred_fast_kernel<T, U>;
    const int lds = lpcn::dred_fast_lds_floats(e->dred, T) * (int)sizeof(float);
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> g(mu);
        if (dev < 0 || dev >= 64 || limit[dev] < lds) {
            HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            if (dev >= 0 && dev < 64) limit[dev] = lds;
        }
    }
    hipLaunchKernelGGL(kernel, dim3((n + T - 1) / T), dim3(lpcn::DRED_FAST_THREADS), lds, st, e->d_dred, e->d_dred_fast, n, max_latents, d_rec, d_state, d_latents, d_out);
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED decode: kernel launch failed"); return LPCN_E_HIP; }
    return 0;
}

template <typename W>
static int dred_launch(const lpcn::DredNetT<W> *P, int S, int grid, int lds, hipStream_t st, int n, int max_latents, const int *d_rec, const float *d_state,
                       const float *d_latents, float *d_out)
{
    switch (S) {
    case 1: return dred_launch_form<1>(P, grid, lds, st, n, max_latents, d_rec, d_state, d_latents, d_out);
    case 2: return dred_launch_form<2>(P, grid, lds, st, n, max_latents, d_rec, d_state, d_latents, d_out);
    case 4: return dred_launch_form<4>(P, grid, lds, st, n, max_latents, d_rec, d_state, d_latents, d_out);
    default: return dred_launch_form<8>(P, grid, lds, st, n, max_latents, d_rec, d_state, d_latents, d_out);
    }
}

// checks, the records' upload through the pinned buffer, one launch.  first == NULL: the plain layout
static int dred_enqueue(lpcn_batch_dev *b, const float *d_state, const float *d_latents, const int *count, const int *first, const int *take, float *d_out,
                        hipStream_t st)
{
    int rc = lpcn_batch_dev_dred_check(b, count, first, take, nullptr);
    if (rc) return rc;
    bool any = false;
    for (int s = 0; s < b->active; ++s) any |= count[s] > 0;
    if (!any) return 0;
    if (!d_state || !d_latents || !d_out) { snprintf(g_err, sizeof(g_err), "bad DRED decode arguments"); return LPCN_E_ARG; }
    if (stream_is_capturing(st)) { snprintf(g_err, sizeof(g_err), "a DRED decode cannot be captured: its launch depends on the host's count array"); return LPCN_E_ARG; }
    lpcn_dred_host *p = b->dred.get();
    if (p->rec_pending) { HIP_TRY(hipEventSynchronize(p->ev_rec)); p->rec_pending = false; }      // (the previous call's records have left the pinned buffer)
    int *h = (int *)p->h_rec.p, row = 0;
    for (int s = 0; s < b->active; ++s) {
        int *q = h + (size_t)s * lpcn::DRED_REC;
        q[0] = count[s]; q[1] = first ? first[s] : -1; q[2] = first ? take[s] : 0; q[3] = row;
        if (first) row += take[s];
    }
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(p->d_rec, h, sizeof(int) * lpcn::DRED_REC * (size_t)b->active, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->ev_rec, st));
    p->rec_pending = true;
    if (p->fast) {
        rc = dred_fast_tile(p, b->active) == 16 ? dred_fast_launch<16, 16>(b->e, st, b->active, p->max_latents, p->d_rec, d_state, d_latents, d_out)
                                                : dred_fast_launch<32, 8>(b->e, st, b->active, p->max_latents, p->d_rec, d_state, d_latents, d_out);
    } else {
        const int S = lpcn_batch_dev_dred_form(b, b->active);
        const int grid = (b->active + S - 1) / S, lds = dred_lds_bytes(b->e, S);
        rc = b->e->is_int8 ? dred_launch(b->e->d_dredq, S, grid, lds, st, b->active, p->max_latents, p->d_rec, d_state, d_latents, d_out)
                           : dred_launch(b->e->d_dred, S, grid, lds, st, b->active, p->max_latents, p->d_rec, d_state, d_latents, d_out);
    }
    if (rc) return rc;
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_dred_decode(lpcn_batch_dev *b, const float *d_state, const float *d_latents, const int *count, float *d_features, void *hip_stream)
{
    NEED_DRED(b);
    DeviceGuard guard(b->e->device);
    return dred_enqueue(b, d_state, d_latents, count, nullptr, nullptr, d_features, hip_stream ? (hipStream_t)hip_stream : b->e->stream);
}

extern "C" int lpcn_batch_dev_dred_decode_packed(lpcn_batch_dev *b, const float *d_state, const float *d_latents, const int *count, const int *first,
                                                 const int *take, float *d_packed, void *hip_stream)
{
    NEED_DRED(b);
    if (!first || !take) { snprintf(g_err, sizeof(g_err), "bad DRED decode arguments"); return LPCN_E_ARG; }
    long long rows = 0;
    int rc = lpcn_batch_dev_dred_check(b, count, first, take, &rows);
    if (rc) return rc;
    if (!rows) return 0;
    DeviceGuard guard(b->e->device);
    return dred_enqueue(b, d_state, d_latents, count, first, take, d_packed, hip_stream ? (hipStream_t)hip_stream : b->e->stream);
}

// host pointers: the active streams' rows in, one launch, the output down whole and out to the caller row by row
extern "C" int lpcn_batch_dev_dred_decode_host(lpcn_batch_dev *b, const float *state, const float *latents, const int *count, float *features)
{
    NEED_DRED(b);
    int rc = lpcn_batch_dev_dred_check(b, count, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (!state || !latents || !features) { snprintf(g_err, sizeof(g_err), "bad DRED decode arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    lpcn_dred_host *p = b->dred.get();
    hipStream_t st = b->e->stream;
    const size_t n = (size_t)b->active, per_s = (size_t)dred_state_dim(b->e), per_l = (size_t)p->max_latents * dred_latent_dim(b->e),
                 per_f = (size_t)LPCN_DRED_FRAMES * p->max_latents * LPCN_NB_FEAT;
    if ((rc = p->d_state.reserve(b, (size_t)b->n * per_s)) || (rc = p->d_latents.reserve(b, (size_t)b->n * per_l)) || (rc = p->d_feat.reserve(b, (size_t)b->n * per_f)) ||
        (rc = p->h_feat.reserve(sizeof(float) * (size_t)b->n * per_f))) return rc;
    HIP_TRY(hipMemcpyAsync(p->d_state, state, sizeof(float) * n * per_s, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p->d_latents, latents, sizeof(float) * n * per_l, hipMemcpyHostToDevice, st));
    if ((rc = dred_enqueue(b, p->d_state, p->d_latents, count, nullptr, nullptr, p->d_feat, st))) return rc;
    HIP_TRY(hipMemcpyAsync(p->h_feat.p, p->d_feat, sizeof(float) * n * per_f, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t s = 0; s < n; ++s)
        memcpy(features + s * per_f, (const float *)p->h_feat.p + s * per_f, sizeof(float) * LPCN_DRED_FRAMES * LPCN_NB_FEAT * (size_t)count[s]);
    return 0;
}

// ---- the decoder as a per-stream state (DRED_rdovae_dec_init_states / DRED_rdovae_decode_qframe; dred_stream_kernel, dred_stream_fast_kernel;
// DESIGN.md §4.6b).  The record is float in every flavour and mode; all zero is DRED_rdovae_init_decoder.
static int dred_state_floats(const lpcn_engine *e) { return e->is_int8 ? lpcn::dred_state_floats(e->dredq) : lpcn::dred_state_floats(e->dred); }
template <int S>
static const void *dred_stream_kernel_of(const lpcn_engine *e)
{
    return e->is_int8 ? (const void *)lpcn::dred_stream_kernel<S, true> : (const void *)lpcn::dred_stream_kernel<S, false>;
}
// the dynamic-LDS limits are raised here, not at a launch: a launch sets nothing, so the uniform forms can be captured
template <int S>
static int dred_stream_prepare(const lpcn_engine *e)
{
    if (!dred_form_fits(e, S)) return 0;
    HIP_TRY(hipFuncSetAttribute(dred_stream_kernel_of<S>(e), hipFuncAttributeMaxDynamicSharedMemorySize, dred_lds_bytes(e, S)));
    return 0;
}
template <int T, int U>
static int dred_stream_fast_prepare(const lpcn_engine *e)
{
    const size_t lds = (size_t)lpcn::dred_fast_lds_floats(e->dred, T) * sizeof(float);
    if (lds > 160 * 1024 - 1024) return 0;      // (dred_set_fast refuses that tile)
    HIP_TRY(hipFuncSetAttribute((const void *)lpcn::dred_stream_fast_kernel<T, U>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
}

extern "C" int lpcn_batch_dev_dred_state_enabled(const lpcn_batch_dev *b) { return b->dred && b->dred->st ? dred_state_floats(b->e) : 0; }

extern "C" int lpcn_batch_dev_dred_state_enable(lpcn_batch_dev *b)
{
    NEED_DRED(b);
    lpcn_engine *e = b->e;
    lpcn_dred_host *p = b->dred.get();
    if (p->st) return 0;
    DeviceGuard guard(e->device);
    int rc = wait_all(b);
    if (rc || (rc = dred_stream_prepare<1>(e)) || (rc = dred_stream_prepare<2>(e)) || (rc = dred_stream_prepare<4>(e)) || (rc = dred_stream_prepare<8>(e))) return rc;
    if (!e->is_int8 && ((rc = dred_stream_fast_prepare<16, 16>(e)) || (rc = dred_stream_fast_prepare<32, 8>(e)))) return rc;
    const size_t per = (size_t)(e->is_int8 ? lpcn::dred_state_rec_floats(e->dredq) : lpcn::dred_state_rec_floats(e->dred));
    DevBuf<float> st;
    if ((rc = st.alloc(per * b->n)) || (rc = p->d_srec.alloc((size_t)lpcn::DRED_SREC * b->n)) || (rc = p->h_srec.reserve(sizeof(int) * lpcn::DRED_SREC * (size_t)b->n))) return rc;
    if (!p->ev_srec.e && hipEventCreateWithFlags(&p->ev_srec.e, hipEventDisableTiming) != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED: hipEventCreate failed"); return LPCN_E_HIP; }
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(float) * per * b->n, e->stream));      // (DRED_rdovae_init_decoder; done before the call returns: the first
    HIP_TRY(hipStreamSynchronize(e->stream));                                   //  init may go to any stream)
    p->st.p = st.p; p->st.cap = st.cap; st.p = nullptr; st.cap = 0;
    p->st_rec = per;
    return 0;
}
#define NEED_DRED_STATE(b) do { NEED_DRED(b); if (!(b)->dred->st) { snprintf(g_err, sizeof(g_err), "the DRED decoder's per-stream state is not enabled on this batch (lpcnet_batch_dred_state_enable)"); return LPCN_E_MODEL; } } while (0)

// lpcn_batch_dev_reset's part: the records of [first, first + count) as DRED_rdovae_init_decoder leaves them
int dred_state_reset(lpcn_batch_dev *b, int first, int count)
{
    lpcn_dred_host *p = b->dred.get();
    if (!count || !p || !p->st) return 0;
    HIP_TRY(hipMemsetAsync(p->st + (size_t)first * p->st_rec, 0, sizeof(float) * (size_t)count * p->st_rec, b->e->stream));
    HIP_TRY(hipStreamSynchronize(b->e->stream));
    return 0;
}

// one stream's three states in the reference's member order: the record without its padding
extern "C" int lpcn_batch_dev_dred_get_dec_state(lpcn_batch_dev *b, int s, float *out)
{
    NEED_DRED_STATE(b);
    lpcn_dred_host *p = b->dred.get();
    if (!out) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    std::vector<float> r(p->st_rec);
    const int rc = stream_rec(b, s, p->st, p->st_rec, r.data(), nullptr);
    if (!rc) memcpy(out, r.data(), sizeof(float) * (size_t)dred_state_floats(b->e));
    return rc;
}
extern "C" int lpcn_batch_dev_dred_set_dec_state(lpcn_batch_dev *b, int s, const float *in)
{
    NEED_DRED_STATE(b);
    lpcn_dred_host *p = b->dred.get();
    if (!in) { snprintf(g_err, sizeof(g_err), "stream index"); return LPCN_E_ARG; }
    std::vector<float> r(p->st_rec, 0.f);
    memcpy(r.data(), in, sizeof(float) * (size_t)dred_state_floats(b->e));
    return stream_rec(b, s, p->st, p->st_rec, nullptr, r.data());
}

// which == NULL: every active stream; else no flag beyond the active prefix
extern "C" int lpcn_batch_dev_dred_init_check(const lpcn_batch_dev *b, const int *which)
{
    NEED_DRED_STATE(b);
    for (int s = b->active; which && s < b->n; ++s)
        if (which[s]) { snprintf(g_err, sizeof(g_err), "DRED init: stream %d is not active and is selected", s); return LPCN_E_ARG; }
    return 0;
}
// start == count == NULL: the uniform form, latents u_start .. u_start + u_count - 1 of every active stream.  Else per stream, zero counts beyond the
// active prefix; the packed form's first / take in the stream's own row numbers, inside the rows this call decodes
extern "C" int lpcn_batch_dev_dred_step_check(const lpcn_batch_dev *b, const int *start, const int *count, int u_start, int u_count, const int *first,
                                              const int *take, long long *rows)
{
    NEED_DRED_STATE(b);
    const int ml = b->dred->max_latents;
    if ((start != nullptr) != (count != nullptr) || (first != nullptr) != (take != nullptr) || (first && !count)) { snprintf(g_err, sizeof(g_err), "bad DRED step arguments"); return LPCN_E_ARG; }
    if (!count) {
        if (u_start < 0 || u_count < 0 || (long long)u_start + u_count > ml) { snprintf(g_err, sizeof(g_err), "DRED step: latents %d .. %d + %d outside 0 .. %d", u_start, u_start, u_count, ml); return LPCN_E_ARG; }
        if (rows) *rows = 0;
        return 0;
    }
    long long total = 0;
    for (int s = 0; s < b->n; ++s) {
        if (start[s] < 0 || count[s] < 0 || (long long)start[s] + count[s] > ml) { snprintf(g_err, sizeof(g_err), "DRED step: stream %d has latents outside 0 .. %d (start %d, count %d)", s, ml, start[s], count[s]); return LPCN_E_ARG; }
        if (s >= b->active && count[s] != 0) { snprintf(g_err, sizeof(g_err), "DRED step: stream %d is not active and has a count", s); return LPCN_E_ARG; }
        if (first && s < b->active) {
            const long long lo = (long long)LPCN_DRED_FRAMES * start[s], hi = lo + (long long)LPCN_DRED_FRAMES * count[s];
            if (take[s] < 0 || (take[s] > 0 && (first[s] < lo || (long long)first[s] + take[s] > hi)) || (take[s] == 0 && first[s] < 0)) {
                snprintf(g_err, sizeof(g_err), "DRED step: stream %d selects rows outside the %lld .. %lld this call decodes", s, lo, hi - 1);
                return LPCN_E_ARG;
            }
            total += take[s];
        }
    }
    if (total > 0x7fffffffLL / LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "DRED step: too many packed rows"); return LPCN_E_ARG; }
    if (rows) *rows = total;
    return 0;
}

// one launch of the stream kernel in the batch's arithmetic, form and tile.  d_rec == nullptr: the uniform form
static int dred_stream_launch(lpcn_batch_dev *b, hipStream_t st, int init, const int *d_rec, int u_start, int u_count, const float *d_state, const float *d_latents,
                              float *d_out)
{
    lpcn_engine *e = b->e;
    lpcn_dred_host *p = b->dred.get();
    const int n = b->active, ml = p->max_latents, rf = (int)p->st_rec;
    float *ds = p->st;
    if (p->fast) {
        if (dred_fast_tile(p, n) == 16)
            hipLaunchKernelGGL((lpcn::dred_stream_fast_kernel<16, 16>), dim3((n + 15) / 16), dim3(lpcn::DRED_FAST_THREADS), lpcn::dred_fast_lds_floats(e->dred, 16) * (int)sizeof(float), st,
                               e->d_dred, e->d_dred_fast, n, ml, init, d_rec, u_start, u_count, d_state, d_latents, d_out, ds, rf);
        else
            hipLaunchKernelGGL((lpcn::dred_stream_fast_kernel<32, 8>), dim3((n + 31) / 32), dim3(lpcn::DRED_FAST_THREADS), lpcn::dred_fast_lds_floats(e->dred, 32) * (int)sizeof(float), st,
                               e->d_dred, e->d_dred_fast, n, ml, init, d_rec, u_start, u_count, d_state, d_latents, d_out, ds, rf);
    } else {
        const int S = lpcn_batch_dev_dred_form(b, n);
        const int grid = (n + S - 1) / S, lds = dred_lds_bytes(e, S);
        auto go = [&](auto form) {
            constexpr int F = decltype(form)::value;
            if (e->is_int8) hipLaunchKernelGGL((lpcn::dred_stream_kernel<F, true>), dim3(grid), dim3(lpcn::DRED_THREADS), lds, st, e->d_dredq, n, ml, init, d_rec, u_start, u_count, d_state, d_latents, d_out, ds, rf);
            else hipLaunchKernelGGL((lpcn::dred_stream_kernel<F, false>), dim3(grid), dim3(lpcn::DRED_THREADS), lds, st, e->d_dred, n, ml, init, d_rec, u_start, u_count, d_state, d_latents, d_out, ds, rf);
        };
        switch (S) {
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        case 4: go(std::integral_constant<int, 4>{}); break;
        default: go(std::integral_constant<int, 8>{}); break;
        }
    }
    if (hipGetLastError() != hipSuccess) { snprintf(g_err, sizeof(g_err), "DRED %s: kernel launch failed", init ? "init" : "step"); return LPCN_E_HIP; }
    return 0;
}

// checks, the records' upload through the pinned buffer (none for the uniform forms), one launch.  init: `flag` is `which`.  first == NULL: the plain layout
static int dred_stream_enqueue(lpcn_batch_dev *b, int init, const float *d_state, const float *d_latents, const int *flag, const int *start, const int *count, int u_start,
                               int u_count, const int *first, const int *take, float *d_out, hipStream_t st)
{
    long long rows = 0;
    int rc = init ? lpcn_batch_dev_dred_init_check(b, flag) : lpcn_batch_dev_dred_step_check(b, start, count, u_start, u_count, first, take, &rows);
    if (rc) return rc;
    const int *per = init ? flag : count;
    bool any = !per && b->active > 0 && (init || u_count > 0);
    for (int s = 0; per && s < b->active; ++s) any |= per[s] != 0;
    if (!any) return 0;
    // (a packed step that takes no row still advances its streams)
    if (init ? !d_state : (!d_latents || (!d_out && (!first || rows)))) { snprintf(g_err, sizeof(g_err), "bad DRED %s arguments", init ? "init" : "step"); return LPCN_E_ARG; }
    lpcn_dred_host *p = b->dred.get();
    if (per && stream_is_capturing(st)) { snprintf(g_err, sizeof(g_err), "a DRED %s with host arrays cannot be captured: its launch depends on them (the uniform form can)", init ? "init" : "step"); return LPCN_E_ARG; }
    if ((rc = order_begin(b, st))) return rc;
    if (per) {
        if (p->srec_pending) { HIP_TRY(hipEventSynchronize(p->ev_srec)); p->srec_pending = false; }      // (the previous call's records have left the pinned buffer)
        int *h = (int *)p->h_srec.p, row = 0;
        for (int s = 0; s < b->active; ++s) {
            int *q = h + (size_t)s * lpcn::DRED_SREC;
            q[0] = init ? flag[s] != 0 : 0; q[1] = init ? 0 : start[s]; q[2] = init ? 0 : count[s];
            q[3] = first ? first[s] : -1; q[4] = first ? take[s] : 0; q[5] = row; q[6] = q[7] = 0;
            if (first) row += take[s];
        }
        HIP_TRY(hipMemcpyAsync(p->d_srec, h, sizeof(int) * lpcn::DRED_SREC * (size_t)b->active, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(p->ev_srec, st));
        p->srec_pending = true;
    }
    if ((rc = dred_stream_launch(b, st, init, per ? (const int *)p->d_srec : nullptr, u_start, u_count, d_state, d_latents, d_out))) return rc;
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_dred_init(lpcn_batch_dev *b, const float *d_state, const int *which, void *hip_stream)
{
    NEED_DRED_STATE(b);
    DeviceGuard guard(b->e->device);
    return dred_stream_enqueue(b, 1, d_state, nullptr, which, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, hip_stream ? (hipStream_t)hip_stream : b->e->stream);
}
extern "C" int lpcn_batch_dev_dred_step(lpcn_batch_dev *b, const float *d_latents, const int *start, const int *count, int first_latent, int n_latents, float *d_features,
                                        void *hip_stream)
{
    NEED_DRED_STATE(b);
    DeviceGuard guard(b->e->device);
    return dred_stream_enqueue(b, 0, nullptr, d_latents, nullptr, start, count, first_latent, n_latents, nullptr, nullptr, d_features, hip_stream ? (hipStream_t)hip_stream : b->e->stream);
}
extern "C" int lpcn_batch_dev_dred_step_packed(lpcn_batch_dev *b, const float *d_latents, const int *start, const int *count, const int *first, const int *take,
                                               float *d_packed, void *hip_stream)
{
    NEED_DRED_STATE(b);
    if (!start || !count || !first || !take) { snprintf(g_err, sizeof(g_err), "bad DRED step arguments"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    return dred_stream_enqueue(b, 0, nullptr, d_latents, nullptr, start, count, 0, 0, first, take, d_packed, hip_stream ? (hipStream_t)hip_stream : b->e->stream);
}

// host pointers: the active streams' rows in, one launch, and for a step the output down whole and out to the caller, the rows of this call alone
extern "C" int lpcn_batch_dev_dred_init_host(lpcn_batch_dev *b, const float *state, const int *which)
{
    NEED_DRED_STATE(b);
    int rc = lpcn_batch_dev_dred_init_check(b, which);
    if (rc) return rc;
    if (!state) { snprintf(g_err, sizeof(g_err), "bad DRED init arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    lpcn_dred_host *p = b->dred.get();
    hipStream_t st = b->e->stream;
    const size_t per_s = (size_t)dred_state_dim(b->e);
    if ((rc = p->d_state.reserve(b, (size_t)b->n * per_s))) return rc;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffer may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(p->d_state, state, sizeof(float) * (size_t)b->active * per_s, hipMemcpyHostToDevice, st));
    if ((rc = dred_stream_enqueue(b, 1, p->d_state, nullptr, which, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
extern "C" int lpcn_batch_dev_dred_step_host(lpcn_batch_dev *b, const float *latents, const int *start, const int *count, float *features)
{
    NEED_DRED_STATE(b);
    if (!start || !count) { snprintf(g_err, sizeof(g_err), "bad DRED step arguments"); return LPCN_E_ARG; }
    int rc = lpcn_batch_dev_dred_step_check(b, start, count, 0, 0, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (!latents || !features) { snprintf(g_err, sizeof(g_err), "bad DRED step arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    lpcn_dred_host *p = b->dred.get();
    hipStream_t st = b->e->stream;
    const size_t n = (size_t)b->active, per_l = (size_t)p->max_latents * dred_latent_dim(b->e), per_f = (size_t)LPCN_DRED_FRAMES * p->max_latents * LPCN_NB_FEAT;
    if ((rc = p->d_latents.reserve(b, (size_t)b->n * per_l)) || (rc = p->d_feat.reserve(b, (size_t)b->n * per_f)) || (rc = p->h_feat.reserve(sizeof(float) * (size_t)b->n * per_f))) return rc;
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(p->d_latents, latents, sizeof(float) * n * per_l, hipMemcpyHostToDevice, st));
    if ((rc = dred_stream_enqueue(b, 0, nullptr, p->d_latents, nullptr, start, count, 0, 0, nullptr, nullptr, p->d_feat, st))) return rc;
    HIP_TRY(hipMemcpyAsync(p->h_feat.p, p->d_feat, sizeof(float) * n * per_f, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t row = (size_t)LPCN_DRED_FRAMES * LPCN_NB_FEAT;
    for (size_t s = 0; s < n; ++s)
        memcpy(features + s * per_f + row * start[s], (const float *)p->h_feat.p + s * per_f + row * start[s], sizeof(float) * row * (size_t)count[s]);
    return 0;
}
