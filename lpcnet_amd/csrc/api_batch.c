/* C host shell of the LPCNet HIP engine, batch half: every entry point of include/lpcnet_batch.h that takes an LPCNetBatch, on top of the
 * device runtime declared in lpcnet_engine.h.  Which streams a shard owns and how one call fans out over the shards is api_shards.h. */
#include "api_internal.h"
#include "api_roster.h"
#include "snapshot_plan.h"

LPCNetBatch *lpcnet_batch_create_sharded(int n_streams, const int *devices, int n_devices)
{
    if (n_streams <= 0 || !devices || n_devices <= 0 || n_devices > LPCN_MAX_SHARDS) { set_err("lpcnet_batch_create_sharded: bad arguments"); return NULL; }
    for (int k = 0; k < n_devices; k++) if (devices[k] < 0) { set_err("lpcnet_batch_create_sharded: bad device"); return NULL; }
    LPCNetBatch *b = (LPCNetBatch *)calloc(1, sizeof(*b));
    if (!b) return NULL;
    b->n = n_streams;
    b->n_shards = shard_partition(n_streams, n_devices, b->at);      /* (more devices than streams: the last ones stay without a shard) */
    for (int k = 0; k < b->n_shards; k++) b->sh[k].device = devices[k];
    return b;
}

LPCNetBatch *lpcnet_batch_create(int n_streams, int device)
{
    if (n_streams <= 0 || device < 0) { set_err("lpcnet_batch_create: bad arguments"); return NULL; }
    return lpcnet_batch_create_sharded(n_streams, &device, 1);
}

void lpcnet_batch_destroy(LPCNetBatch *b)
{
    if (!b) return;
    for (int k = 0; k < b->n_shards; k++) {
        if (b->sh[k].dev) lpcn_batch_dev_destroy(b->sh[k].dev);
        if (b->sh[k].engine) lpcn_engine_destroy(b->sh[k].engine);
    }
    free(b);
}

int lpcnet_batch_streams(const LPCNetBatch *b) { return b->n; }
int lpcnet_batch_shards(const LPCNetBatch *b) { return b ? b->n_shards : 0; }

int lpcnet_batch_shard_info(const LPCNetBatch *b, int shard, int *first, int *count, int *device)
{
    if (!b || shard < 0 || shard >= b->n_shards) { set_err("shard index"); return LPCN_E_ARG; }
    if (first) *first = b->at[shard].first;
    if (count) *count = b->at[shard].count;
    if (device) *device = b->sh[shard].device;
    return 0;
}

#define BATCH_CHUNK_FRAMES 100       /* frame products are staged per chunk: 100 frames = 1 s of audio */

int lpcnet_batch_load_model(LPCNetBatch *b, const unsigned char *data, int len)
{
    lpcn_model_host m;
    if (!b) { set_err("lpcnet_batch_load_model: bad arguments"); return -1; }
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return -1; }
    lpcn_engine *e[LPCN_MAX_SHARDS] = {0};
    lpcn_batch_dev *d[LPCN_MAX_SHARDS] = {0};
    int rc = 0;
    for (int k = 0; k < b->n_shards && !rc; k++) {          /* the model is replicated on every shard's device */
        rc = lpcn_engine_create(&e[k], b->sh[k].device, &m);
        if (!rc) rc = lpcn_batch_dev_create(&d[k], e[k], b->at[k].count, BATCH_CHUNK_FRAMES);
    }
    lpcn_model_release(&m);
    if (rc) {
        take_engine_err();
        for (int k = 0; k < b->n_shards; k++) { if (d[k]) lpcn_batch_dev_destroy(d[k]); if (e[k]) lpcn_engine_destroy(e[k]); }
        return -1;
    }
    for (int k = 0; k < b->n_shards; k++) {
        if (b->sh[k].dev) lpcn_batch_dev_destroy(b->sh[k].dev);
        if (b->sh[k].engine) lpcn_engine_destroy(b->sh[k].engine);
        b->sh[k].engine = e[k]; b->sh[k].dev = d[k]; b->sh[k].cb_version = 0;
    }
    b->model_hash = 14695981039346656037ull;             /* (taken once, here: a snapshot's layout carries it) */
    for (int i = 0; i < len; i++) b->model_hash = (b->model_hash ^ data[i]) * 1099511628211ull;
    return 0;
}

#define NEED_MODEL(b) do { if (!(b) || !(b)->n_shards || !(b)->sh[0].dev) { set_err("batch has no model (lpcnet_batch_load_model)"); return LPCN_E_MODEL; } } while (0)
#define NEED_ONE_SHARD(b, what) do { if ((b)->n_shards != 1) { set_err(what ": device pointers belong to one device; use the _shard form on a sharded batch"); return LPCN_E_ARG; } } while (0)

/* ---- one call over the shards (api_shards.h).  Shard after shard on the calling thread, stopping at the first that fails: `call` on every shard
 * `s` that holds some of the streams [first, first + count) -- [lfirst, lfirst + lcount) of its own; the shard's streams are `at` -- ... */
#define EACH_SHARD_IN(first, count, call) do { for (int k_ = -1, lfirst, lcount; shard_next_in(b->at, b->n_shards, first, count, &k_, &lfirst, &lcount); ) { \
    batch_shard *s = &b->sh[k_]; const shard_span at = b->at[k_]; (void)at; int rc_ = (call); if (rc_) { take_engine_err(); return rc_; } } return 0; } while (0)
#define EACH_SHARD(call) EACH_SHARD_IN(0, b->n, call)
/* ... or all shards at once, one host thread per shard, each on its own device and stream; with a single shard the work runs on the
 * calling thread.  These calls hand each shard its streams' part of the caller's arrays: an argument struct and a per-shard function stand next to
 * each such entry point. */
static int run_shards(LPCNetBatch *b, shard_fn fn, void *args)
{
    char err[SHARD_ERR_LEN];
    const int rc = shards_run(b->n_shards, 1, fn, lpcn_last_error, args, err);      /* (the engine's message is thread-local) */
    if (rc) set_err(err);
    return rc;
}

int lpcnet_batch_reset(LPCNetBatch *b, int first, int count)
{
    NEED_MODEL(b);
    if (first < 0 || count < 0 || first + count > b->n) { set_err("reset range"); return LPCN_E_ARG; }
    EACH_SHARD_IN(first, count, lpcn_batch_dev_reset(s->dev, lfirst, lcount));
}

typedef struct { LPCNetBatch *b; const float *features; int feat_stride; short *pcm; int n_frames, preload; } synth_args;
static int synth_shard(void *args, int k)
{
    const synth_args *a = (const synth_args *)args;
    const size_t o = (size_t)a->b->at[k].first * a->n_frames;
    return lpcn_batch_dev_run_host(a->b->sh[k].dev, a->features + o * a->feat_stride, a->feat_stride, a->pcm + o * LPCN_FRAME_SIZE, a->n_frames, a->preload);
}
int lpcnet_batch_synthesize_preload(LPCNetBatch *b, const float *features, int feat_stride, short *pcm, int n_frames, int preload)
{
    NEED_MODEL(b);
    synth_args a = {b, features, feat_stride, pcm, n_frames, preload};
    return run_shards(b, synth_shard, &a);
}

/* one frame step with per-stream arguments (see include/lpcnet_batch.h); shards run one after the other */
int lpcnet_batch_synthesize_step(LPCNetBatch *b, const float *features, int feat_stride, short *pcm,
                                 const int *n_samples, const int *preload, const int *mode)
{
    NEED_MODEL(b);
    if (!features || !pcm || !n_samples || !preload || !mode) { set_err("lpcnet_batch_synthesize_step: bad arguments"); return LPCN_E_ARG; }
    EACH_SHARD(lpcn_batch_dev_step_host(s->dev, features + (size_t)at.first * feat_stride, feat_stride, pcm + (size_t)at.first * LPCN_FRAME_SIZE,
                                        n_samples + at.first, preload + at.first, mode + at.first));
}

int lpcnet_batch_synthesize(LPCNetBatch *b, const float *features, int feat_stride, short *pcm, int n_frames)
{
    return lpcnet_batch_synthesize_preload(b, features, feat_stride, pcm, n_frames, 0);
}

int lpcnet_batch_synthesize_device_shard(LPCNetBatch *b, int shard, const float *d_features, int feat_stride, short *d_pcm,
                                         int n_frames, void *hip_stream)
{
    NEED_MODEL(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("shard index"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_run(b->sh[shard].dev, d_features, feat_stride, d_pcm, n_frames, 0, hip_stream));
}

int lpcnet_batch_synthesize_device(LPCNetBatch *b, const float *d_features, int feat_stride, short *d_pcm, int n_frames, void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_synthesize_device");
    return lpcnet_batch_synthesize_device_shard(b, 0, d_features, feat_stride, d_pcm, n_frames, hip_stream);
}

int lpcnet_batch_sync(LPCNetBatch *b) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_sync(s->dev)); }

/* the device copies of the VQ codebooks follow lpcnet_hip_set_codebooks() */
static int batch_codebooks(LPCNetBatch *b)
{
    int version, rc = 0;
    const float *const *cb = codebooks_rdlock(&version);
    if (!cb[0]) { set_err("lpcnet_batch_decode: no VQ codebooks installed (lpcnet_hip_set_codebooks)"); rc = LPCN_E_MODEL; }
    for (int k = 0; !rc && k < b->n_shards; k++)
        if (b->sh[k].cb_version != version) {
            rc = lpcn_engine_set_codebooks(b->sh[k].engine, cb[0], cb[1], cb[2], cb[3]);
            if (rc) take_engine_err(); else b->sh[k].cb_version = version;
        }
    codebooks_unlock();
    return rc;
}

typedef struct { LPCNetBatch *b; const unsigned char *packets; short *pcm; int n_packets; } decode_args;
static int decode_shard(void *args, int k)
{
    const decode_args *a = (const decode_args *)args;
    const size_t o = (size_t)a->b->at[k].first * a->n_packets;
    return lpcn_batch_dev_decode_host(a->b->sh[k].dev, a->packets + o * 8, a->pcm + o * 4 * LPCN_FRAME_SIZE, a->n_packets);
}
/* packets [n][n_packets][8] (host) -> pcm [n][n_packets*640]; unpacking, VQ lookup and interpolation run on the device */
int lpcnet_batch_decode(LPCNetBatch *b, const unsigned char *packets, short *pcm, int n_packets)
{
    NEED_MODEL(b);
    if (n_packets <= 0) { set_err("lpcnet_batch_decode: bad arguments"); return LPCN_E_ARG; }
    int rc = batch_codebooks(b);
    if (rc) return rc;
    decode_args a = {b, packets, pcm, n_packets};
    return run_shards(b, decode_shard, &a);
}

/* the same with device pointers, enqueued on the caller's stream (NULL = the batch's own) */
int lpcnet_batch_decode_device(LPCNetBatch *b, const unsigned char *d_packets, short *d_pcm, int n_packets, void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_decode_device");
    if (n_packets <= 0) { set_err("lpcnet_batch_decode_device: bad arguments"); return LPCN_E_ARG; }
    int rc = batch_codebooks(b);
    if (rc) return rc;
    FWD(lpcn_batch_dev_decode(b->sh[0].dev, d_packets, d_pcm, n_packets, hip_stream));
}

/* LPC_GAMMA of the model (a #define of the reference's generated nnet_data.h, not in the blob); default 1 */
int lpcnet_batch_set_lpc_gamma(LPCNetBatch *b, float gamma) { NEED_MODEL(b); EACH_SHARD(lpcn_engine_set_lpc_gamma(s->engine, gamma)); }
/* END2END models (LPC from the network's reflection coefficients); a #define of the reference, not in the blob */
int lpcnet_batch_set_end2end(LPCNetBatch *b, int on) { NEED_MODEL(b); EACH_SHARD(lpcn_engine_set_end2end(s->engine, on)); }

/* arithmetic flavour: 0 = PARITY (default, bit-identical to the reference's generic-C build), 1 = FAST (what the
 * reference's own SIMD builds do: fused multiply-add / int32 block accumulation; validated teacher-forced) */
static int set_fast_shard(batch_shard *s, int on) { const int rc = lpcn_engine_set_fast(s->engine, on); return rc ? rc : lpcn_batch_dev_retune(s->dev); }
int lpcnet_batch_set_fast(LPCNetBatch *b, int on) { NEED_MODEL(b); EACH_SHARD(set_fast_shard(s, on)); }

/* the shard `sv` that owns a stream, and the stream's index `iv` within it */
#define SHARD_OF(sv, iv, b, stream) int iv; const int k_##sv = shard_of((b)->at, (b)->n_shards, stream, &iv); \
    if (k_##sv < 0) { set_err("stream index"); return LPCN_E_ARG; } batch_shard *sv = &(b)->sh[k_##sv]

int lpcnet_batch_export_state(LPCNetBatch *b, int stream, LPCNetState *st)
{
    NEED_MODEL(b);
    SHARD_OF(s, i, b, stream);
    if (st->magic != LPCN_MAGIC) { st->magic = LPCN_MAGIC; st->model_id = -1; }
    FWD(lpcn_batch_dev_get_state(s->dev, i, &st->s));
}

int lpcnet_batch_import_state(LPCNetBatch *b, int stream, const LPCNetState *st)
{
    NEED_MODEL(b);
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_set_state(s->dev, i, &st->s));
}

/* ---- packet-loss concealment (lpcnet_plc_update / lpcnet_plc_conceal per stream, causal mode; include/lpcnet_batch.h) ---- */
#define NEED_PLC_ON(b) do { NEED_MODEL(b); if (!lpcn_batch_dev_plc_enabled((b)->sh[0].dev)) { set_err("packet-loss concealment is not enabled on this batch (lpcnet_batch_plc_enable)"); return LPCN_E_MODEL; } } while (0)
int lpcnet_batch_plc_enable(LPCNetBatch *b, int options)
{
    NEED_MODEL(b);
    if ((options & 3) == LPCNET_PLC_NONCAUSAL) { set_err("lpcnet_batch_plc_enable: LPCNET_PLC_NONCAUSAL needs a model without feature delay (src/lpcnet_plc.c:357-361); this engine's model format has FEATURES_DELAY = 2"); return LPCN_E_ARG; }
    if ((options & 3) == 3 || (options & ~7)) { set_err("lpcnet_batch_plc_enable: options are LPCNET_PLC_CAUSAL or LPCNET_PLC_CODEC, optionally | LPCNET_PLC_DC_FILTER"); return LPCN_E_ARG; }
    EACH_SHARD(lpcn_batch_dev_plc_enable(s->dev, options));
}
int lpcnet_batch_plc_flavour(const LPCNetBatch *b)
{
    NEED_PLC_ON(b);
    FWD(lpcn_batch_dev_plc_flavour(b->sh[0].dev));
}
int lpcnet_batch_plc_reset(LPCNetBatch *b, int first, int count)
{
    NEED_PLC_ON(b);
    if (first < 0 || count < 0 || first + count > b->n) { set_err("PLC reset range"); return LPCN_E_ARG; }
    EACH_SHARD_IN(first, count, lpcn_batch_dev_plc_reset(s->dev, lfirst, lcount));
}
typedef struct { LPCNetBatch *b; short *pcm; const unsigned char *lost; } plc_step_args;
static int plc_step_shard(void *args, int k)
{
    const plc_step_args *a = (const plc_step_args *)args;
    const int f = a->b->at[k].first;
    return lpcn_batch_dev_plc_step_host(a->b->sh[k].dev, a->pcm + (size_t)f * LPCN_FRAME_SIZE, a->lost + f);
}
int lpcnet_batch_plc_step(LPCNetBatch *b, short *pcm, const unsigned char *lost)
{
    NEED_PLC_ON(b);
    if (!pcm || !lost) { set_err("lpcnet_batch_plc_step: bad arguments"); return LPCN_E_ARG; }
    plc_step_args a = {b, pcm, lost};
    return run_shards(b, plc_step_shard, &a);
}
int lpcnet_batch_plc_step_device_shard(LPCNetBatch *b, int shard, short *d_pcm, const unsigned char *lost, void *hip_stream)
{
    NEED_PLC_ON(b);
    if (shard < 0 || shard >= b->n_shards || !d_pcm || !lost) { set_err("lpcnet_batch_plc_step_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_plc_step(b->sh[shard].dev, d_pcm, lost, hip_stream));
}
int lpcnet_batch_plc_step_device(LPCNetBatch *b, short *d_pcm, const unsigned char *lost, void *hip_stream)
{
    NEED_PLC_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_plc_step_device");
    return lpcnet_batch_plc_step_device_shard(b, 0, d_pcm, lost, hip_stream);
}
int lpcnet_batch_plc_fec_add(LPCNetBatch *b, int stream, const float *features20)
{
    NEED_PLC_ON(b);
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_plc_fec_add(s->dev, i, features20));
}
int lpcnet_batch_plc_fec_clear(LPCNetBatch *b, int stream)
{
    NEED_PLC_ON(b);
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_plc_fec_clear(s->dev, i));
}
typedef struct { LPCNetBatch *b; const float *features; const int *count, *skip; const unsigned char *clear; int *dropped; const int *vec0; } fec_feed_args;
static int fec_feed_shard(void *args, int k)      /* (vec0[k]: shard k's first row of the packed vectors) */
{
    const fec_feed_args *a = (const fec_feed_args *)args;
    const int f = a->b->at[k].first;
    return lpcn_batch_dev_plc_fec_feed_host(a->b->sh[k].dev, a->features ? a->features + (size_t)a->vec0[k] * LPCN_NB_FEAT : NULL, a->count + f,
                                            a->skip ? a->skip + f : NULL, a->clear ? a->clear + f : NULL, a->dropped ? a->dropped + f : NULL);
}
/* every stream's FEC traffic in one call (include/lpcnet_batch.h) */
int lpcnet_batch_plc_fec_feed(LPCNetBatch *b, const float *features, const int *count, const int *skip, const unsigned char *clear, int *dropped)
{
    NEED_PLC_ON(b);
    if (!count) { set_err("lpcnet_batch_plc_fec_feed: bad arguments"); return LPCN_E_ARG; }
    int vec0[LPCN_MAX_SHARDS];
    long long total = 0;
    for (int k = 0; k < b->n_shards; k++) {          /* (checked for the whole batch before any shard's rings change) */
        vec0[k] = (int)total;
        const int active = lpcn_batch_dev_active(b->sh[k].dev);
        for (int i = b->at[k].first; i < b->at[k].first + b->at[k].count; i++) {
            const int inactive = i >= b->at[k].first + active;      /* (its skip and clear are ignored; vectors for it would make the packed array ambiguous) */
            if (inactive && count[i] != 0) { set_err("lpcnet_batch_plc_fec_feed: a stream beyond its shard's active prefix has a count"); return LPCN_E_ARG; }
            if (count[i] < 0 || (!inactive && skip && skip[i] < 0)) { set_err("lpcnet_batch_plc_fec_feed: negative count"); return LPCN_E_ARG; }
            if ((total += count[i]) > 0x7fffffff) { set_err("lpcnet_batch_plc_fec_feed: more than 2^31 - 1 vectors"); return LPCN_E_ARG; }
        }
    }
    if (total && !features) { set_err("lpcnet_batch_plc_fec_feed: bad arguments"); return LPCN_E_ARG; }
    fec_feed_args a = {b, features, count, skip, clear, dropped, vec0};
    return run_shards(b, fec_feed_shard, &a);
}
int lpcnet_batch_plc_fec_feed_device_shard(LPCNetBatch *b, int shard, const float *d_features, const int *count, const int *skip, const unsigned char *clear,
                                           int *dropped, void *hip_stream)
{
    NEED_PLC_ON(b);
    if (shard < 0 || shard >= b->n_shards || !count) { set_err("lpcnet_batch_plc_fec_feed_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_plc_fec_feed(b->sh[shard].dev, d_features, count, skip, clear, dropped, hip_stream));
}
int lpcnet_batch_plc_fec_feed_device(LPCNetBatch *b, const float *d_features, const int *count, const int *skip, const unsigned char *clear, int *dropped,
                                     void *hip_stream)
{
    NEED_PLC_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_plc_fec_feed_device");
    return lpcnet_batch_plc_fec_feed_device_shard(b, 0, d_features, count, skip, clear, dropped, hip_stream);
}
int lpcnet_batch_plc_state_size(void) { return (int)sizeof(lpcn_plc_state_rec); }
int lpcnet_batch_get_plc_state(LPCNetBatch *b, int stream, void *out)
{
    NEED_PLC_ON(b);
    if (!out) { set_err("lpcnet_batch_get_plc_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_get_plc_state(s->dev, i, (lpcn_plc_state_rec *)out));
}
int lpcnet_batch_set_plc_state(LPCNetBatch *b, int stream, const void *in)
{
    NEED_PLC_ON(b);
    if (!in) { set_err("lpcnet_batch_set_plc_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_set_plc_state(s->dev, i, (const lpcn_plc_state_rec *)in));
}
int lpcnet_batch_plc_burg(LPCNetBatch *b, const float *x, float *ceps36)
{
    NEED_PLC_ON(b);
    if (!x || !ceps36) { set_err("lpcnet_batch_plc_burg: bad arguments"); return LPCN_E_ARG; }
    EACH_SHARD(lpcn_batch_dev_plc_burg_host(s->dev, x + (size_t)at.first * LPCN_FRAME_SIZE, ceps36 + (size_t)at.first * 2 * LPCN_NB_BANDS));
}
int lpcnet_batch_plc_pred(LPCNetBatch *b, const float *in57, float *out20)
{
    NEED_PLC_ON(b);
    if (!in57 || !out20) { set_err("lpcnet_batch_plc_pred: bad arguments"); return LPCN_E_ARG; }
    EACH_SHARD(lpcn_batch_dev_plc_pred_host(s->dev, in57 + (size_t)at.first * LPCN_PLC_IN, out20 + (size_t)at.first * LPCN_NB_FEAT));
}
int lpcnet_batch_plc_set_pred_form(LPCNetBatch *b, int S) { NEED_PLC_ON(b); EACH_SHARD(lpcn_batch_dev_plc_pred_set_form(s->dev, S)); }
int lpcnet_batch_plc_get_pred_form(const LPCNetBatch *b, int n_streams)
{
    NEED_PLC_ON(b);
    const int rc = lpcn_batch_dev_plc_pred_form(b->sh[0].dev, n_streams);
    if (rc < 0) take_engine_err();
    return rc;
}
/* ---- DRED decoder (DRED_rdovae_decode_all per stream; include/lpcnet_batch.h) ---- */
#define NEED_DRED_ON(b) do { NEED_MODEL(b); if (!lpcn_batch_dev_dred_enabled((b)->sh[0].dev)) { set_err("the DRED decoder is not enabled on this batch (lpcnet_batch_dred_enable)"); return LPCN_E_MODEL; } } while (0)
int lpcnet_batch_dred_enable(LPCNetBatch *b, int max_latents) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_dred_enable(s->dev, max_latents)); }
int lpcnet_batch_dred_info(const LPCNetBatch *b, int *info)
{
    NEED_DRED_ON(b);
    if (!info) { set_err("lpcnet_batch_dred_info: bad arguments"); return LPCN_E_ARG; }
    info[0] = lpcn_batch_dev_dred_enabled(b->sh[0].dev);
    FWD(lpcn_batch_dev_dred_dims(b->sh[0].dev, &info[1], &info[2]));
}
int lpcnet_batch_dred_flavour(const LPCNetBatch *b)
{
    NEED_DRED_ON(b);
    FWD(lpcn_batch_dev_dred_flavour(b->sh[0].dev));
}
int lpcnet_batch_dred_set_form(LPCNetBatch *b, int S) { NEED_DRED_ON(b); EACH_SHARD(lpcn_batch_dev_dred_set_form(s->dev, S)); }
int lpcnet_batch_dred_get_form(const LPCNetBatch *b, int n_streams)
{
    NEED_DRED_ON(b);
    const int rc = lpcn_batch_dev_dred_form(b->sh[0].dev, n_streams);
    if (rc < 0) take_engine_err();
    return rc;
}
/* all shards or none: a shard that refuses puts the earlier ones back, so that a sharded batch never decodes in two arithmetics */
int lpcnet_batch_dred_set_fast(LPCNetBatch *b, int mode)
{
    NEED_DRED_ON(b);
    const int before = lpcn_batch_dev_dred_get_fast(b->sh[0].dev);
    for (int k = 0; k < b->n_shards; k++) {
        const int rc = lpcn_batch_dev_dred_set_fast(b->sh[k].dev, mode);
        if (rc) {
            take_engine_err();
            while (k-- > 0) lpcn_batch_dev_dred_set_fast(b->sh[k].dev, before);
            return rc;
        }
    }
    return 0;
}
int lpcnet_batch_dred_get_fast(const LPCNetBatch *b)
{
    NEED_DRED_ON(b);
    FWD(lpcn_batch_dev_dred_get_fast(b->sh[0].dev));
}
typedef struct { LPCNetBatch *b; const float *state, *latents; const int *count; float *features; int max_latents, latent_dim, state_dim; } dred_args;
static int dred_shard(void *args, int k)
{
    const dred_args *a = (const dred_args *)args;
    const size_t f = (size_t)a->b->at[k].first;
    return lpcn_batch_dev_dred_decode_host(a->b->sh[k].dev, a->state + f * a->state_dim, a->latents + f * a->max_latents * a->latent_dim, a->count + f,
                                           a->features + f * LPCN_DRED_FRAMES * a->max_latents * LPCN_NB_FEAT);
}
int lpcnet_batch_dred_decode(LPCNetBatch *b, const float *state, const float *latents, const int *count, float *features)
{
    NEED_DRED_ON(b);
    if (!state || !latents || !count || !features) { set_err("lpcnet_batch_dred_decode: bad arguments"); return LPCN_E_ARG; }
    for (int k = 0; k < b->n_shards; k++) {          /* (checked for the whole batch before any shard writes) */
        const int rc = lpcn_batch_dev_dred_check(b->sh[k].dev, count + b->at[k].first, NULL, NULL, NULL);
        if (rc) { take_engine_err(); return rc; }
    }
    dred_args a = {b, state, latents, count, features, lpcn_batch_dev_dred_enabled(b->sh[0].dev), 0, 0};
    lpcn_batch_dev_dred_dims(b->sh[0].dev, &a.latent_dim, &a.state_dim);
    return run_shards(b, dred_shard, &a);
}
int lpcnet_batch_dred_decode_device_shard(LPCNetBatch *b, int shard, const float *d_state, const float *d_latents, const int *count, float *d_features,
                                          void *hip_stream)
{
    NEED_DRED_ON(b);
    if (shard < 0 || shard >= b->n_shards || !count) { set_err("lpcnet_batch_dred_decode_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_decode(b->sh[shard].dev, d_state, d_latents, count, d_features, hip_stream));
}
int lpcnet_batch_dred_decode_device(LPCNetBatch *b, const float *d_state, const float *d_latents, const int *count, float *d_features, void *hip_stream)
{
    NEED_DRED_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_dred_decode_device");
    return lpcnet_batch_dred_decode_device_shard(b, 0, d_state, d_latents, count, d_features, hip_stream);
}
int lpcnet_batch_dred_decode_packed_device_shard(LPCNetBatch *b, int shard, const float *d_state, const float *d_latents, const int *count, const int *first,
                                                 const int *take, float *d_packed, void *hip_stream)
{
    NEED_DRED_ON(b);
    if (shard < 0 || shard >= b->n_shards || !count || !first || !take) { set_err("lpcnet_batch_dred_decode_packed_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_decode_packed(b->sh[shard].dev, d_state, d_latents, count, first, take, d_packed, hip_stream));
}
int lpcnet_batch_dred_decode_packed_device(LPCNetBatch *b, const float *d_state, const float *d_latents, const int *count, const int *first, const int *take,
                                           float *d_packed, void *hip_stream)
{
    NEED_DRED_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_dred_decode_packed_device");
    return lpcnet_batch_dred_decode_packed_device_shard(b, 0, d_state, d_latents, count, first, take, d_packed, hip_stream);
}

/* ---- the DRED decoder as a per-stream state (DRED_rdovae_dec_init_states / DRED_rdovae_decode_qframe per stream; include/lpcnet_batch.h) ---- */
#define NEED_DRED_STATE_ON(b) do { NEED_DRED_ON(b); if (!lpcn_batch_dev_dred_state_enabled((b)->sh[0].dev)) { set_err("the DRED decoder's per-stream state is not enabled on this batch (lpcnet_batch_dred_state_enable)"); return LPCN_E_MODEL; } } while (0)
int lpcnet_batch_dred_state_enable(LPCNetBatch *b) { NEED_DRED_ON(b); EACH_SHARD(lpcn_batch_dev_dred_state_enable(s->dev)); }
int lpcnet_batch_dred_dec_state_size(const LPCNetBatch *b)
{
    NEED_DRED_STATE_ON(b);
    return lpcn_batch_dev_dred_state_enabled(b->sh[0].dev);
}
int lpcnet_batch_get_dred_dec_state(LPCNetBatch *b, int stream, float *out)
{
    NEED_DRED_STATE_ON(b);
    if (!out) { set_err("lpcnet_batch_get_dred_dec_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_dred_get_dec_state(s->dev, i, out));
}
int lpcnet_batch_set_dred_dec_state(LPCNetBatch *b, int stream, const float *in)
{
    NEED_DRED_STATE_ON(b);
    if (!in) { set_err("lpcnet_batch_set_dred_dec_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_dred_set_dec_state(s->dev, i, in));
}
typedef struct { LPCNetBatch *b; const float *state, *latents; const int *which, *start, *count; float *features; int max_latents, latent_dim, state_dim; } dred_stream_args;
static int dred_init_shard(void *args, int k)
{
    const dred_stream_args *a = (const dred_stream_args *)args;
    const size_t f = (size_t)a->b->at[k].first;
    return lpcn_batch_dev_dred_init_host(a->b->sh[k].dev, a->state + f * a->state_dim, a->which ? a->which + f : NULL);
}
static int dred_step_shard(void *args, int k)
{
    const dred_stream_args *a = (const dred_stream_args *)args;
    const size_t f = (size_t)a->b->at[k].first;
    return lpcn_batch_dev_dred_step_host(a->b->sh[k].dev, a->latents + f * a->max_latents * a->latent_dim, a->start + f, a->count + f,
                                         a->features + f * LPCN_DRED_FRAMES * a->max_latents * LPCN_NB_FEAT);
}
int lpcnet_batch_dred_init(LPCNetBatch *b, const float *state, const int *which)
{
    NEED_DRED_STATE_ON(b);
    if (!state) { set_err("lpcnet_batch_dred_init: bad arguments"); return LPCN_E_ARG; }
    for (int k = 0; k < b->n_shards; k++) {          /* (checked for the whole batch before any shard writes) */
        const int rc = lpcn_batch_dev_dred_init_check(b->sh[k].dev, which ? which + b->at[k].first : NULL);
        if (rc) { take_engine_err(); return rc; }
    }
    dred_stream_args a = {b, state, NULL, which, NULL, NULL, NULL, 0, 0, 0};
    lpcn_batch_dev_dred_dims(b->sh[0].dev, &a.latent_dim, &a.state_dim);
    return run_shards(b, dred_init_shard, &a);
}
int lpcnet_batch_dred_step(LPCNetBatch *b, const float *latents, const int *start, const int *count, float *features)
{
    NEED_DRED_STATE_ON(b);
    if (!latents || !start || !count || !features) { set_err("lpcnet_batch_dred_step: bad arguments"); return LPCN_E_ARG; }
    for (int k = 0; k < b->n_shards; k++) {          /* (checked for the whole batch before any shard writes or advances) */
        const int rc = lpcn_batch_dev_dred_step_check(b->sh[k].dev, start + b->at[k].first, count + b->at[k].first, 0, 0, NULL, NULL, NULL);
        if (rc) { take_engine_err(); return rc; }
    }
    dred_stream_args a = {b, NULL, latents, NULL, start, count, features, lpcn_batch_dev_dred_enabled(b->sh[0].dev), 0, 0};
    lpcn_batch_dev_dred_dims(b->sh[0].dev, &a.latent_dim, &a.state_dim);
    return run_shards(b, dred_step_shard, &a);
}
int lpcnet_batch_dred_init_device_shard(LPCNetBatch *b, int shard, const float *d_state, const int *which, void *hip_stream)
{
    NEED_DRED_STATE_ON(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("lpcnet_batch_dred_init_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_init(b->sh[shard].dev, d_state, which, hip_stream));
}
int lpcnet_batch_dred_init_device(LPCNetBatch *b, const float *d_state, const int *which, void *hip_stream)
{
    NEED_DRED_STATE_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_dred_init_device");
    return lpcnet_batch_dred_init_device_shard(b, 0, d_state, which, hip_stream);
}
int lpcnet_batch_dred_step_device_shard(LPCNetBatch *b, int shard, const float *d_latents, const int *start, const int *count, int first_latent, int n_latents,
                                        float *d_features, void *hip_stream)
{
    NEED_DRED_STATE_ON(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("lpcnet_batch_dred_step_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_step(b->sh[shard].dev, d_latents, start, count, first_latent, n_latents, d_features, hip_stream));
}
int lpcnet_batch_dred_step_device(LPCNetBatch *b, const float *d_latents, const int *start, const int *count, int first_latent, int n_latents, float *d_features,
                                  void *hip_stream)
{
    NEED_DRED_STATE_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_dred_step_device");
    return lpcnet_batch_dred_step_device_shard(b, 0, d_latents, start, count, first_latent, n_latents, d_features, hip_stream);
}
int lpcnet_batch_dred_step_packed_device_shard(LPCNetBatch *b, int shard, const float *d_latents, const int *start, const int *count, const int *first,
                                               const int *take, float *d_packed, void *hip_stream)
{
    NEED_DRED_STATE_ON(b);
    if (shard < 0 || shard >= b->n_shards || !start || !count || !first || !take) { set_err("lpcnet_batch_dred_step_packed_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_step_packed(b->sh[shard].dev, d_latents, start, count, first, take, d_packed, hip_stream));
}
int lpcnet_batch_dred_step_packed_device(LPCNetBatch *b, const float *d_latents, const int *start, const int *count, const int *first, const int *take,
                                         float *d_packed, void *hip_stream)
{
    NEED_DRED_STATE_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_dred_step_packed_device");
    return lpcnet_batch_dred_step_packed_device_shard(b, 0, d_latents, start, count, first, take, d_packed, hip_stream);
}

/* ---- DRED encoder (DRED_rdovae_encode_dframe per stream and double frame; include/lpcnet_batch.h) ---- */
#define NEED_DENC_ON(b) do { NEED_MODEL(b); if (!lpcn_batch_dev_dred_enc_enabled((b)->sh[0].dev)) { set_err("the DRED encoder is not enabled on this batch (lpcnet_batch_dred_enc_enable)"); return LPCN_E_MODEL; } } while (0)
int lpcnet_batch_dred_enc_enable(LPCNetBatch *b, int max_dframes) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_dred_enc_enable(s->dev, max_dframes)); }
int lpcnet_batch_dred_enc_info(const LPCNetBatch *b, int *info)
{
    NEED_DENC_ON(b);
    if (!info) { set_err("lpcnet_batch_dred_enc_info: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_enc_info(b->sh[0].dev, info));
}
int lpcnet_batch_dred_enc_flavour(const LPCNetBatch *b)
{
    NEED_DENC_ON(b);
    FWD(lpcn_batch_dev_dred_enc_flavour(b->sh[0].dev));
}
int lpcnet_batch_dred_enc_set_form(LPCNetBatch *b, int S) { NEED_DENC_ON(b); EACH_SHARD(lpcn_batch_dev_dred_enc_set_form(s->dev, S)); }
int lpcnet_batch_dred_enc_get_form(const LPCNetBatch *b, int n_streams)
{
    NEED_DENC_ON(b);
    const int rc = lpcn_batch_dev_dred_enc_form(b->sh[0].dev, n_streams);
    if (rc < 0) take_engine_err();
    return rc;
}
/* all shards or none, like the decoder's switch: a sharded batch never encodes in two arithmetics */
int lpcnet_batch_dred_enc_set_fast(LPCNetBatch *b, int mode)
{
    NEED_DENC_ON(b);
    const int before = lpcn_batch_dev_dred_enc_get_fast(b->sh[0].dev);
    for (int k = 0; k < b->n_shards; k++) {
        const int rc = lpcn_batch_dev_dred_enc_set_fast(b->sh[k].dev, mode);
        if (rc) {
            take_engine_err();
            while (k-- > 0) lpcn_batch_dev_dred_enc_set_fast(b->sh[k].dev, before);
            return rc;
        }
    }
    return 0;
}
int lpcnet_batch_dred_enc_get_fast(const LPCNetBatch *b)
{
    NEED_DENC_ON(b);
    FWD(lpcn_batch_dev_dred_enc_get_fast(b->sh[0].dev));
}
typedef struct { LPCNetBatch *b; const float *features; int stride; const int *count; float *latents, *initial; int info[7]; } denc_args;
static int denc_shard(void *args, int k)
{
    const denc_args *a = (const denc_args *)args;
    const size_t f = (size_t)a->b->at[k].first, md = (size_t)a->info[0];
    return lpcn_batch_dev_dred_encode_host(a->b->sh[k].dev, a->features + f * 2 * md * a->stride, a->stride, a->count + f, a->latents + f * md * a->info[2],
                                           a->initial + f * md * a->info[3]);
}
int lpcnet_batch_dred_encode(LPCNetBatch *b, const float *features, int stride, const int *count, float *latents, float *initial_state)
{
    NEED_DENC_ON(b);
    if (!features || !count || !latents || !initial_state) { set_err("lpcnet_batch_dred_encode: bad arguments"); return LPCN_E_ARG; }
    for (int k = 0; k < b->n_shards; k++) {          /* (checked for the whole batch before any shard writes or advances) */
        const int rc = lpcn_batch_dev_dred_enc_check(b->sh[k].dev, count + b->at[k].first, 0, stride);
        if (rc) { take_engine_err(); return rc; }
    }
    denc_args a = {b, features, stride, count, latents, initial_state, {0}};
    lpcn_batch_dev_dred_enc_info(b->sh[0].dev, a.info);
    return run_shards(b, denc_shard, &a);
}
int lpcnet_batch_dred_encode_device_shard(LPCNetBatch *b, int shard, const float *d_features, int stride, const int *count, int n_dframes, float *d_latents,
                                          float *d_initial_state, void *hip_stream)
{
    NEED_DENC_ON(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("lpcnet_batch_dred_encode_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_dred_encode(b->sh[shard].dev, d_features, stride, count, n_dframes, d_latents, d_initial_state, hip_stream));
}
int lpcnet_batch_dred_encode_device(LPCNetBatch *b, const float *d_features, int stride, const int *count, int n_dframes, float *d_latents, float *d_initial_state,
                                    void *hip_stream)
{
    NEED_DENC_ON(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_dred_encode_device");
    return lpcnet_batch_dred_encode_device_shard(b, 0, d_features, stride, count, n_dframes, d_latents, d_initial_state, hip_stream);
}
int lpcnet_batch_dred_enc_get_state(LPCNetBatch *b, int stream, float *out)
{
    NEED_DENC_ON(b);
    if (!out) { set_err("lpcnet_batch_dred_enc_get_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_dred_enc_get_state(s->dev, i, out));
}
int lpcnet_batch_dred_enc_set_state(LPCNetBatch *b, int stream, const float *in)
{
    NEED_DENC_ON(b);
    if (!in) { set_err("lpcnet_batch_dred_enc_set_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_dred_enc_set_state(s->dev, i, in));
}

/* ---- feature analysis (lpcnet_compute_single_frame_features per stream and frame; include/lpcnet_batch.h) ---- */
typedef struct { LPCNetBatch *b; const void *pcm; int is_float; float *features; int feat_stride, n_frames; } analyze_args;
static int analyze_shard(void *args, int k)
{
    const analyze_args *a = (const analyze_args *)args;
    const size_t o = (size_t)a->b->at[k].first * a->n_frames, op = o * LPCN_FRAME_SIZE;
    return lpcn_batch_dev_analyze_host(a->b->sh[k].dev, a->is_float ? (const void *)((const float *)a->pcm + op) : (const void *)((const short *)a->pcm + op),
                                       a->is_float, a->features + o * a->feat_stride, a->feat_stride, a->n_frames);
}
static int analyze_host(LPCNetBatch *b, const void *pcm, int is_float, float *features, int feat_stride, int n_frames)
{
    NEED_MODEL(b);
    if (!pcm || !features || n_frames < 1 || feat_stride < LPCN_AN_NB_FEATURES) { set_err("lpcnet_batch_analyze: bad arguments"); return LPCN_E_ARG; }
    analyze_args a = {b, pcm, is_float, features, feat_stride, n_frames};
    return run_shards(b, analyze_shard, &a);
}
int lpcnet_batch_analyze(LPCNetBatch *b, const short *pcm, float *features, int feat_stride, int n_frames)
{
    return analyze_host(b, pcm, 0, features, feat_stride, n_frames);
}
int lpcnet_batch_analyze_float(LPCNetBatch *b, const float *pcm, float *features, int feat_stride, int n_frames)
{
    return analyze_host(b, pcm, 1, features, feat_stride, n_frames);
}
int lpcnet_batch_analyze_device_shard(LPCNetBatch *b, int shard, const void *d_pcm, int pcm_is_float, float *d_features, int feat_stride,
                                      int n_frames, void *hip_stream)
{
    NEED_MODEL(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("shard index"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_analyze(b->sh[shard].dev, d_pcm, pcm_is_float, d_features, feat_stride, n_frames, hip_stream));
}
int lpcnet_batch_analyze_device(LPCNetBatch *b, const void *d_pcm, int pcm_is_float, float *d_features, int feat_stride, int n_frames,
                                void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_analyze_device");
    return lpcnet_batch_analyze_device_shard(b, 0, d_pcm, pcm_is_float, d_features, feat_stride, n_frames, hip_stream);
}
int lpcnet_batch_analysis_enable(LPCNetBatch *b, int max_frames) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_analysis_enable(s->dev, max_frames)); }
int lpcnet_batch_analysis_reset(LPCNetBatch *b, int first, int count)
{
    NEED_MODEL(b);
    if (first < 0 || count < 0 || first + count > b->n) { set_err("analysis reset range"); return LPCN_E_ARG; }
    EACH_SHARD_IN(first, count, lpcn_batch_dev_analysis_reset(s->dev, lfirst, lcount));
}
int lpcnet_batch_analysis_state_size(void) { return (int)sizeof(lpcn_analysis_state); }
int lpcnet_batch_get_analysis_state(LPCNetBatch *b, int stream, void *out)
{
    NEED_MODEL(b);
    if (!out) { set_err("lpcnet_batch_get_analysis_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_get_analysis_state(s->dev, i, (lpcn_analysis_state *)out));
}
int lpcnet_batch_set_analysis_state(LPCNetBatch *b, int stream, const void *in)
{
    NEED_MODEL(b);
    if (!in) { set_err("lpcnet_batch_set_analysis_state: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_set_analysis_state(s->dev, i, (const lpcn_analysis_state *)in));
}

typedef struct { LPCNetBatch *b; const short *pcm; unsigned char *packets; float *features; int feat_stride, n_packets; } encode_args;      /* packets or features */
static int encode_shard(void *args, int k)
{
    const encode_args *a = (const encode_args *)args;
    const size_t o = (size_t)a->b->at[k].first * a->n_packets;
    return lpcn_batch_dev_encode_host(a->b->sh[k].dev, a->pcm + o * 4 * LPCN_FRAME_SIZE, a->packets ? a->packets + o * 8 : NULL,
                                      a->features ? a->features + o * 4 * a->feat_stride : NULL, a->feat_stride, a->n_packets);
}
/* ---- encoder (lpcnet_encode / lpcnet_compute_features per stream and packet; include/lpcnet_batch.h) ---- */
int lpcnet_batch_encode(LPCNetBatch *b, const short *pcm, unsigned char *packets, int n_packets)
{
    NEED_MODEL(b);
    if (!pcm || !packets || n_packets < 1) { set_err("lpcnet_batch_encode: bad arguments"); return LPCN_E_ARG; }
    int rc = batch_codebooks(b);
    if (rc) return rc;
    encode_args a = {b, pcm, packets, NULL, 0, n_packets};
    return run_shards(b, encode_shard, &a);
}
int lpcnet_batch_encode_device_shard(LPCNetBatch *b, int shard, const short *d_pcm, unsigned char *d_packets, int n_packets, void *hip_stream)
{
    NEED_MODEL(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("shard index"); return LPCN_E_ARG; }
    if (!d_pcm || !d_packets || n_packets < 1) { set_err("lpcnet_batch_encode_device: bad arguments"); return LPCN_E_ARG; }
    int rc = batch_codebooks(b);
    if (rc) return rc;
    FWD(lpcn_batch_dev_encode(b->sh[shard].dev, d_pcm, d_packets, n_packets, hip_stream));
}
int lpcnet_batch_encode_device(LPCNetBatch *b, const short *d_pcm, unsigned char *d_packets, int n_packets, void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_encode_device");
    return lpcnet_batch_encode_device_shard(b, 0, d_pcm, d_packets, n_packets, hip_stream);
}
int lpcnet_batch_compute_features(LPCNetBatch *b, const short *pcm, float *features, int feat_stride, int n_packets)
{
    NEED_MODEL(b);
    if (!pcm || !features || n_packets < 1 || feat_stride < LPCN_AN_NB_FEATURES) { set_err("lpcnet_batch_compute_features: bad arguments"); return LPCN_E_ARG; }
    encode_args a = {b, pcm, NULL, features, feat_stride, n_packets};
    return run_shards(b, encode_shard, &a);
}
int lpcnet_batch_compute_features_device(LPCNetBatch *b, const short *d_pcm, float *d_features, int feat_stride, int n_packets, void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_compute_features_device");
    if (!d_pcm || !d_features || n_packets < 1 || feat_stride < LPCN_AN_NB_FEATURES) { set_err("lpcnet_batch_compute_features_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_compute_features(b->sh[0].dev, d_pcm, d_features, feat_stride, n_packets, hip_stream));
}
int lpcnet_batch_encoder_enable(LPCNetBatch *b, int max_packets) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_encoder_enable(s->dev, max_packets)); }
int lpcnet_batch_get_encoder_vq_mem(LPCNetBatch *b, int stream, float *out18)
{
    NEED_MODEL(b);
    if (!out18) { set_err("lpcnet_batch_get_encoder_vq_mem: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_get_encoder_vq_mem(s->dev, i, out18));
}
int lpcnet_batch_set_encoder_vq_mem(LPCNetBatch *b, int stream, const float *in18)
{
    NEED_MODEL(b);
    if (!in18) { set_err("lpcnet_batch_set_encoder_vq_mem: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_set_encoder_vq_mem(s->dev, i, in18));
}

int lpcnet_batch_get_decoder_vq_mem(LPCNetBatch *b, int stream, float *out18)
{
    NEED_MODEL(b);
    if (!out18) { set_err("lpcnet_batch_get_decoder_vq_mem: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_get_decoder_vq_mem(s->dev, i, out18));
}
int lpcnet_batch_set_decoder_vq_mem(LPCNetBatch *b, int stream, const float *in18)
{
    NEED_MODEL(b);
    if (!in18) { set_err("lpcnet_batch_set_decoder_vq_mem: bad arguments"); return LPCN_E_ARG; }
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_set_decoder_vq_mem(s->dev, i, in18));
}

/* ---- streams that come and go (include/lpcnet_batch.h): the active prefix of every shard and the device-side stream copies; which pair lists
 * are valid and how they split over the shards is api_roster.h ---- */
int lpcnet_batch_set_active(LPCNetBatch *b, const int *active, int n_shards)
{
    NEED_MODEL(b);
    if (!active || n_shards != b->n_shards) { set_err("lpcnet_batch_set_active: one count per shard (lpcnet_batch_shards)"); return LPCN_E_ARG; }
    for (int k = 0; k < n_shards; k++)       /* (checked for every shard before any shard changes) */
        if (active[k] < 0 || active[k] > b->at[k].count) { set_err("lpcnet_batch_set_active: a count outside 0 .. the shard's streams"); return LPCN_E_ARG; }
    for (int k = 0; k < n_shards; k++) { const int rc = lpcn_batch_dev_set_active(b->sh[k].dev, active[k]); if (rc) { take_engine_err(); return rc; } }
    return 0;
}
int lpcnet_batch_get_active(const LPCNetBatch *b, int *active, int cap)
{
    NEED_MODEL(b);
    for (int k = 0; active && k < b->n_shards && k < cap; k++) active[k] = lpcn_batch_dev_active(b->sh[k].dev);
    return b->n_shards;
}
int lpcnet_batch_active_streams(const LPCNetBatch *b)
{
    NEED_MODEL(b);
    int sum = 0;
    for (int k = 0; k < b->n_shards; k++) sum += lpcn_batch_dev_active(b->sh[k].dev);
    return sum;
}
static int copy_pairs_between(LPCNetBatch *from, const int *src, LPCNetBatch *to, const int *dst, int m);
int lpcnet_batch_copy_streams(LPCNetBatch *b, const int *src, const int *dst, int m, void *hip_stream)
{
    NEED_MODEL(b);
    if (m < 0 || (m && (!src || !dst))) { set_err("lpcnet_batch_copy_streams: bad arguments"); return LPCN_E_ARG; }
    if (hip_stream && b->n_shards != 1) { set_err("lpcnet_batch_copy_streams: a sharded batch copies on its shards' own streams (hip_stream must be NULL)"); return LPCN_E_ARG; }
    if (!m) return 0;
    /* scratch: the marks of the check, then the split's four lists */
    unsigned char *mark = (unsigned char *)malloc((size_t)b->n + 4 * (size_t)m * sizeof(int) + sizeof(int));
    if (!mark) { set_err("lpcnet_batch_copy_streams: out of memory"); return LPCN_E_ARG; }
    int rc = roster_check(b->at, b->n_shards, src, dst, m, mark);
    if (rc) {
        set_err("lpcnet_batch_copy_streams: every index must lie inside the batch, all destinations be distinct and no stream be both a source and a destination");
        free(mark);
        return LPCN_E_ARG;
    }
    int *lsrc = (int *)(mark + ((size_t)b->n + sizeof(int) - 1) / sizeof(int) * sizeof(int)), *ldst = lsrc + m, *xsrc = ldst + m, *xdst = xsrc + m;
    int first[LPCN_MAX_SHARDS + 1];
    const int nx = roster_split(b->at, b->n_shards, src, dst, m, first, lsrc, ldst, xsrc, xdst);
    for (int k = 0; k < b->n_shards && !rc; k++)         /* one upload and one launch per shard, only enqueued */
        if (first[k + 1] > first[k]) rc = lpcn_batch_dev_copy_streams(b->sh[k].dev, lsrc + first[k], ldst + first[k], first[k + 1] - first[k], hip_stream);
    if (rc) take_engine_err();
    else if (nx) rc = copy_pairs_between(b, xsrc, b, xdst, nx);      /* across shards: one gather, one transfer and one scatter per shard pair, only enqueued */
    free(mark);
    return rc;
}

/* ---- stream snapshots (include/lpcnet_batch.h; the record, its layout and the blob are snapshot_plan.h) ---- */
/* the batch's present layout: shard 0's with the model's hash; every shard must have the same sections (a copy across shards can enable a
 * subsystem in one shard alone: such a batch is brought level with the lpcnet_batch_*_enable calls) */
static int batch_layout(const LPCNetBatch *b, int *lay)
{
    int other[LPCN_SNAP_LAYOUT_MAX];
    int n = lpcn_batch_dev_snapshot_layout(b->sh[0].dev, lay);
    if (n < 0) { take_engine_err(); return n; }
    for (int k = 1; k < b->n_shards; k++) {
        const int nk = lpcn_batch_dev_snapshot_layout(b->sh[k].dev, other);
        if (nk < 0) { take_engine_err(); return nk; }
        if (nk != n || memcmp(other, lay, sizeof(int) * (size_t)n)) { set_err("snapshot: the shards of the batch have different subsystems enabled"); return LPCN_E_MODEL; }
    }
    lay[SNAP_L_HASH_LO] = (int)(unsigned)(b->model_hash & 0xffffffffu); lay[SNAP_L_HASH_HI] = (int)(unsigned)(b->model_hash >> 32);
    return n;
}
int lpcnet_batch_snapshot_layout(const LPCNetBatch *b, int *sections, int cap, int *record_bytes)
{
    NEED_MODEL(b);
    int lay[LPCN_SNAP_LAYOUT_MAX];
    if (cap < 0 || (cap && !sections)) { set_err("lpcnet_batch_snapshot_layout: bad arguments"); return LPCN_E_ARG; }
    const int n = batch_layout(b, lay);
    if (n < 0) return n;
    for (int k = 0; k < lay[SNAP_L_SECTIONS] && k < cap; k++) memcpy(sections + 3 * k, snap_section(lay, k), sizeof(int) * 3);
    if (record_bytes) *record_bytes = lay[SNAP_L_RECORD];
    return lay[SNAP_L_SECTIONS];
}
size_t lpcnet_batch_snapshot_bytes(const LPCNetBatch *b, int m)
{
    int lay[LPCN_SNAP_LAYOUT_MAX];
    if (!b || !b->n_shards || !b->sh[0].dev || m < 0 || batch_layout(b, lay) < 0) return 0;
    return snap_blob_bytes(lay, m);
}
/* a list of the batch's streams, distinct: the streams of shard k in the shard's own indices at ls [first[k], first[k + 1]) with the list entry each
 * came from in pos; ls and pos hold m ints each, mark one byte per stream of the batch.  0, or -1 - i with i the first bad entry */
static int snapshot_split(const LPCNetBatch *b, const int *streams, int m, int *first, int *ls, int *pos, unsigned char *mark)
{
    int fill[LPCN_MAX_SHARDS], local = 0;
    memset(mark, 0, (size_t)b->n);
    for (int k = 0; k <= b->n_shards; k++) first[k] = 0;
    for (int i = 0; i < m; i++) {
        const int k = shard_of(b->at, b->n_shards, streams[i], &local);
        if (k < 0 || mark[streams[i]]) return -1 - i;
        mark[streams[i]] = 1;
        first[k + 1]++;
    }
    for (int k = 0; k < b->n_shards; k++) { first[k + 1] += first[k]; fill[k] = first[k]; }
    for (int i = 0; i < m; i++) {
        const int k = shard_of(b->at, b->n_shards, streams[i], &local);
        ls[fill[k]] = local; pos[fill[k]++] = i;
    }
    return 0;
}
typedef struct { LPCNetBatch *b; const int *first, *ls, *pos; char *records; int *meta; const char *in_records; const int *in_meta, *layout; } snap_args;
static int snapshot_shard(void *args, int k)
{
    const snap_args *a = (const snap_args *)args;
    const int f = a->first[k], cnt = a->first[k + 1] - f;
    if (!cnt) return 0;
    if (a->layout) return lpcn_batch_dev_restore_host(a->b->sh[k].dev, a->ls + f, a->pos + f, cnt, a->in_records, a->in_meta, a->layout);
    return lpcn_batch_dev_snapshot_host(a->b->sh[k].dev, a->ls + f, a->pos + f, cnt, a->records, a->meta);
}
/* the split of a list for the host forms, in one allocation: *scratch is the caller's to free */
static int snapshot_lists(LPCNetBatch *b, const int *streams, int m, int *first, int **ls, int **pos, void **scratch, const char *what)
{
    char msg[160];
    if (m < 0 || m > b->n || (m && !streams)) { snprintf(msg, sizeof(msg), "%s: bad arguments", what); set_err(msg); return LPCN_E_ARG; }
    int *mem = (int *)malloc(2 * (size_t)(m + 1) * sizeof(int) + (size_t)b->n);
    if (!mem) { set_err("snapshot: out of memory"); return LPCN_E_ARG; }
    *ls = mem; *pos = mem + m + 1; *scratch = mem;
    const int bad = snapshot_split(b, streams, m, first, *ls, *pos, (unsigned char *)(mem + 2 * (m + 1)));
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: entry %d (stream %d) lies outside the batch's %d streams or is listed twice", what, -1 - bad, streams[-1 - bad], b->n);
        set_err(msg); free(mem); return LPCN_E_ARG;
    }
    return 0;
}
int lpcnet_batch_snapshot(LPCNetBatch *b, const int *streams, int m, void *buf, size_t cap)
{
    NEED_MODEL(b);
    int lay[LPCN_SNAP_LAYOUT_MAX], first[LPCN_MAX_SHARDS + 1], *ls, *pos, *meta;
    void *scratch;
    char *records;
    int rc = batch_layout(b, lay);
    if (rc < 0) return rc;
    if ((rc = snapshot_lists(b, streams, m, first, &ls, &pos, &scratch, "lpcnet_batch_snapshot"))) return rc;
    if (snap_blob_begin(buf, cap, lay, m, &meta, &records)) { set_err("lpcnet_batch_snapshot: the buffer is NULL, not 4-byte aligned or smaller than lpcnet_batch_snapshot_bytes"); free(scratch); return LPCN_E_ARG; }
    snap_args a = {b, first, ls, pos, records, meta, NULL, NULL, NULL};
    rc = run_shards(b, snapshot_shard, &a);
    free(scratch);
    return rc;
}
int lpcnet_batch_restore(LPCNetBatch *b, const int *streams, int m, const void *buf, size_t len)
{
    NEED_MODEL(b);
    int lay[LPCN_SNAP_LAYOUT_MAX], first[LPCN_MAX_SHARDS + 1], *ls, *pos, have = 0, need = 0;
    const int *meta;
    const char *records;
    void *scratch;
    if (snap_blob_parse(buf, len, &have, lay, &meta, &records)) { set_err("lpcnet_batch_restore: not a snapshot blob (NULL, truncated, wrong magic or version, or lengths that do not add up)"); return LPCN_E_ARG; }
    if (m > have) { set_err("lpcnet_batch_restore: the blob holds fewer records"); return LPCN_E_ARG; }
    int rc = snapshot_lists(b, streams, m, first, &ls, &pos, &scratch, "lpcnet_batch_restore");
    if (rc) return rc;
    for (int k = 0; k < b->n_shards && rc >= 0; k++) {   /* (every shard is asked before any shard changes) */
        rc = lpcn_batch_dev_snapshot_match(b->sh[k].dev, lay, 0);
        if (rc > 0) need = 1;
    }
    if (rc < 0) { take_engine_err(); free(scratch); return rc; }
    for (int k = 0; need && k < b->n_shards; k++)
        if ((rc = lpcn_batch_dev_snapshot_enable(b->sh[k].dev, lay))) { take_engine_err(); free(scratch); return rc; }
    snap_args a = {b, first, ls, pos, NULL, NULL, records, meta, lay};
    rc = run_shards(b, snapshot_shard, &a);
    free(scratch);
    return rc;
}
int lpcnet_batch_snapshot_device_shard(LPCNetBatch *b, int shard, const int *streams, int m, void *d_records, int *meta, void *hip_stream)
{
    NEED_MODEL(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("shard index"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_snapshot(b->sh[shard].dev, streams, m, d_records, meta, hip_stream));
}
int lpcnet_batch_snapshot_device(LPCNetBatch *b, const int *streams, int m, void *d_records, int *meta, void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_snapshot_device");
    return lpcnet_batch_snapshot_device_shard(b, 0, streams, m, d_records, meta, hip_stream);
}
int lpcnet_batch_restore_device_shard(LPCNetBatch *b, int shard, const int *streams, int m, const void *d_records, const int *meta,
                                      const int *sections, int n_sections, void *hip_stream)
{
    NEED_MODEL(b);
    if (shard < 0 || shard >= b->n_shards) { set_err("shard index"); return LPCN_E_ARG; }
    int lay[LPCN_SNAP_LAYOUT_MAX];
    if (!sections || n_sections < 1 || n_sections > LPCN_SNAP_MAX_SECTIONS) { set_err("lpcnet_batch_restore_device: bad section table"); return LPCN_E_ARG; }
    /* the head fields do not travel in a section table: the batch's own stand in, and the sections decide */
    if (lpcn_batch_dev_snapshot_layout(b->sh[shard].dev, lay) < 0) { take_engine_err(); return LPCN_E_HIP; }
    memcpy(lay + SNAP_L_HEAD, sections, sizeof(int) * 3 * (size_t)n_sections);
    lay[SNAP_L_SECTIONS] = n_sections;
    lay[SNAP_L_RECORD] = (sections[3 * (n_sections - 1) + 1] + sections[3 * (n_sections - 1) + 2] + 15) / 16 * 16;
    if (!snap_layout_valid(lay, SNAP_L_HEAD + 3 * n_sections)) { set_err("lpcnet_batch_restore_device: bad section table"); return LPCN_E_ARG; }
    FWD(lpcn_batch_dev_restore(b->sh[shard].dev, streams, m, d_records, meta, lay, hip_stream));
}
int lpcnet_batch_restore_device(LPCNetBatch *b, const int *streams, int m, const void *d_records, const int *meta, const int *sections, int n_sections,
                                void *hip_stream)
{
    NEED_MODEL(b);
    NEED_ONE_SHARD(b, "lpcnet_batch_restore_device");
    return lpcnet_batch_restore_device_shard(b, 0, streams, m, d_records, meta, sections, n_sections, hip_stream);
}
/* Pairs between two batches (or two shards of one), shard pair by shard pair: the pairs from shard ks of `from` to shard kd of `to` are one gather,
 * one transfer and one scatter (lpcn_batch_dev_copy_streams_to).  The indices are the batches' own and lie inside them. */
static int copy_pairs_between(LPCNetBatch *from, const int *src, LPCNetBatch *to, const int *dst, int m)
{
    int first[LPCN_MAX_SHARDS * LPCN_MAX_SHARDS + 1] = {0}, fill[LPCN_MAX_SHARDS * LPCN_MAX_SHARDS], ls = 0, ld = 0, rc = 0;
    const int K = to->n_shards, keys = from->n_shards * K;
    int *psrc = (int *)malloc(2 * (size_t)(m + 1) * sizeof(int)), *pdst = psrc ? psrc + m + 1 : NULL;
    if (!psrc) { set_err("copy_streams: out of memory"); return LPCN_E_ARG; }
    for (int i = 0; i < m; i++) first[shard_of(from->at, from->n_shards, src[i], &ls) * K + shard_of(to->at, K, dst[i], &ld) + 1]++;
    for (int k = 0; k < keys; k++) { first[k + 1] += first[k]; fill[k] = first[k]; }
    for (int i = 0; i < m; i++) {
        const int key = shard_of(from->at, from->n_shards, src[i], &ls) * K + shard_of(to->at, K, dst[i], &ld);
        psrc[fill[key]] = ls; pdst[fill[key]++] = ld;
    }
    for (int key = 0; key < keys && !rc; key++)
        if (first[key + 1] > first[key]) rc = lpcn_batch_dev_copy_streams_to(from->sh[key / K].dev, psrc + first[key], to->sh[key % K].dev, pdst + first[key], first[key + 1] - first[key]);
    if (rc) take_engine_err();
    free(psrc);
    return rc;
}
int lpcnet_batch_copy_streams_to(LPCNetBatch *from, const int *src, LPCNetBatch *to, const int *dst, int m)
{
    NEED_MODEL(from);
    NEED_MODEL(to);
    if (from == to || m < 0 || m > to->n || (m && (!src || !dst))) { set_err("lpcnet_batch_copy_streams_to: two batches, and at most as many pairs as the destination has streams"); return LPCN_E_ARG; }
    int lay[LPCN_SNAP_LAYOUT_MAX], need = 0, rc = 0;
    unsigned char *mark = (unsigned char *)calloc((size_t)to->n, 1);
    if (!mark) { set_err("lpcnet_batch_copy_streams_to: out of memory"); return LPCN_E_ARG; }
    for (int i = 0; i < m && !rc; i++) {
        if (src[i] < 0 || src[i] >= from->n || dst[i] < 0 || dst[i] >= to->n || mark[dst[i]]) rc = LPCN_E_ARG; else mark[dst[i]] = 1;
    }
    free(mark);
    if (rc) { set_err("lpcnet_batch_copy_streams_to: every index must lie inside its batch and all destinations be distinct"); return rc; }
    if ((rc = batch_layout(from, lay)) < 0) return rc;
    for (int k = 0; k < to->n_shards && rc >= 0; k++) {  /* (every destination shard is asked before anything changes) */
        rc = lpcn_batch_dev_snapshot_match(to->sh[k].dev, lay, 0);
        if (rc > 0) need = 1;
    }
    if (rc < 0) { take_engine_err(); return rc; }
    for (int k = 0; need && k < to->n_shards; k++)
        if ((rc = lpcn_batch_dev_snapshot_enable(to->sh[k].dev, lay))) { take_engine_err(); return rc; }
    return copy_pairs_between(from, src, to, dst, m);
}

int lpcnet_batch_set_streams_per_workgroup(LPCNetBatch *b, int spw) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_set_streams_per_wg(s->dev, spw)); }
int lpcnet_batch_tune(LPCNetBatch *b) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_tune(s->dev)); }
int lpcnet_batch_set_twelve_waves(LPCNetBatch *b, int mode) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_set_x3(s->dev, mode)); }
/* (every shard holds the same model: a refusal comes from the first shard, before anything has changed) */
int lpcnet_batch_set_two_group_streaming(LPCNetBatch *b, int on) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_set_x2_streamed(s->dev, on)); }
int lpcnet_batch_get_two_group_streaming(const LPCNetBatch *b) { return b && b->n_shards && b->sh[0].dev ? lpcn_batch_dev_x2_streamed(b->sh[0].dev) : 0; }
int lpcnet_batch_set_fast_two_group(LPCNetBatch *b, int on) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_set_x2_fast(s->dev, on)); }
int lpcnet_batch_get_fast_two_group(const LPCNetBatch *b) { return b && b->n_shards && b->sh[0].dev ? lpcn_batch_dev_x2_fast(b->sh[0].dev) : 0; }
int lpcnet_batch_set_group_schedule(LPCNetBatch *b, int form, int lanes)
{
    NEED_MODEL(b);
    if (form < 0 || form > 1 || lanes < 1 || lanes > 4) { set_err("lpcnet_batch_set_group_schedule: form must be 0 or 1 and lanes 1 .. 4"); return LPCN_E_ARG; }      /* (no shard changes) */
    EACH_SHARD(lpcn_batch_dev_set_group_schedule(s->dev, form, lanes));
}
int lpcnet_batch_get_group_schedule(const LPCNetBatch *b, int *form, int *lanes)
{
    NEED_MODEL(b);
    FWD(lpcn_batch_dev_get_group_schedule(b->sh[0].dev, form, lanes));
}
int lpcnet_batch_group_form(const LPCNetBatch *b, int cnt)
{
    NEED_MODEL(b);
    const int rc = lpcn_batch_dev_group_form(b->sh[0].dev, cnt);
    if (rc < 0) take_engine_err();
    return rc;
}
int lpcnet_batch_last_groups(const LPCNetBatch *b, int *rec, int cap)
{
    NEED_MODEL(b);
    if (cap < 0 || (cap && !rec)) { set_err("lpcnet_batch_last_groups: bad arguments"); return LPCN_E_ARG; }
    return lpcn_batch_dev_last_groups(b->sh[0].dev, rec, cap);
}
int lpcnet_batch_get_twelve_waves(const LPCNetBatch *b) { return b && b->n_shards && b->sh[0].dev ? lpcn_batch_dev_x3(b->sh[0].dev) : 0; }
int lpcnet_batch_get_streams_per_workgroup(const LPCNetBatch *b) { return b && b->n_shards && b->sh[0].dev ? lpcn_batch_dev_streams_per_wg(b->sh[0].dev) : 0; }
int lpcnet_batch_enable_timing(LPCNetBatch *b, int on) { NEED_MODEL(b); EACH_SHARD(lpcn_batch_dev_enable_timing(s->dev, on)); }
/* kernel milliseconds of the most recent run: the slowest shard */
int lpcnet_batch_last_timing(LPCNetBatch *b, float *ms_s, float *ms_f)
{
    NEED_MODEL(b);
    float bs = 0.f, bf = 0.f;
    for (int k = 0; k < b->n_shards; k++) {
        float a = 0.f, c = 0.f;
        lpcn_batch_dev_last_timing(b->sh[k].dev, &a, &c);
        if (a > bs) bs = a;
        if (c > bf) bf = c;
    }
    if (ms_s) *ms_s = bs;
    if (ms_f) *ms_f = bf;
    return 0;
}

int lpcnet_batch_run_tail(LPCNetBatch *b, const float *cond_a, const float *cond_b, const float *lpc, short *pcm, int n_frames, int preload)
{
    NEED_MODEL(b);
    const size_t per = (size_t)n_frames;                /* (per stream: frames) */
    EACH_SHARD(lpcn_batch_dev_run_tail_host(s->dev, cond_a + at.first * per * LPCN_ROWS_A, cond_b + at.first * per * LPCN_ROWS_B, lpc + at.first * per * LPCN_LPC_ORDER,
                                            pcm + at.first * per * LPCN_FRAME_SIZE, n_frames, preload));
}

int lpcnet_batch_run_frames(LPCNetBatch *b, const float *features, int feat_stride, float *cond_a, float *cond_b, float *lpc, int n_frames)
{
    NEED_MODEL(b);
    const size_t per = (size_t)n_frames;                /* (per stream: frames) */
    EACH_SHARD(lpcn_batch_dev_run_frames_host(s->dev, features + at.first * per * feat_stride, feat_stride, cond_a ? cond_a + at.first * per * LPCN_ROWS_A : NULL,
                                              cond_b ? cond_b + at.first * per * LPCN_ROWS_B : NULL, lpc ? lpc + at.first * per * LPCN_LPC_ORDER : NULL, n_frames));
}

/* the unpacker alone: packets [n][n_packets][8] -> features [n][4 n_packets][20]; only the decoder's VQ memory advances */
int lpcnet_batch_run_decode(LPCNetBatch *b, const unsigned char *packets, float *features, int n_packets)
{
    NEED_MODEL(b);
    if (n_packets <= 0 || !packets || !features) { set_err("lpcnet_batch_run_decode: bad arguments"); return LPCN_E_ARG; }
    const int rc = batch_codebooks(b);
    if (rc) return rc;
    const size_t per = (size_t)n_packets;               /* (per stream: packets) */
    EACH_SHARD(lpcn_batch_dev_run_decode_host(s->dev, packets + at.first * per * 8, features + at.first * per * 4 * LPCN_NB_FEAT, n_packets));
}

int lpcnet_batch_state_size(void) { return (int)sizeof(lpcn_stream_state); }
int lpcnet_batch_get_raw_state(LPCNetBatch *b, int stream, void *out)
{
    NEED_MODEL(b);
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_get_state(s->dev, i, (lpcn_stream_state *)out));
}
int lpcnet_batch_set_raw_state(LPCNetBatch *b, int stream, const void *in)
{
    NEED_MODEL(b);
    SHARD_OF(s, i, b, stream);
    FWD(lpcn_batch_dev_set_state(s->dev, i, (const lpcn_stream_state *)in));
}
int lpcnet_batch_debug_trace(LPCNetBatch *b, int n_samples, float *host_out) { NEED_MODEL(b); FWD(lpcn_batch_dev_debug_trace(b->sh[0].dev, n_samples, host_out)); }
int lpcnet_batch_profile(LPCNetBatch *b, unsigned long long *out) { NEED_MODEL(b); FWD(lpcn_batch_dev_profile(b->sh[0].dev, out)); }
