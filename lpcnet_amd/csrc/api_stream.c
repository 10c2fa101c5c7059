/* C host shell of the LPCNet HIP engine: the public entry points of include/lpcnet.h on top of the
 * device runtime declared in lpcnet_engine.h.
 *
 * Single-stream API ownership model (SURVEY.md §7 hard part 7): the reference lets callers
 * allocate LPCNetState themselves (lpcnet_get_size + lpcnet_init, no de-init hook) and copy it
 * by value (PLC snapshot / rollback, src/lpcnet_plc.c:216-231).  LPCNetState therefore stays a
 * self-contained POD: it carries the complete per-stream state plus an integer handle of the
 * model; device memory belongs to a process-global registry (one engine + one 1-stream device
 * batch per distinct blob, created lazily on the device chosen with lpcnet_hip_set_device()).  The registry
 * remembers the POD state it last downloaded: a lpcnet_synthesize() call whose state still equals that copy
 * (the normal frame-after-frame case) skips the upload; the new state and the PCM come back in one pinned
 * transfer with one synchronisation per frame.
 *
 * A state without an explicitly loaded model uses the process-default model, which mirrors the reference's
 * compiled-in model: lpcnet_hip_set_default_model(), else the file named by $LPCNET_HIP_MODEL, else
 * ./weights_blob.bin (the file name the reference's demo hard-codes, src/lpcnet_demo.c:113).  The same applies
 * to the decoder's VQ codebooks ($LPCNET_HIP_CODEBOOKS, ./ceps_codebooks.bin; api_core.c).
 *
 * This unit: the model registry, the combining dispatcher, every entry point that takes an LPCNetState or an LPCNetDecState.
 */
#include <math.h>
#include "api_internal.h"

/* packet -> 4 feature vectors.  Follows src/lpcnet_dec.c:81-155 and src/common.c:37-65:
 * 7+6+3+2+10+10+10+13+3 bits, MSB first. */
static unsigned get_bits(const unsigned char *buf, int *pos, int n)
{
    unsigned d = 0;
    for (; n > 0; n--, (*pos)++) d = (d << 1) | ((buf[*pos >> 3] >> (7 - (*pos & 7))) & 1u);
    return d;
}

static void band_interp(float *x, const float *left, const float *right, int mode)
{
    for (int i = 0; i < LPCN_NB_BANDS; i++)
        x[i] = mode == 0 ? .5f * (left[i] + right[i]) : (mode == 1 ? left[i] : right[i]);
}

/* (cb: the codebooks, read-locked by codebooks_rdlock() -- another thread may replace them; api_tools.c calls it too) */
int packet_to_features(const float *const *cb, float feat[4][NB_TOTAL_FEATURES], float *vq_mem, const unsigned char *buf)
{
    if (!cb[0]) return -1;
    int pos = 0;
    const int c0_id = (int)get_bits(buf, &pos, 7), main_pitch = (int)get_bits(buf, &pos, 6);
    int modulation = (int)get_bits(buf, &pos, 3);
    const int corr_id = (int)get_bits(buf, &pos, 2);
    const int e0 = (int)get_bits(buf, &pos, 10), e1 = (int)get_bits(buf, &pos, 10), e2 = (int)get_bits(buf, &pos, 10);
    int vq_mid = (int)get_bits(buf, &pos, 13), interp_id = (int)get_bits(buf, &pos, 3);
    int voiced = 1;
    memset(feat, 0, sizeof(float) * 4 * NB_TOTAL_FEATURES);
    modulation -= 4;
    if (modulation == -4) { voiced = 0; modulation = 0; }
    const float frame_corr = voiced ? 0.3875f + .175f * corr_id : 0.0375f + .075f * corr_id;
    for (int sub = 0; sub < 4; sub++) {
        float p = (float)(pow(2.f, main_pitch / 21.) * 32);
        p *= 1.f + modulation / 16.f / 7.f * (2 * sub - 3);
        if (p < 33) p = 33;
        if (p > 255) p = 255;
        feat[sub][LPCN_NB_BANDS] = .02f * (p - 100.f);
        feat[sub][LPCN_NB_BANDS + 1] = frame_corr - .5f;
    }
    feat[3][0] = (c0_id - 64) / 4.f;
    for (int i = 0; i < LPCN_NB_BANDS - 1; i++)
        feat[3][i + 1] = cb[0][e0 * 17 + i] + cb[1][e1 * 17 + i] + cb[2][e2 * 17 + i];
    float sign = 1;
    if (vq_mid >= 4096) { vq_mid -= 4096; sign = -1; }
    for (int i = 0; i < LPCN_NB_BANDS; i++) feat[1][i] = sign * cb[3][vq_mid * LPCN_NB_BANDS + i];
    if ((vq_mid & 3) < 2)       for (int i = 0; i < LPCN_NB_BANDS; i++) feat[1][i] += .5f * (vq_mem[i] + feat[3][i]);
    else if ((vq_mid & 3) == 2) for (int i = 0; i < LPCN_NB_BANDS; i++) feat[1][i] += vq_mem[i];
    else                        for (int i = 0; i < LPCN_NB_BANDS; i++) feat[1][i] += feat[3][i];
    interp_id += (interp_id >= 7);
    band_interp(feat[0], vq_mem, feat[1], interp_id / 3);
    band_interp(feat[2], feat[1], feat[3], interp_id % 3);
    memcpy(vq_mem, feat[3], sizeof(float) * LPCN_NB_BANDS);
    return 0;
}

/* ---- model registry for the single-stream API ------------------------------------------------
 * One slot per distinct weight blob (the registry keeps its own copy: dedupe compares the bytes, and a slot can
 * rebuild its device side at any time).  lpcnet_hip_shutdown() only releases the device resources, so a state bound
 * before the shutdown simply re-creates them at its next call.  Two limits (round 4): at most MAX_RESIDENT slots hold a
 * device side -- materialising one more releases the device side of the least recently used idle slot, whose handle and
 * blob copy stay valid (its states re-create it transparently at their next call, like after a shutdown) -- and MAX_MODELS
 * slots in all (the handle's low byte).  Only when that many DISTINCT blobs are bound does binding another one evict a slot
 * altogether (states are PODs that may be copied or dropped at will, so there is nothing to count references with); a
 * state still holding such a handle stops with a message. */
typedef struct {
    int used;
    unsigned gen;                     /* bumped when the slot is evicted: a state's handle carries the generation it was bound with */
    unsigned long last_use;           /* g_use_clock at the last bind / run (least recently used slot is evicted when the table is full) */
    int pins;                         /* callers between "slot chosen" and "run_lock taken" (g_lock protects it) */
    unsigned char *blob; int len; uint64_t hash;
    lpcn_engine *engine;
    lpcn_batch_dev *dev;              /* 1 stream */
    int device;
    int cache_valid;                  /* `cached` equals the device copy of the stream state */
    lpcn_stream_state cached;
    pthread_mutex_t run_lock;         /* one device round trip at a time per model */
    /* combining dispatcher of lpcnet_synthesize (see comb_synthesize) */
    lpcn_batch_dev *gdev;             /* COMB_MAX streams on the slot's engine, created when two callers first meet */
    pthread_mutex_t q_lock;
    pthread_cond_t q_cv;
    struct comb_req *q_head, *q_tail;
    int q_leader;                     /* a caller is dispatching (on the device or about to) */
    int fail_code, fail_count;        /* sticky: first failed pass on this model (lpcnet_hip_model_status) */
} registry_entry;
#define COMB_MAX 256
/* one waiting call of an entry point */
typedef struct comb_req {
    LPCNetState *st; const float *feat; short *pcm; int N;
    int kind, preload;                /* LPCN_GROUP_FRAME_SAMPLES / _TAIL / _FRAMES (lpcnet_engine.h) */
    int want_products;                /* FRAME_SAMPLES: the frame products must come back (lpcnet_synthesize_impl; a combined pass always returns them) */
    float *ga, *gb, *lpc;             /* the products: in (TAIL), out (FRAMES, FRAME_SAMPLES) */
    int done, rc;
    struct comb_req *next;
    char err[256];                    /* the leader's message for this caller (tl_err is thread-local) */
} comb_req;
#ifndef LPCN_MAX_MODELS
#define LPCN_MAX_MODELS 256           /* slots (the handle's low byte); tests build a library with a handful to reach the eviction paths */
#endif
#ifndef LPCN_MAX_RESIDENT
#define LPCN_MAX_RESIDENT 16          /* slots that hold a device side at the same time */
#endif
#define MAX_MODELS LPCN_MAX_MODELS
#define MAX_RESIDENT LPCN_MAX_RESIDENT
_Static_assert(MAX_MODELS >= 2 && MAX_MODELS <= 256 && MAX_RESIDENT >= 1, "the handle keeps the slot in its low byte");
static registry_entry g_reg[MAX_MODELS];
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;      /* the registry's lock; order: g_lock -> a slot's run_lock */
static int g_device = -1;             /* device of the single-stream API: lpcnet_hip_set_device(), $LPCNET_HIP_DEVICE, else 0 */
static int g_default_model = -1;      /* handle of the process-default model, -1 = not resolved yet */
static unsigned long g_use_clock;
/* A state's model handle: slot in the low byte, the slot's generation above it (a POD state cannot be told that its
 * model went away; a stale handle is detected instead and stops with a message). */
#define HANDLE(slot) ((int)(((g_reg[slot].gen & 0x7FFFFFu) << 8) | (unsigned)(slot)))
static int handle_slot(int h) { const int slot = h & 0xFF; return (h >= 0 && slot < MAX_MODELS && g_reg[slot].used && HANDLE(slot) == h) ? slot : -1; }

static uint64_t fnv1a(const unsigned char *p, int n)
{
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

int single_stream_device(void)
{
    if (g_device >= 0) return g_device;
    const char *e = getenv("LPCNET_HIP_DEVICE");
    return (e && *e) ? atoi(e) : 0;
}

int lpcnet_hip_set_device(int device)
{
    if (device < 0) { set_err("lpcnet_hip_set_device: bad device"); return -1; }
    pthread_mutex_lock(&g_lock);
    g_device = device;
    pthread_mutex_unlock(&g_lock);
    return 0;
}

/* (g_lock and the slot's run_lock held) the slot gives up its device side; handle, blob copy and queue stay */
static void release_device_side(registry_entry *r)
{
    if (r->gdev) { lpcn_batch_dev_destroy(r->gdev); r->gdev = NULL; }
    if (r->dev) { lpcn_batch_dev_destroy(r->dev); lpcn_engine_destroy(r->engine); }
    __atomic_store_n(&r->dev, (lpcn_batch_dev *)NULL, __ATOMIC_SEQ_CST);      /* (acquire_slot looks at it from outside g_lock) */
    r->engine = NULL; r->cache_valid = 0;
}

/* (g_lock held) device side of a slot, created on first use, after lpcnet_hip_shutdown() and after it was released to make
 * room: the number of resident device sides is bounded, the least recently used idle one goes first */
static int registry_materialize(registry_entry *r)
{
    if (r->dev) return 0;
    {
        int resident = 0, victim = -1;
        for (int i = 0; i < MAX_MODELS; i++) if (g_reg[i].used && g_reg[i].dev) resident++;
        while (resident >= MAX_RESIDENT) {
            victim = -1;
            for (int i = 0; i < MAX_MODELS; i++)
                if (g_reg[i].used && g_reg[i].dev && &g_reg[i] != r && __atomic_load_n(&g_reg[i].pins, __ATOMIC_SEQ_CST) == 0 &&
                    (victim < 0 || g_reg[i].last_use < g_reg[victim].last_use)) victim = i;
            if (victim < 0 || pthread_mutex_trylock(&g_reg[victim].run_lock) != 0) break;       /* everything resident is in a call: go over the limit for now */
            release_device_side(&g_reg[victim]);
            pthread_mutex_unlock(&g_reg[victim].run_lock);
            resident--;
        }
    }
    lpcn_model_host m;
    if (lpcn_model_parse(&m, r->blob, r->len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return -1; }
    lpcn_engine *e = NULL;
    lpcn_batch_dev *d = NULL;
    const int device = single_stream_device();
    int rc = lpcn_engine_create(&e, device, &m);
    lpcn_model_release(&m);
    if (rc) { take_engine_err(); return -1; }
    rc = lpcn_batch_dev_create(&d, e, 1, 1);
    if (rc) { take_engine_err(); lpcn_engine_destroy(e); return -1; }
    r->engine = e; r->dev = d; r->device = device; r->cache_valid = 0;
    return 0;
}

/* (g_lock held) handle of this blob's slot, new or existing; -1 on a malformed blob / no device / every slot busy */
static int registry_bind(const unsigned char *blob, int len)
{
    const uint64_t h = fnv1a(blob, len);
    int slot = -1;
    for (int i = 0; i < MAX_MODELS; i++) {
        if (g_reg[i].used && g_reg[i].len == len && g_reg[i].hash == h && memcmp(g_reg[i].blob, blob, (size_t)len) == 0) {
            g_reg[i].last_use = ++g_use_clock;
            return registry_materialize(&g_reg[i]) == 0 ? HANDLE(i) : -1;
        }
        if (!g_reg[i].used && slot < 0) slot = i;
    }
    if (slot < 0) {                                          /* table full: evict the least recently used slot that nobody is running on */
        for (int i = 0; i < MAX_MODELS; i++)
            if (__atomic_load_n(&g_reg[i].pins, __ATOMIC_SEQ_CST) == 0 && i != handle_slot(g_default_model) && (slot < 0 || g_reg[i].last_use < g_reg[slot].last_use) &&
                pthread_mutex_trylock(&g_reg[i].run_lock) == 0) {
                if (slot >= 0) pthread_mutex_unlock(&g_reg[slot].run_lock);
                slot = i;
            }
        if (slot < 0) { set_err("too many distinct models in use at once through lpcnet_load_model"); return -1; }
        registry_entry *v = &g_reg[slot];
        release_device_side(v);
        free(v->blob);
        const unsigned gen = v->gen + 1;
        pthread_mutex_unlock(&v->run_lock);
        pthread_mutex_destroy(&v->run_lock);
        pthread_mutex_destroy(&v->q_lock);
        pthread_cond_destroy(&v->q_cv);
        memset(v, 0, sizeof(*v));
        v->gen = gen;
    }
    registry_entry *r = &g_reg[slot];
    { const unsigned gen = r->gen; memset(r, 0, sizeof(*r)); r->gen = gen; }
    r->blob = (unsigned char *)malloc((size_t)len);
    if (!r->blob) { set_err("out of memory"); return -1; }
    memcpy(r->blob, blob, (size_t)len);
    r->len = len; r->hash = h;
    if (registry_materialize(r) != 0) { free(r->blob); r->blob = NULL; return -1; }
    pthread_mutex_init(&r->run_lock, NULL);
    pthread_mutex_init(&r->q_lock, NULL);
    pthread_cond_init(&r->q_cv, NULL);
    r->used = 1;
    r->last_use = ++g_use_clock;
    return HANDLE(slot);
}

/* Device resources of the single-stream API are released; bound states stay valid and re-create them on demand. */
void lpcnet_hip_shutdown(void)
{
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < MAX_MODELS; i++)
        if (g_reg[i].used && g_reg[i].dev) {
            pthread_mutex_lock(&g_reg[i].run_lock);
            release_device_side(&g_reg[i]);
            pthread_mutex_unlock(&g_reg[i].run_lock);
        }
    pthread_mutex_unlock(&g_lock);
}

int lpcnet_hip_set_default_model(const unsigned char *data, int len)
{
    if (!data || len <= 0) { set_err("lpcnet_hip_set_default_model: bad arguments"); return -1; }
    pthread_mutex_lock(&g_lock);
    const int id = registry_bind(data, len);
    if (id >= 0) g_default_model = id;
    pthread_mutex_unlock(&g_lock);
    return id >= 0 ? 0 : -1;
}

/* (g_lock held) the process-default model: explicit, else $LPCNET_HIP_MODEL, else ./weights_blob.bin */
static int default_model_locked(void)
{
    if (handle_slot(g_default_model) >= 0) return g_default_model;
    g_default_model = -1;
    /* (a failed lookup is not remembered: the file may appear, or the working directory change, before the next call) */
    const char *path = getenv("LPCNET_HIP_MODEL");
    const int from_cwd = !(path && *path);
    long len = 0;
    unsigned char *buf = read_file(from_cwd ? "weights_blob.bin" : path, &len);
    if (!buf) return -1;
    if (len > 0 && len < 0x7FFFFFFF) g_default_model = registry_bind(buf, (int)len);
    free(buf);
    if (g_default_model >= 0 && from_cwd && !getenv("LPCNET_HIP_QUIET"))
        fprintf(stderr, "lpcnet_hip: no model given (lpcnet_load_model / lpcnet_hip_set_default_model / $LPCNET_HIP_MODEL): using ./weights_blob.bin "
                        "from the current directory, like the reference's demo does (src/lpcnet_demo.c:113)\n");
    return g_default_model;
}

/* ---- single-stream API ------------------------------------------------------------------------ */
/* KISS99 seeding from the string "LPCNet" (src/lpcnet.c:176,181; src/kiss99.c:34-57) */
static void seed_rng(uint32_t c[4])
{
    static const unsigned char d[6] = {'L', 'P', 'C', 'N', 'e', 't'};
    c[0] = 362436069u ^ d[0]; c[1] = 521288629u ^ d[1]; c[2] = 123456789u ^ d[2]; c[3] = 380116160u ^ d[3];
    {   /* one generator step (src/kiss99.c:59-81) */
        uint32_t z = 36969u * (c[0] & 0xFFFF) + (c[0] >> 16), w = 18000u * (c[1] & 0xFFFF) + (c[1] >> 16);
        uint32_t j = c[2];
        j ^= j << 13; j ^= j >> 17; j ^= j << 5;
        c[0] = z; c[1] = w; c[2] = j; c[3] = 69069u * c[3] + 1234567u;
    }
    c[0] ^= d[4]; c[1] ^= d[5];
    if (c[0] == 0 || c[0] == 0x9068FFFFu) c[0]++;
    if (c[1] == 0 || c[1] == 0x464FFFFFu) c[1]++;
    if (c[2] == 0) c[2]++;
}

int lpcnet_get_size(void) { return (int)sizeof(LPCNetState); }

void lpcnet_reset(LPCNetState *st)
{
    memset(&st->s, 0, sizeof(*st) - offsetof(LPCNetState, s));      /* everything behind the model handle, src/lpcnet.c:177-179 */
    st->s.last_exc = 128;             /* lin2ulaw(0), src/lpcnet.c:180 */
    seed_rng(st->s.rng);
}

int lpcnet_init(LPCNetState *st)
{
    st->magic = LPCN_MAGIC;
    st->model_id = -1;                /* resolved to the process-default model at first use (the reference binds its compiled-in model here) */
    lpcnet_reset(st);
    return 0;
}

LPCNetState *lpcnet_create(void)
{
    LPCNetState *st = (LPCNetState *)calloc(1, sizeof(*st));
    if (st) lpcnet_init(st);
    return st;
}

void lpcnet_destroy(LPCNetState *st) { free(st); }

int lpcnet_load_model(LPCNetState *st, const unsigned char *data, int len)
{
    if (!st || !data || len <= 0) { set_err("lpcnet_load_model: bad arguments"); return -1; }
    pthread_mutex_lock(&g_lock);
    const int id = registry_bind(data, len);
    pthread_mutex_unlock(&g_lock);
    if (id < 0) return -1;
    st->magic = LPCN_MAGIC;
    st->model_id = id;
    return 0;
}

/* The reference has no public way to give an LPCNetDecState a model other than its compiled-in one
 * (src/lpcnet.c:284-290: lpcnet_decoder_init -> lpcnet_init); this is the explicit form for weight-file users. */
int lpcnet_hip_decoder_load_model(LPCNetDecState *st, const unsigned char *data, int len)
{
    if (!st) { set_err("lpcnet_hip_decoder_load_model: bad arguments"); return -1; }
    return lpcnet_load_model(&st->lpcnet_state, data, len);
}

/* ---- failure of an entry point that returns void in the reference (SURVEY.md §8b "Errors") -------------------------------
 * The reference's lpcnet_synthesize & co. cannot fail; here a device can.  Such a call does NOT abort the process: it
 * zero-fills what it was asked to produce (silence / zero frame products), leaves the caller's state as it was, and records
 * the failure in a sticky per-thread status (lpcnet_hip_status(), message in lpcnet_hip_last_error(), until
 * lpcnet_hip_clear_error()) and a sticky per-model status (lpcnet_hip_model_status()).  Under the combining dispatcher every
 * caller of a failed pass gets its own zero-filled output and its own status.  The first few failures of a process are also
 * written to stderr (LPCNET_HIP_QUIET=1: never); LPCNET_HIP_ABORT_ON_ERROR=1 restores the old stop-with-a-message. */
static __thread unsigned tl_fail_seq;                        /* failures recorded on this thread so far */
static void entry_failed(const char *who, int code, const char *msg)      /* (msg may be tl_err itself) */
{
    tl_fail_seq++;
    char buf[sizeof(tl_err)];
    snprintf(buf, sizeof(buf), "%s: %s", who, msg ? msg : "");
    snprintf(tl_err, sizeof(tl_err), "%s", buf);
    if (!tl_status) tl_status = code;
    /* (the per-model status is recorded by dispatch() while the slot is pinned) */
    static int reported, env_read, env_fatal, env_quiet;     /* the two environment switches are read once (this is the per-frame path of a PLC that lost its device) */
    if (!__atomic_load_n(&env_read, __ATOMIC_ACQUIRE)) {
        const char *ab = getenv("LPCNET_HIP_ABORT_ON_ERROR");
        env_fatal = ab && *ab == '1';
        env_quiet = getenv("LPCNET_HIP_QUIET") != NULL;
        __atomic_store_n(&env_read, 1, __ATOMIC_RELEASE);
    }
    const int fatal = env_fatal;
    if (fatal || (!env_quiet && __atomic_fetch_add(&reported, 1, __ATOMIC_SEQ_CST) < 8))
        fprintf(stderr, "%s%s\n", tl_err, fatal ? "" : " -- output zero-filled, see lpcnet_hip_status()");
    if (fatal) abort();
}
/* the common case: the message is in tl_err, and what the call was asked to produce is one block of memory */
static void void_entry_failed(const char *who, int code, void *zero, size_t zero_bytes)
{
    memset(zero, 0, zero_bytes);
    entry_failed(who, code, tl_err);
}

/* (g_lock held) registry slot of this state's model -- its own handle, else the process-default model -- with a device
 * side; -1 with *code and tl_err set.  `msg` receives the explanation (the engine's message is thread-local too). */
static int resolve_slot_locked(LPCNetState *st, int *code)
{
    int h = (st->magic == LPCN_MAGIC) ? st->model_id : -1;
    if (h >= 0 && handle_slot(h) < 0) {
        snprintf(tl_err, sizeof(tl_err), "the model bound to this state was evicted (more than %d distinct models bound in this process); "
                                         "call lpcnet_load_model again", MAX_MODELS);
        *code = LPCN_E_MODEL;
        return -1;
    }
    if (h < 0) {
        h = default_model_locked();
        if (h >= 0 && st->magic == LPCN_MAGIC) st->model_id = h;
    }
    const int id = handle_slot(h);
    if (id < 0 || registry_materialize(&g_reg[id]) != 0) {
        char why[256];
        snprintf(why, sizeof(why), "%.255s", (id >= 0 && tl_err[0]) ? tl_err : "none found");
        snprintf(tl_err, sizeof(tl_err), "no model bound to this state and no default model (lpcnet_load_model, lpcnet_hip_set_default_model, "
                                         "$LPCNET_HIP_MODEL or ./weights_blob.bin): %s; the HIP engine has no built-in model and no CPU fallback", why);
        *code = id >= 0 ? LPCN_E_HIP : LPCN_E_MODEL;
        return -1;
    }
    return id;
}

/* The registry slot this state runs on, PINNED (neither evicted nor recycled until unpinned) but not locked: resolves the
 * handle / the default model and makes sure the slot has a device side.  Only g_lock is taken.  NULL: *code, tl_err. */
static registry_entry *pin_entry(LPCNetState *st, int *code)
{
    pthread_mutex_lock(&g_lock);
    const int id = resolve_slot_locked(st, code);
    if (id < 0) { pthread_mutex_unlock(&g_lock); return NULL; }
    registry_entry *r = &g_reg[id];
    r->last_use = ++g_use_clock;
    __atomic_add_fetch(&r->pins, 1, __ATOMIC_SEQ_CST);
    pthread_mutex_unlock(&g_lock);
    return r;
}
static void unpin_entry(registry_entry *r) { __atomic_sub_fetch(&r->pins, 1, __ATOMIC_SEQ_CST); }

/* A PINNED slot, locked for one device round trip (unlock with release_entry).  The lock is taken BY SLOT: the caller's
 * queue, model and device side are this slot's whatever the state's handle or the default model have become meanwhile
 * (ADVICE r4).  lpcnet_hip_shutdown() may have released the device side while we waited: it is re-created (lock order
 * g_lock -> run_lock everywhere).  0, or a negative code with tl_err set. */
static int acquire_slot(registry_entry *r)
{
    for (;;) {
        pthread_mutex_lock(&g_lock);
        const int rc = registry_materialize(r);
        pthread_mutex_unlock(&g_lock);
        if (rc) return LPCN_E_HIP;
        pthread_mutex_lock(&r->run_lock);
        if (__atomic_load_n(&r->dev, __ATOMIC_SEQ_CST) != NULL) return 0;
        pthread_mutex_unlock(&r->run_lock);
    }
}
static void release_entry(registry_entry *r) { pthread_mutex_unlock(&r->run_lock); }

/* upload the caller's POD state unless it is the copy the device already holds */
static int push_state(registry_entry *r, const lpcn_stream_state *s)
{
    if (r->cache_valid && memcmp(&r->cached, s, sizeof(*s)) == 0) return 0;
    r->cache_valid = 0;
    return lpcn_batch_dev_set_state(r->dev, 0, s);
}
static int pull_state(registry_entry *r, lpcn_stream_state *s)
{
    int rc = lpcn_batch_dev_get_state(r->dev, 0, s);
    if (!rc) { r->cached = *s; r->cache_valid = 1; }
    return rc;
}

/* sticky status of the model a state is bound to (0, or the code of its first failed pass since the last clear) */
int lpcnet_hip_model_status(const LPCNetState *st, int clear)
{
    if (!st || st->magic != LPCN_MAGIC) return LPCN_E_ARG;
    pthread_mutex_lock(&g_lock);
    const int slot = handle_slot(st->model_id >= 0 ? st->model_id : g_default_model);
    int code = slot < 0 ? LPCN_E_MODEL : __atomic_load_n(&g_reg[slot].fail_code, __ATOMIC_SEQ_CST);
    if (slot >= 0 && clear) __atomic_store_n(&g_reg[slot].fail_code, 0, __ATOMIC_SEQ_CST);
    pthread_mutex_unlock(&g_lock);
    return code;
}

/* ---- the reference's internal entry points (src/lpcnet_private.h:125-132), which src/lpcnet_plc.c links to ---- */

/* src/lpcnet.c:226-233 */
void lpcnet_reset_signal(LPCNetState *st)
{
    st->s.deemph_mem = 0;
    st->s.last_exc = 128;             /* lin2ulaw(0.f) */
    memset(st->s.last_sig, 0, sizeof(st->s.last_sig));
    memset(st->s.gru_a, 0, sizeof(st->s.gru_a));
    memset(st->s.gru_b, 0, sizeof(st->s.gru_b));
}

/* ---- combining dispatcher (round 4: lpcnet_synthesize; round 5: every entry point that touches the device) ---------------------------
 * The reference is re-entrant per state: a server with one thread per stream scales over its cores.  Here every state of a model
 * shares one device, so concurrent callers are COMBINED instead of serialised: a call queues itself on its model's slot; if no pass
 * is being dispatched it becomes the leader, takes every queued call of its own shape -- same entry point, N and preload -- up to
 * COMB_MAX, and runs them as ONE multi-stream pass (each caller's POD state up, kernels, states and results down, one
 * synchronisation); calls that arrive meanwhile queue up and form the next pass, led by one of them -- group commit, no timer: a lone
 * caller never waits for company, and under load a pass carries as many streams as arrived during the previous one.  Results are
 * bit-identical to running the calls one by one (streams are independent).  The PLC-facing entry points (run_frame_network,
 * lpcnet_synthesize_impl, lpcnet_synthesize_tail_impl: src/lpcnet_private.h:125-132, what a threaded PLC server calls through
 * src/lpcnet_plc.c:216-239,378-421) go through the same queue as lpcnet_synthesize. */

/* (run_lock held) the 100 Hz network for one state, serially; nothing is written unless it succeeded */
static int frame_network_locked(registry_entry *r, LPCNetState *st, float *gru_a_condition, float *gru_b_condition, float *lpc, const float *features)
{
    float lpc_new[LPCN_LPC_ORDER];      /* `lpc` may point into st->s, which the state download overwrites */
    float ga[LPCN_ROWS_A], gb[LPCN_ROWS_B];
    lpcn_stream_state snew;
    int rc = push_state(r, &st->s);
    r->cache_valid = 0;
    if (!rc) rc = lpcn_batch_dev_run_frames_host(r->dev, features, NB_FEATURES, ga, gb, lpc_new, 1);
    if (!rc) rc = pull_state(r, &snew);
    if (rc) { r->cache_valid = 0; return rc; }
    st->s = snew;
    memcpy(gru_a_condition, ga, sizeof(ga));
    memcpy(gru_b_condition, gb, sizeof(gb));
    memcpy(lpc, lpc_new, sizeof(lpc_new));
    return 0;
}

/* (run_lock held) N samples (any N: consecutive pieces of <= 160) from the products held in the state, serially */
static int tail_locked(registry_entry *r, LPCNetState *st, short *output, int N, int preload)
{
    lpcn_stream_state snew;
    int rc = push_state(r, &st->s);
    r->cache_valid = 0;
    short one[LPCN_FRAME_SIZE];                              /* (the caller's buffer is written only when every piece has succeeded; N <= 160 -- every caller in
                                                              * the reference -- needs no heap) */
    short *tmp = N <= LPCN_FRAME_SIZE ? one : (short *)malloc(sizeof(short) * (size_t)N);
    if (!tmp) { set_err("out of memory"); return LPCN_E_HIP; }
    for (int done = 0; !rc && done < N; done += LPCN_FRAME_SIZE) {
        const int n = N - done < LPCN_FRAME_SIZE ? N - done : LPCN_FRAME_SIZE;
        const int pre = preload - done < 0 ? 0 : (preload - done > n ? n : preload - done);
        short frame[LPCN_FRAME_SIZE] = {0};
        memcpy(frame, output + done, sizeof(short) * (size_t)pre);
        rc = lpcn_batch_dev_set_frame_len(r->dev, n);
        if (!rc) rc = lpcn_batch_dev_run_tail_host(r->dev, st->gru_a_condition, st->gru_b_condition, st->s.lpc, frame, 1, pre);
        /* live frames return the imposed samples unchanged; start-up frames are cleared entirely (src/lpcnet.c:239-243) */
        if (!rc) memcpy(tmp + done, frame, sizeof(short) * (size_t)n);
    }
    if (!rc) rc = pull_state(r, &snew);
    if (rc) { r->cache_valid = 0; if (tmp != one) free(tmp); return rc; }
    st->s = snew;
    memcpy(output, tmp, sizeof(short) * (size_t)N);
    if (tmp != one) free(tmp);
    return 0;
}

/* One device pass for `k` queued calls of one shape on one model (run_lock held by the caller through acquire_slot). */
static int comb_run(registry_entry *r, comb_req **grp, int k)
{
    comb_req *q = grp[0];
    if (k == 1) {                                            /* nobody to share with */
        if (q->kind == LPCN_GROUP_FRAME_SAMPLES && q->preload == 0 && !q->want_products) {
            /* lpcnet_synthesize alone: the single-stream fast path (state upload skipped when the device copy is current) */
            const int fresh = !(r->cache_valid && memcmp(&r->cached, &q->st->s, sizeof(q->st->s)) == 0);
            r->cache_valid = 0;
            lpcn_stream_state snew;
            int rc = lpcn_batch_dev_set_frame_len(r->dev, q->N);
            if (!rc) rc = lpcn_batch_dev_run_single(r->dev, fresh ? &q->st->s : NULL, q->feat, q->pcm, &snew);
            if (!rc) { q->st->s = snew; r->cached = snew; r->cache_valid = 1; }
            return rc;
        }
        if (q->kind == LPCN_GROUP_FRAMES) return frame_network_locked(r, q->st, q->ga, q->gb, q->lpc, q->feat);
        if (q->kind == LPCN_GROUP_TAIL) return tail_locked(r, q->st, q->pcm, q->N, q->preload);
        /* lpcnet_synthesize_impl alone: the reference's two steps (src/lpcnet.c:273-277); atomic for the caller -- the state is put back
         * if the second step fails */
        const LPCNetState keep = *q->st;
        int rc = frame_network_locked(r, q->st, q->ga, q->gb, q->lpc, q->feat);
        if (!rc) rc = tail_locked(r, q->st, q->pcm, q->N, q->preload);
        if (rc) *q->st = keep;
        return rc;
    }
    if (!r->gdev) {
        int rc = lpcn_batch_dev_create(&r->gdev, r->engine, COMB_MAX, 1);
        if (rc) return rc;
    }
    const lpcn_stream_state *sin[COMB_MAX];
    lpcn_stream_state *sout[COMB_MAX];
    const float *ft[COMB_MAX];
    short *pc[COMB_MAX];
    float *ga[COMB_MAX], *gb[COMB_MAX], *lp[COMB_MAX];
    for (int i = 0; i < k; i++) {
        sin[i] = &grp[i]->st->s; sout[i] = &grp[i]->st->s; ft[i] = grp[i]->feat; pc[i] = grp[i]->pcm;
        /* a plain lpcnet_synthesize never refreshes the frame products kept in the state -- not on the lone fast path, and therefore not here either
         * (whether it did used to depend on whether another thread happened to call at the same time) */
        const int takes = grp[i]->kind != LPCN_GROUP_FRAME_SAMPLES || grp[i]->want_products;
        ga[i] = takes ? grp[i]->ga : NULL; gb[i] = takes ? grp[i]->gb : NULL; lp[i] = grp[i]->lpc;
    }
    r->cache_valid = 0;                                      /* (the one-stream batch's device copy is not what these states continue from) */
    return lpcn_batch_dev_run_group(r->gdev, k, q->kind, q->N, q->preload, sin, ft, pc, sout, ga, gb, lp);      /* (writes only after the pass has succeeded) */
}

/* dispatcher statistics (process-wide, relaxed atomics): calls served, device passes that served them, the largest pass */
static unsigned long long g_disp_calls, g_disp_passes, g_disp_max;
int lpcnet_hip_dispatch_stats(unsigned long long *out3, int reset)
{
    if (out3) {
        out3[0] = __atomic_load_n(&g_disp_calls, __ATOMIC_RELAXED);
        out3[1] = __atomic_load_n(&g_disp_passes, __ATOMIC_RELAXED);
        out3[2] = __atomic_load_n(&g_disp_max, __ATOMIC_RELAXED);
    }
    if (reset) {
        __atomic_store_n(&g_disp_calls, 0ull, __ATOMIC_RELAXED);
        __atomic_store_n(&g_disp_passes, 0ull, __ATOMIC_RELAXED);
        __atomic_store_n(&g_disp_max, 0ull, __ATOMIC_RELAXED);
    }
    return 0;
}

/* Queue one call on its model's slot and wait until a pass has served it (possibly leading that pass).  Returns 0 or a negative
 * code (tl_err set); nothing is written to the caller's memory on failure. */
static int dispatch(comb_req *me)
{
    /* the slot of this state's model, pinned while the call is queued (a pinned slot is neither evicted nor recycled) */
    int code = 0;
    registry_entry *r = pin_entry(me->st, &code);            /* (g_lock only: a pass in flight on this model must not keep other callers from queueing) */
    if (!r) return code;
    pthread_mutex_lock(&r->q_lock);
    if (r->q_tail) r->q_tail->next = me; else r->q_head = me;
    r->q_tail = me;
    while (!me->done) {
        if (r->q_leader) { pthread_cond_wait(&r->q_cv, &r->q_lock); continue; }
        /* lead one pass: my own call and everything queued with the same shape */
        r->q_leader = 1;
        comb_req *grp[COMB_MAX];
        int k = 0;
        grp[k++] = me;
        comb_req **pp = &r->q_head, *last = NULL;
        while (*pp) {
            comb_req *q = *pp;
            if (q == me || (q->kind == me->kind && q->N == me->N && q->preload == me->preload && q->N <= LPCN_FRAME_SIZE && k < COMB_MAX && q->st != me->st)) {
                if (q != me) grp[k++] = q;
                *pp = q->next;                               /* unlink */
            } else { last = q; pp = &q->next; }
        }
        r->q_tail = last;
        pthread_mutex_unlock(&r->q_lock);
        __atomic_fetch_add(&g_disp_calls, (unsigned long long)k, __ATOMIC_RELAXED);
        __atomic_fetch_add(&g_disp_passes, 1ull, __ATOMIC_RELAXED);
        {
            unsigned long long mx = __atomic_load_n(&g_disp_max, __ATOMIC_RELAXED);
            while ((unsigned long long)k > mx && !__atomic_compare_exchange_n(&g_disp_max, &mx, (unsigned long long)k, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { }
        }
        int rc = acquire_slot(r);                            /* run_lock of THIS slot; re-creates the device side if it was released meanwhile */
        if (!rc) {
            rc = comb_run(r, grp, k);
            if (rc) { r->cache_valid = 0; take_engine_err(); }
            release_entry(r);
        }
        pthread_mutex_lock(&r->q_lock);
        for (int i = 0; i < k; i++) {
            grp[i]->rc = rc;
            if (rc) snprintf(grp[i]->err, sizeof(grp[i]->err), "%.255s", tl_err);      /* (the message is thread-local: hand every caller its copy) */
            grp[i]->done = 1;
        }
        r->q_leader = 0;
        pthread_cond_broadcast(&r->q_cv);
    }
    pthread_mutex_unlock(&r->q_lock);
    if (me->rc) {                                            /* the model's sticky status, recorded while the slot is still pinned (behind the unpin
                                                              * the slot may already belong to another model) */
        int zero = 0;
        __atomic_compare_exchange_n(&r->fail_code, &zero, me->rc, 0, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
        __atomic_add_fetch(&r->fail_count, 1, __ATOMIC_SEQ_CST);
    }
    unpin_entry(r);
    if (me->rc) snprintf(tl_err, sizeof(tl_err), "%s", me->err);
    return me->rc;
}

/* src/lpcnet.c:82-120: one step of the 100 Hz network; products go to the caller's arrays (zeros on failure) */
void run_frame_network(LPCNetState *st, float *gru_a_condition, float *gru_b_condition, float *lpc, const float *features)
{
    comb_req me = {st, features, NULL, LPCN_FRAME_SIZE, LPCN_GROUP_FRAMES, 0, 0, gru_a_condition, gru_b_condition, lpc, 0, 0, NULL, {0}};
    const int rc = dispatch(&me);
    if (rc) {
        memset(gru_a_condition, 0, sizeof(float) * LPCN_ROWS_A);
        memset(gru_b_condition, 0, sizeof(float) * LPCN_ROWS_B);
        void_entry_failed("run_frame_network", rc, lpc, sizeof(float) * LPCN_LPC_ORDER);
    }
}

/* src/lpcnet.c:122-132: queue a frame (at most kernel_size1 + kernel_size2 - 2 = 4, oldest dropped) */
void run_frame_network_deferred(LPCNetState *st, const float *features)
{
    const int max_buffer_size = MAX_FEATURE_BUFFER_SIZE;
    if (st->feature_buffer_fill == max_buffer_size)
        memmove(st->feature_buffer, &st->feature_buffer[NB_FEATURES], sizeof(float) * (size_t)(max_buffer_size - 1) * NB_FEATURES);
    else
        st->feature_buffer_fill++;
    memcpy(&st->feature_buffer[(st->feature_buffer_fill - 1) * NB_FEATURES], features, sizeof(float) * NB_FEATURES);
}

/* src/lpcnet.c:134-144: run the queued frames, products discarded */
void run_frame_network_flush(LPCNetState *st)
{
    for (int i = 0; i < st->feature_buffer_fill; i++) {
        float lpc[LPCN_LPC_ORDER], ga[LPCN_ROWS_A], gb[LPCN_ROWS_B];
        run_frame_network(st, ga, gb, lpc, &st->feature_buffer[i * NB_FEATURES]);
    }
    st->feature_buffer_fill = 0;
}

/* src/lpcnet.c:235-271: N samples from the products held in the state; the first `preload` samples of
 * `output` are imposed on the synthesis filter (teacher forcing) instead of being written.  Any N: the
 * sample loop does not care where a call ends, so N > 160 runs as consecutive pieces of <= 160 samples (never combined).
 * On failure the samples behind the imposed ones are zero-filled and the state is left as it was. */
void lpcnet_synthesize_tail_impl(LPCNetState *st, short *output, int N, int preload)
{
    if (N <= 0) return;
    if (preload < 0 || preload > N) {
        char why[96];
        snprintf(why, sizeof(why), "preload=%d outside 0..N=%d", preload, N);
        memset(output, 0, sizeof(short) * (size_t)N);
        entry_failed("lpcnet_synthesize_tail_impl", LPCN_E_ARG, why);
        return;
    }
    comb_req me = {st, NULL, output, N, LPCN_GROUP_TAIL, preload, 0, st->gru_a_condition, st->gru_b_condition, st->s.lpc, 0, 0, NULL, {0}};
    const int rc = dispatch(&me);
    if (rc) void_entry_failed("lpcnet_synthesize_tail_impl", rc, output + preload, sizeof(short) * (size_t)(N - preload));
}

/* src/lpcnet.c:273-277: the frame network, then N samples; the frame products stay in the state for a later tail call */
void lpcnet_synthesize_impl(LPCNetState *st, const float *features, short *output, int N, int preload)
{
    if (N > LPCN_FRAME_SIZE || N <= 0 || preload < 0 || preload > N) {      /* the reference's two steps, each with its own checks */
        const LPCNetState keep = *st;                        /* atomic for the caller like the one-pass form: a failed second step puts the state back */
        const unsigned seq0 = tl_fail_seq;
        run_frame_network(st, st->gru_a_condition, st->gru_b_condition, st->s.lpc, features);
        if (N > 0 && tl_fail_seq == seq0) lpcnet_synthesize_tail_impl(st, output, N, preload);
        else if (N > 0) memset(output + (preload > 0 && preload <= N ? preload : 0), 0, sizeof(short) * (size_t)(N - (preload > 0 && preload <= N ? preload : 0)));
        if (tl_fail_seq != seq0) *st = keep;
        return;
    }
    comb_req me = {st, features, output, N, LPCN_GROUP_FRAME_SAMPLES, preload, 1, st->gru_a_condition, st->gru_b_condition, st->s.lpc, 0, 0, NULL, {0}};
    const int rc = dispatch(&me);
    if (rc) void_entry_failed("lpcnet_synthesize_impl", rc, output + preload, sizeof(short) * (size_t)(N - preload));
}

/* src/lpcnet.c:279-281.  N <= 160 (every caller in the reference): one fused device pass -- frame kernels and sample
 * kernel back to back, one synchronisation; bit-identical to lpcnet_synthesize_impl(..., 0) (tests/test_gpu_parity.py).
 * N > 160: the reference runs the frame network once and then N samples; so does the two-step form.
 * One difference a caller of the INTERNAL entry points could observe: a lone lpcnet_synthesize call does not refresh the frame
 * products kept in the state (gru_a_condition / gru_b_condition: 4.8 KB more to download per frame on the single-stream fast path);
 * a lpcnet_synthesize_tail_impl that continues a frame must follow lpcnet_synthesize_impl, as it does in src/lpcnet_plc.c.
 * Returns 0 or a negative code (tl_err set); nothing is written on failure. */
static int synthesize_rc(LPCNetState *st, const float *features, short *output, int N)
{
    comb_req me = {st, features, output, N, LPCN_GROUP_FRAME_SAMPLES, 0, 0, st->gru_a_condition, st->gru_b_condition, st->s.lpc, 0, 0, NULL, {0}};
    return dispatch(&me);
}

void lpcnet_synthesize(LPCNetState *st, const float *features, short *output, int N)
{
    if (N <= 0) return;
    if (N > LPCN_FRAME_SIZE) { lpcnet_synthesize_impl(st, features, output, N, 0); return; }
    const int rc = synthesize_rc(st, features, output, N);
    if (rc) void_entry_failed("lpcnet_synthesize", rc, output, sizeof(short) * (size_t)N);
}

/* ---- decoder ----------------------------------------------------------------------------------- */
int lpcnet_decoder_get_size(void) { return (int)sizeof(LPCNetDecState); }

int lpcnet_decoder_init(LPCNetDecState *st)
{
    memset(st, 0, sizeof(*st));
    lpcnet_init(&st->lpcnet_state);
    return 0;
}

LPCNetDecState *lpcnet_decoder_create(void)
{
    LPCNetDecState *st = (LPCNetDecState *)malloc(sizeof(*st));
    if (st) lpcnet_decoder_init(st);
    return st;
}

void lpcnet_decoder_destroy(LPCNetDecState *st) { free(st); }

/* src/lpcnet.c:310-319.  -1 (the reference always returns 0) when no codebooks are installed or a frame's device pass
 * failed -- the packet's remaining samples are zero-filled in that case. */
int lpcnet_decode(LPCNetDecState *st, const unsigned char *buf, short *pcm)
{
    float feat[4][NB_TOTAL_FEATURES];
    const float *const *cb = codebooks_rdlock(NULL);         /* shared: decoder threads unpack concurrently, the VQ memory is the caller's */
    const int rc = packet_to_features(cb, feat, st->vq_mem, buf);
    codebooks_unlock();
    if (rc != 0) {
        set_err("lpcnet_decode: no VQ codebooks installed (lpcnet_hip_set_codebooks, $LPCNET_HIP_CODEBOOKS or ./ceps_codebooks.bin)");
        return -1;
    }
    for (int k = 0; k < 4; k++) {
        const int rs = synthesize_rc(&st->lpcnet_state, feat[k], &pcm[k * LPCN_FRAME_SIZE], LPCN_FRAME_SIZE);
        if (rs) {
            void_entry_failed("lpcnet_decode", rs, &pcm[k * LPCN_FRAME_SIZE], sizeof(short) * (size_t)(4 - k) * LPCN_FRAME_SIZE);
            return -1;
        }
    }
    return 0;
}
