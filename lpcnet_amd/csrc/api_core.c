/* C host shell of the LPCNet HIP engine, the part every other unit of the shell leans on: the per-thread error message and
 * status, the identity of the sources the library was built from, and the store of the decoder's VQ codebooks (process-wide;
 * the default file: $LPCNET_HIP_CODEBOOKS, else ./ceps_codebooks.bin). */
#include "api_internal.h"

__thread char tl_err[512];
__thread int tl_status;
const char *lpcnet_hip_last_error(void) { return tl_err; }
const char *lpcnet_batch_last_error(void) { return tl_err; }
int lpcnet_hip_status(void) { return tl_status; }
void lpcnet_hip_clear_error(void) { tl_status = 0; tl_err[0] = 0; }

#ifndef LPCN_SOURCE_HASH
#define LPCN_SOURCE_HASH "unknown"
#endif
#ifndef LPCN_DEVICE_SOURCE_HASH
#define LPCN_DEVICE_SOURCE_HASH "unknown"
#endif
/* identity of the sources this library was built from (lpcnet_amd/build.py bakes both in; the marker makes the string
 * findable in the file without loading it): src = every file under csrc/ + include/, dev = the device sources only */
static const char g_build_info[] = "LPCN_BUILD_INFO: src=" LPCN_SOURCE_HASH " dev=" LPCN_DEVICE_SOURCE_HASH;
const char *lpcnet_hip_build_info(void) { return g_build_info + sizeof("LPCN_BUILD_INFO: ") - 1; }

/* ---- VQ codebooks for the codec path (absent generated file ceps_codebooks.c) ---------------- */
static float *g_cb[4];
static int g_cb_version;              /* bumped by every lpcnet_hip_set_codebooks: batches re-upload lazily */
/* The codebooks have a lock of their own, and readers share it: decoder threads unpack their packets concurrently (the
 * per-stream VQ memory lives in the caller's LPCNetDecState) and never meet the registry lock; only
 * lpcnet_hip_set_codebooks() -- and the one-time lookup of the default file -- excludes them. */
static pthread_rwlock_t g_cb_lock = PTHREAD_RWLOCK_INITIALIZER;
static int g_cb_default_tried;

static const size_t g_cb_count[4] = {1024 * 17, 1024 * 17, 1024 * 17, 4096 * 18};

static int install_codebooks_locked(const float *const src[4])
{
    float *fresh[4] = {NULL, NULL, NULL, NULL};
    for (int i = 0; i < 4; i++) {
        fresh[i] = (float *)malloc(g_cb_count[i] * sizeof(float));
        if (!fresh[i]) { for (int k = 0; k < i; k++) free(fresh[k]); return -1; }
        memcpy(fresh[i], src[i], g_cb_count[i] * sizeof(float));
    }
    for (int i = 0; i < 4; i++) { free(g_cb[i]); g_cb[i] = fresh[i]; }
    g_cb_version++;
    return 0;
}

void lpcnet_hip_set_codebooks(const float *cb1, const float *cb2, const float *cb3, const float *cbd)
{
    const float *const src[4] = {cb1, cb2, cb3, cbd};
    pthread_rwlock_wrlock(&g_cb_lock);
    if (install_codebooks_locked(src) != 0) set_err("lpcnet_hip_set_codebooks: out of memory");
    pthread_rwlock_unlock(&g_cb_lock);
}

unsigned char *read_file(const char *path, long *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    unsigned char *buf = NULL;
    long n = -1;
    if (fseek(f, 0, SEEK_END) == 0 && (n = ftell(f)) > 0 && fseek(f, 0, SEEK_SET) == 0) {
        buf = (unsigned char *)malloc((size_t)n);
        if (buf && fread(buf, 1, (size_t)n, f) != (size_t)n) { free(buf); buf = NULL; }
    }
    fclose(f);
    *len = n;
    return buf;
}

/* Process-default codebooks (the reference compiles ceps_codebooks.c in): $LPCNET_HIP_CODEBOOKS, else ./ceps_codebooks.bin;
 * raw little-endian float32: ceps_codebook1..3 [1024][17] each, then ceps_codebook_diff4 [4096][18]. */
static void default_codebooks_locked(void)
{
    if (g_cb[0] || g_cb_default_tried) return;
    g_cb_default_tried = 1;
    const char *path = getenv("LPCNET_HIP_CODEBOOKS");
    long len = 0;
    unsigned char *buf = read_file(path && *path ? path : "ceps_codebooks.bin", &len);
    if (!buf) return;
    const size_t want = (g_cb_count[0] + g_cb_count[1] + g_cb_count[2] + g_cb_count[3]) * sizeof(float);
    if ((size_t)len == want) {
        const float *f = (const float *)buf;
        const float *const src[4] = {f, f + g_cb_count[0], f + g_cb_count[0] + g_cb_count[1], f + g_cb_count[0] + g_cb_count[1] + g_cb_count[2]};
        (void)install_codebooks_locked(src);
    }
    free(buf);
}

/* the codebooks, read-locked (shared); the default file is looked for once, under the write lock */
const float *const *codebooks_rdlock(int *version)
{
    pthread_rwlock_rdlock(&g_cb_lock);
    if (!g_cb[0] && !g_cb_default_tried) {
        pthread_rwlock_unlock(&g_cb_lock);
        pthread_rwlock_wrlock(&g_cb_lock);
        default_codebooks_locked();
        pthread_rwlock_unlock(&g_cb_lock);
        pthread_rwlock_rdlock(&g_cb_lock);
    }
    if (version) *version = g_cb_version;
    return (const float *const *)g_cb;
}
void codebooks_unlock(void) { pthread_rwlock_unlock(&g_cb_lock); }
