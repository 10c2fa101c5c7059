/* Host check of lpcnet_amd/csrc/api_shards.h, alone (tests/test_shard_fanout_host.py builds it with the address / undefined-behaviour and the
 * thread sanitizer): the partition against the rule of lpcnet_amd/shard.py restated here, the clipped ranges, the owner lookup, and the runner
 * with a fake per-shard function that records its arguments and returns scripted codes.  Prints "ok <checks>" and returns 0, or says what failed. */
#include <errno.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

/* thread creation can be made to fail for chosen shards: the runner must then do their work on the caller */
static unsigned g_refuse_mask;
static int checked_pthread_create(pthread_t *th, const pthread_attr_t *attr, void *(*fn)(void *), void *arg);
#define pthread_create checked_pthread_create
#include "api_shards.h"
#undef pthread_create
static int checked_pthread_create(pthread_t *th, const pthread_attr_t *attr, void *(*fn)(void *), void *arg)
{
    if (g_refuse_mask >> ((shard_call *)arg)->shard & 1u) return EAGAIN;
    return pthread_create(th, attr, fn, arg);
}

static long g_checks;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

/* lpcnet_amd/shard.py: partition(n_streams, rank, world) and owner(stream, n_streams, world) */
static void py_partition(int n, int rank, int world, int *first, int *count)
{
    const int base = n / world, extra = n % world;
    *count = base + (rank < extra ? 1 : 0);
    *first = rank * base + (rank < extra ? rank : extra);
}
static int py_owner(int stream, int n, int world)
{
    const int base = n / world, extra = n % world, edge = extra * (base + 1);
    if (stream < edge) return stream / (base + 1);
    return extra + (stream - edge) / (base > 1 ? base : 1);
}

static void check_geometry(int n, int K)
{
    shard_span sp[LPCN_MAX_SHARDS];
    const int ns = shard_partition(n, K, sp);
    /* the rule, empty shards dropped */
    int want = 0, next = 0, lo = n, hi = 0;
    for (int r = 0; r < K; r++) {
        int f, c;
        py_partition(n, r, K, &f, &c);
        if (c == 0) continue;
        CHECK(want < ns && sp[want].first == f && sp[want].count == c, "n=%d K=%d rank %d: (%d, %d)", n, K, r, f, c);
        want++;
    }
    CHECK(ns == want && ns == (n < K ? n : K), "n=%d K=%d: %d shards", n, K, ns);
    for (int k = 0; k < ns; k++) {                            /* contiguous, nothing empty, sizes differ by at most one */
        CHECK(sp[k].first == next && sp[k].count > 0, "n=%d K=%d shard %d", n, K, k);
        next += sp[k].count;
        if (sp[k].count < lo) lo = sp[k].count;
        if (sp[k].count > hi) hi = sp[k].count;
    }
    CHECK(next == n && hi - lo <= 1, "n=%d K=%d: covers %d, sizes %d..%d", n, K, next, lo, hi);
    /* the owner of every stream, and of the two just outside */
    for (int s = -1; s <= n; s++) {
        int local = -7;
        const int k = shard_of(sp, ns, s, &local);
        if (s < 0 || s >= n) { CHECK(k == -1, "n=%d K=%d stream %d: owner %d", n, K, s, k); continue; }
        CHECK(k == py_owner(s, n, K) && k >= 0 && k < ns && s >= sp[k].first && s < sp[k].first + sp[k].count && local == s - sp[k].first,
              "n=%d K=%d stream %d: owner %d local %d", n, K, s, k, local);
    }
    if (n > 12) return;
    /* every range: the local pieces cover exactly the requested streams, once each, in shard order */
    for (int first = 0; first <= n; first++)
        for (int count = 0; first + count <= n; count++) {
            int seen[12] = {0}, last = -1, lf = -7, lc = -7;
            for (int k = -1; shard_next_in(sp, ns, first, count, &k, &lf, &lc); ) {
                CHECK(k > last && k < ns && lc > 0 && lf >= 0 && lf + lc <= sp[k].count, "n=%d K=%d [%d,+%d): shard %d local (%d, %d)", n, K, first, count, k, lf, lc);
                CHECK(lf == (first > sp[k].first ? first - sp[k].first : 0), "n=%d K=%d [%d,+%d): shard %d starts at %d", n, K, first, count, k, lf);
                for (int i = 0; i < lc; i++) seen[sp[k].first + lf + i]++;
                last = k;
            }
            for (int s = 0; s < n; s++) CHECK(seen[s] == (s >= first && s < first + count), "n=%d K=%d [%d,+%d): stream %d seen %d times", n, K, first, count, s, seen[s]);
        }
}

/* the fake per-shard function: each shard writes its own record only */
typedef struct { int rc[LPCN_MAX_SHARDS], calls[LPCN_MAX_SHARDS], on_caller[LPCN_MAX_SHARDS]; pthread_t caller; void *self; } script;
static __thread char tl_msg[64];
static const char *fake_msg(void) { return tl_msg; }
static int fake_shard(void *ctx, int k)
{
    script *sc = (script *)ctx;
    sc->calls[k] += sc->self == ctx ? 1 : 100;
    sc->on_caller[k] = pthread_equal(pthread_self(), sc->caller);
    snprintf(tl_msg, sizeof(tl_msg), "shard %d says %d", k, sc->rc[k]);
    return sc->rc[k];
}

static void check_run(int ns, const int *rc, unsigned refuse)
{
    for (int threaded = 0; threaded < 2; threaded++) {
        script sc;
        memset(&sc, 0, sizeof(sc));
        memcpy(sc.rc, rc, sizeof(int) * (size_t)ns);
        sc.caller = pthread_self(); sc.self = &sc;
        char err[SHARD_ERR_LEN] = "untouched";
        g_refuse_mask = refuse;
        const int got = shards_run(ns, threaded, fake_shard, fake_msg, &sc, err);
        g_refuse_mask = 0;
        int stop = ns, win = -1;                              /* in turn: the first failure ends the walk; threaded: first negative, then first positive */
        for (int k = ns - 1; k >= 0; k--) if (rc[k]) stop = k;
        for (int k = 0; win < 0 && k < ns; k++) if (rc[k] < 0) win = k;
        for (int k = 0; win < 0 && k < ns; k++) if (rc[k]) win = k;
        if (!threaded) win = stop < ns ? stop : -1;
        for (int k = 0; k < ns; k++) {
            CHECK(sc.calls[k] == (threaded || k <= stop), "%d shards, threaded %d: shard %d called %d times", ns, threaded, k, sc.calls[k]);
            if (sc.calls[k] && (!threaded || k == 0 || (refuse >> k & 1u))) CHECK(sc.on_caller[k], "%d shards, threaded %d: shard %d left the calling thread", ns, threaded, k);
            if (threaded && k > 0 && !(refuse >> k & 1u)) CHECK(!sc.on_caller[k], "%d shards: shard %d has no thread of its own", ns, k);
        }
        char want[64];
        snprintf(want, sizeof(want), "shard %d says %d", win, win < 0 ? 0 : rc[win]);
        CHECK(got == (win < 0 ? 0 : rc[win]), "%d shards, threaded %d: rc %d, shard %d should win", ns, threaded, got, win);
        CHECK(strcmp(err, win < 0 ? "untouched" : want) == 0, "%d shards, threaded %d: message '%s'", ns, threaded, err);
    }
}

int main(void)
{
    for (int n = 1; n <= 40; n++)
        for (int K = 1; K <= LPCN_MAX_SHARDS; K++) check_geometry(n, K);
    /* every script of {0, two negative codes, the FEC feed's 1, another note} on up to four shards ... */
    static const int codes[5] = {0, -3, -7, 1, 2};
    for (int ns = 1; ns <= 4; ns++) {
        int total = 1;
        for (int k = 0; k < ns; k++) total *= 5;
        for (int c = 0; c < total; c++) {
            int rc[4];
            for (int k = 0, d = c; k < ns; k++, d /= 5) rc[k] = codes[d % 5];
            check_run(ns, rc, 0);
        }
    }
    /* ... and at every shard count: all well, one failure at each place, a note in front of a failure, threads that cannot be created */
    for (int ns = 1; ns <= LPCN_MAX_SHARDS; ns++) {
        int rc[LPCN_MAX_SHARDS] = {0};
        check_run(ns, rc, 0);
        check_run(ns, rc, 0xAAAAu);
        for (int bad = 0; bad < ns; bad++) {
            memset(rc, 0, sizeof(rc));
            rc[bad] = -2 - bad;
            check_run(ns, rc, 0);
            check_run(ns, rc, 1u << bad);
            rc[0] = bad ? 1 : rc[0];
            rc[ns - 1] = rc[ns - 1] ? rc[ns - 1] : -99;
            check_run(ns, rc, 0xFFFEu);
        }
    }
    CHECK(shards_run(0, 1, fake_shard, fake_msg, NULL, NULL) == 0, "no shards");
    printf("ok %ld\n", g_checks);
    return 0;
}
