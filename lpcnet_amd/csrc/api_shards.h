/* Shards of a batch: which streams each one owns, and the fan-out of one call over all of them.  Plain C with no engine or HIP
 * include: the per-shard work is the caller's function (tests/tools/shard_fanout_host.c drives this header alone). */
#pragma once
#include <pthread.h>
#include <stdio.h>

#define LPCN_MAX_SHARDS 16
#define SHARD_ERR_LEN 512

typedef struct { int first, count; } shard_span;      /* streams [first, first + count) of the batch */

/* Contiguous block partition of n streams over K devices (lpcnet_amd/shard.py: partition): shard k gets n / K streams, the first
 * n % K shards one more.  Empty shards (more devices than streams) are dropped; they are the last ones, so shard k stays on
 * device k.  Returns the number of shards written to sp[]. */
static inline int shard_partition(int n, int K, shard_span *sp)
{
    const int base = n / K, extra = n % K;
    int n_shards = 0;
    for (int k = 0; k < K; k++) {
        const int count = base + (k < extra ? 1 : 0);
        if (count == 0) continue;
        sp[n_shards].first = k * base + (k < extra ? k : extra);
        sp[n_shards++].count = count;
    }
    return n_shards;
}

/* the shard that owns `stream` (-1: none) and the stream's index within it */
static inline int shard_of(const shard_span *sp, int n_shards, int stream, int *local)
{
    for (int k = 0; k < n_shards; k++)
        if (stream >= sp[k].first && stream < sp[k].first + sp[k].count) { *local = stream - sp[k].first; return k; }
    return -1;
}

/* Iterator over the shards that hold some of the streams [first, first + count): start with *k = -1; returns 1 with *k = the
 * next such shard and its part of the range in the shard's own indices, 0 when there is none left. */
static inline int shard_next_in(const shard_span *sp, int n_shards, int first, int count, int *k, int *lfirst, int *lcount)
{
    for (++*k; *k < n_shards; ++*k) {
        const int end = sp[*k].first + sp[*k].count;
        const int lo = first > sp[*k].first ? first : sp[*k].first, hi = first + count < end ? first + count : end;
        if (hi > lo) { *lfirst = lo - sp[*k].first; *lcount = hi - lo; return 1; }
    }
    return 0;
}

typedef int (*shard_fn)(void *ctx, int shard);        /* one shard's part of a call: 0, a negative code, or a positive note */
typedef const char *(*shard_msg_fn)(void);            /* the message of a shard_fn that failed, asked for on the thread that ran it */

typedef struct { shard_fn fn; shard_msg_fn msg; void *ctx; int shard, rc; char err[SHARD_ERR_LEN]; } shard_call;

static inline void *shard_call_run(void *arg)
{
    shard_call *c = (shard_call *)arg;
    c->rc = c->fn(c->ctx, c->shard);
    if (c->rc) snprintf(c->err, sizeof(c->err), "%s", c->msg());
    return NULL;
}

/* fn on every shard.  threaded = 0: shard after shard on the calling thread, stopping at the first one that does not return 0.
 * threaded = 1: all shards at once, one thread each -- shard 0, and a shard whose thread cannot be created, on the caller.
 * Returns 0, else the first negative rc in shard order, else the first positive one, with that shard's message in
 * err[SHARD_ERR_LEN]. */
static inline int shards_run(int n_shards, int threaded, shard_fn fn, shard_msg_fn msg, void *ctx, char *err)
{
    shard_call c[LPCN_MAX_SHARDS];
    pthread_t th[LPCN_MAX_SHARDS];
    int started[LPCN_MAX_SHARDS] = {0};
    if (n_shards < 1) return 0;
    for (int k = 0; k < n_shards; k++) { c[k].fn = fn; c[k].msg = msg; c[k].ctx = ctx; c[k].shard = k; c[k].rc = 0; c[k].err[0] = 0; }
    if (threaded) {
        for (int k = 1; k < n_shards; k++) started[k] = pthread_create(&th[k], NULL, shard_call_run, &c[k]) == 0;
        shard_call_run(&c[0]);
        for (int k = 1; k < n_shards; k++) { if (started[k]) pthread_join(th[k], NULL); else shard_call_run(&c[k]); }
    } else {
        for (int k = 0; k < n_shards; k++) { shard_call_run(&c[k]); if (c[k].rc) break; }
    }
    int bad = -1;
    for (int k = 0; bad < 0 && k < n_shards; k++) if (c[k].rc < 0) bad = k;
    for (int k = 0; bad < 0 && k < n_shards; k++) if (c[k].rc) bad = k;
    if (bad < 0) return 0;
    snprintf(err, SHARD_ERR_LEN, "%s", c[bad].err);
    return c[bad].rc;
}
