/* The roster of a batch whose streams come and go: which pair lists lpcnet_batch_copy_streams accepts, how a list splits over the shards, and
 * the swap-remove plan that keeps every shard's active streams a prefix when streams leave.  Plain C with no engine or HIP include, like
 * api_shards.h (tests/tools/roster_host.c drives this header alone).  `mark` is the caller's scratch of one byte per stream of the batch. */
#pragma once
#include <string.h>
#include "api_shards.h"

static inline int roster_streams(const shard_span *sp, int n_shards) { return n_shards > 0 ? sp[n_shards - 1].first + sp[n_shards - 1].count : 0; }

/* A pair list src[i] -> dst[i], i < m: every index inside the batch, all destinations distinct, no stream both a source and a destination (a
 * source may feed several destinations).  0, or -1 - i with i the first bad pair. */
static inline int roster_check(const shard_span *sp, int n_shards, const int *src, const int *dst, int m, unsigned char *mark)
{
    const int n = roster_streams(sp, n_shards);
    if (m < 0 || (m && (!src || !dst))) return -1;
    memset(mark, 0, (size_t)n);
    for (int i = 0; i < m; i++) {
        if (src[i] < 0 || src[i] >= n || dst[i] < 0 || dst[i] >= n) return -1 - i;
        if (mark[src[i]] == 2 || mark[dst[i]] != 0 || src[i] == dst[i]) return -1 - i;
        mark[src[i]] = 1; mark[dst[i]] = 2;
    }
    return 0;
}

/* The split of a valid list: the pairs inside shard k, in the shard's own indices, at lsrc / ldst [first[k], first[k + 1]) (first has
 * n_shards + 1 entries), and the pairs across shards, in the batch's indices, at xsrc / xdst.  Every output array holds m entries.  Returns the
 * number of cross-shard pairs. */
static inline int roster_split(const shard_span *sp, int n_shards, const int *src, const int *dst, int m, int *first, int *lsrc, int *ldst, int *xsrc, int *xdst)
{
    int fill[LPCN_MAX_SHARDS], nx = 0, ls = 0, ld = 0;
    for (int k = 0; k <= n_shards; k++) first[k] = 0;
    for (int i = 0; i < m; i++) {
        const int ks = shard_of(sp, n_shards, src[i], &ls), kd = shard_of(sp, n_shards, dst[i], &ld);
        if (ks == kd) first[ks + 1]++;
    }
    for (int k = 0; k < n_shards; k++) { first[k + 1] += first[k]; fill[k] = first[k]; }
    for (int i = 0; i < m; i++) {
        const int ks = shard_of(sp, n_shards, src[i], &ls), kd = shard_of(sp, n_shards, dst[i], &ld);
        if (ks == kd) { lsrc[fill[ks]] = ls; ldst[fill[ks]++] = ld; }
        else { xsrc[nx] = src[i]; xdst[nx++] = dst[i]; }
    }
    return nx;
}

/* Swap-remove: shard k's active streams are [first_k, first_k + active[k]); the m streams of `leaving` (distinct, all active) go.  Every shard's
 * survivors must end up as the prefix of new_active[k] = active[k] - (its leaving streams) streams: a leaving stream below the new count is a hole
 * and takes the record of a survivor at or above it -- the lowest hole the lowest such survivor -- and a leaving stream that is already in the
 * tail costs nothing, so the plan has the fewest copies there can be.  Pairs go to src / dst (the batch's indices, room for m) and form a valid
 * list for roster_check.  Returns their number, or -1 - i with i the first bad entry of `leaving` (-1 also for bad counts). */
static inline int roster_plan_leave(const shard_span *sp, int n_shards, const int *active, const int *leaving, int m, int *src, int *dst, int *new_active,
                                    unsigned char *mark)
{
    const int n = roster_streams(sp, n_shards);
    int pairs = 0, local;
    if (m < 0 || (m && !leaving)) return -1;
    for (int k = 0; k < n_shards; k++) { if (active[k] < 0 || active[k] > sp[k].count) return -1; new_active[k] = active[k]; }
    memset(mark, 0, (size_t)n);
    for (int i = 0; i < m; i++) {
        const int k = (leaving[i] >= 0 && leaving[i] < n) ? shard_of(sp, n_shards, leaving[i], &local) : -1;
        if (k < 0 || local >= active[k] || mark[leaving[i]]) return -1 - i;
        mark[leaving[i]] = 1;
        new_active[k]--;
    }
    for (int k = 0; k < n_shards; k++) {
        const int f = sp[k].first;
        int mover = f + new_active[k];                       /* the next candidate survivor of the tail */
        for (int hole = f; hole < f + new_active[k]; hole++) {
            if (!mark[hole]) continue;
            while (mark[mover]) mover++;                     /* (as many survivors in the tail as holes in the prefix: it stays below f + active[k]) */
            src[pairs] = mover++; dst[pairs++] = hole;
        }
    }
    return pairs;
}
