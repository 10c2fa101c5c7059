/* Drives lpcnet_amd/csrc/api_roster.h alone (no engine, no HIP): the pair-list check, its split over the shards and the swap-remove planner, for
 * 1..40 streams on 1..8 shards and every set of up to 4 leaving streams.  Prints "ok <checks>" or the first failure (tests/test_roster_host.py). */
#include <stdio.h>
#include <stdlib.h>
#include "api_roster.h"

#define MAXN 40
static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { printf("FAIL %s:%d: %s (n %d, K %d)\n", __FILE__, __LINE__, #c, g_n, g_K); exit(1); } } while (0)
static int g_n, g_K;

static shard_span sp[LPCN_MAX_SHARDS];
static int n_shards, active[LPCN_MAX_SHARDS];

static void one_plan(const int *leaving, int m)
{
    int src[MAXN], dst[MAXN], na[LPCN_MAX_SHARDS], content[MAXN], is_leaving[MAXN] = {0}, local;
    unsigned char mark[MAXN], mark2[MAXN];
    const int pairs = roster_plan_leave(sp, n_shards, active, leaving, m, src, dst, na, mark);
    CHECK(pairs >= 0 && pairs <= m);
    for (int i = 0; i < m; i++) is_leaving[leaving[i]] = 1;
    /* the plan is a list copy_streams accepts, with every pair inside one shard and no leaving stream as a source */
    CHECK(roster_check(sp, n_shards, src, dst, pairs, mark2) == 0);
    for (int i = 0; i < pairs; i++) {
        CHECK(!is_leaving[src[i]] && is_leaving[dst[i]]);
        CHECK(shard_of(sp, n_shards, src[i], &local) == shard_of(sp, n_shards, dst[i], &local));
        for (int j = 0; j < i; j++) CHECK(dst[j] != dst[i] && src[j] != dst[i] && dst[j] != src[i]);
    }
    /* after the copies each shard's survivors are exactly its new prefix, and the copies are as many as the leaving streams inside it */
    for (int s = 0; s < g_n; s++) content[s] = s;
    for (int i = 0; i < pairs; i++) content[dst[i]] = content[src[i]];
    int need = 0;
    for (int k = 0; k < n_shards; k++) {
        int gone = 0, seen[MAXN] = {0};
        for (int s = sp[k].first; s < sp[k].first + active[k]; s++) gone += is_leaving[s];
        CHECK(na[k] == active[k] - gone);
        for (int s = sp[k].first; s < sp[k].first + na[k]; s++) {
            const int c = content[s];
            CHECK(c >= sp[k].first && c < sp[k].first + active[k] && !is_leaving[c] && !seen[c]);
            seen[c] = 1;
            need += is_leaving[s];
        }
    }
    CHECK(pairs == need);
}

static void all_sets(void)
{
    int act[MAXN], na = 0, L[4];
    for (int k = 0; k < n_shards; k++) for (int i = 0; i < active[k]; i++) act[na++] = sp[k].first + i;
    one_plan(L, 0);
    for (int a = 0; a < na; a++) {
        L[0] = act[a]; one_plan(L, 1);
        for (int b = a + 1; b < na; b++) {
            L[1] = act[b]; one_plan(L, 2);
            for (int c = b + 1; c < na; c++) {
                L[2] = act[c]; one_plan(L, 3);
                for (int d = c + 1; d < na; d++) { L[3] = act[d]; one_plan(L, 4); }
            }
        }
    }
    if (na >= 2) { int R[2] = {act[na - 1], act[0]}; one_plan(R, 2); }      /* (any order) */
}

static void refusals(void)
{
    unsigned char mark[MAXN];
    int src[MAXN], dst[MAXN], na[LPCN_MAX_SHARDS], first[LPCN_MAX_SHARDS + 1], ls[4], ld[4], xs[4], xd[4];
    const int n = g_n;
    if (n >= 3) {
        int a[2] = {0, 1}, b[2] = {2, 2};
        CHECK(roster_check(sp, n_shards, a, b, 2, mark) == -2);      /* duplicate destination */
        int c[2] = {0, 1}, d[2] = {1, 2};
        CHECK(roster_check(sp, n_shards, c, d, 2, mark) == -2);      /* stream 1 is a source and a destination */
        int e[2] = {0, 2}, f[2] = {1, 0};
        CHECK(roster_check(sp, n_shards, e, f, 2, mark) == -2);      /* destination 0 was a source */
        int g[2] = {0, 0}, h[2] = {1, 2};
        CHECK(roster_check(sp, n_shards, g, h, 2, mark) == 0);       /* one source, two destinations */
    }
    { int a[1] = {0}, b[1] = {0}; CHECK(roster_check(sp, n_shards, a, b, 1, mark) == -1); }      /* onto itself */
    { int a[1] = {0}, b[1] = {n}; CHECK(roster_check(sp, n_shards, a, b, 1, mark) == -1); }      /* out of range */
    { int a[1] = {-1}, b[1] = {0}; CHECK(roster_check(sp, n_shards, a, b, 1, mark) == -1); }
    CHECK(roster_check(sp, n_shards, NULL, NULL, 1, mark) == -1 && roster_check(sp, n_shards, NULL, NULL, 0, mark) == 0);
    /* the planner refuses a stream that is not active, one that leaves twice, one outside the batch, and bad counts */
    { int l[1] = {n}; CHECK(roster_plan_leave(sp, n_shards, active, l, 1, src, dst, na, mark) == -1); }
    { int l[1] = {-1}; CHECK(roster_plan_leave(sp, n_shards, active, l, 1, src, dst, na, mark) == -1); }
    for (int k = 0; k < n_shards; k++) {
        if (active[k] < sp[k].count) { int l[1] = {sp[k].first + active[k]}; CHECK(roster_plan_leave(sp, n_shards, active, l, 1, src, dst, na, mark) == -1); }
        if (active[k] > 0) { int l[2] = {sp[k].first, sp[k].first}; CHECK(roster_plan_leave(sp, n_shards, active, l, 2, src, dst, na, mark) == -2); }
        const int keep = active[k];
        active[k] = sp[k].count + 1;
        CHECK(roster_plan_leave(sp, n_shards, active, NULL, 0, src, dst, na, mark) == -1);
        active[k] = keep;
    }
    /* the split: pairs inside a shard in the shard's own indices, the others as they came */
    if (n_shards >= 2 && sp[0].count >= 2 && sp[1].count >= 2) {
        const int f1 = sp[1].first;
        int c[3] = {f1 + 1, 0, 1}, d[3] = {f1, sp[n_shards - 1].first + sp[n_shards - 1].count - 1, 0};
        const int last_same = shard_of(sp, n_shards, d[1], &ls[0]) == 0;
        const int nx = roster_split(sp, n_shards, c, d, 3, first, ls, ld, xs, xd);
        CHECK(nx == (last_same ? 0 : 1));
        CHECK(first[0] == 0 && first[1] == (last_same ? 2 : 1) && first[2] == first[1] + 1 && first[n_shards] == 3 - nx);
        CHECK(ls[first[1]] == 1 && ld[first[1]] == 0);               /* shard 1's pair, local */
        CHECK(ls[first[1] - 1] == 1 && ld[first[1] - 1] == 0);       /* shard 0's pair 1 -> 0 */
        if (nx) CHECK(xs[0] == 0 && xd[0] == d[1]);
    }
}

int main(void)
{
    unsigned rng = 12345u;
    for (g_n = 1; g_n <= MAXN; g_n++)
        for (g_K = 1; g_K <= 8; g_K++) {
            n_shards = shard_partition(g_n, g_K, sp);
            CHECK(roster_streams(sp, n_shards) == g_n);
            for (int k = 0; k < n_shards; k++) {
                active[k] = sp[k].count;
                if ((g_n + g_K) & 1) { rng = rng * 1664525u + 1013904223u; active[k] = (int)((rng >> 16) % (unsigned)(sp[k].count + 1)); }      /* every other case: a partial roster */
            }
            all_sets();
            refusals();
        }
    printf("ok %ld\n", checks);
    return 0;
}
