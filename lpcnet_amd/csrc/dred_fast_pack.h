/* The FAST DRED decoder's image of a GRU's sparse input matrix (dred_fast_kernels.hip.h), plain C so that a host program can call it
 * (tests/tools/dred_fast_pack_host.c).
 *
 * The blob has the matrix as 8x4 blocks [block][4 cols][8 rows] with one block list {count, pos...} per 8-row group (src/vec.h:347-360).  The FAST
 * kernel multiplies 32 rows at a time on the matrix pipe -- the z, r or h rows of 32 units, that is four 8-row groups -- and one product needs one
 * input column for all its rows.  So a tile (unit tile, gate) is packed over the UNION of its groups' blocks, in ascending input position, and a group
 * that lacks a block of the union has zeros there: fma(0, x, acc) leaves the group's chain where it was, so every row's sum is still the fma chain
 * over its own blocks in list order (sparse_sgemv_accum8x4 of the AVX2 float build, src/vec_avx.h:865-903).  That needs every list ascending, which
 * the packer checks.
 *
 *   start [3 tiles + 1]   first union block of tile 3 t + gate (t: unit tile, units 32 t .. 32 t + 31; gate 0 z, 1 r, 2 h)
 *   pos   [blocks]        a union block's first input column
 *   w     [blocks][4][32] its weights: column c, unit 32 t + i of the gate at [c][i]; zero past the layer's last unit
 */
#pragma once
#include <stdlib.h>
#include <string.h>

#define LPCN_DRED_FAST_TILE 32

typedef struct lpcn_dred_fast_gru {
    int n_in, n, tiles;
    int *start, *pos;
    float *w;
} lpcn_dred_fast_gru;

static inline void lpcn_dred_fast_release(lpcn_dred_fast_gru *o)
{
    free(o->start); free(o->pos); free(o->w);
    memset(o, 0, sizeof(*o));
}

/* w: the blob's blocks, idx: its index stream, n_in inputs, n units (a multiple of 8).  0; -1 out of memory; -2 a block list that is not ascending
 * or leaves the input */
static inline int lpcn_dred_fast_pack(const float *w, const int *idx, int n_in, int n, lpcn_dred_fast_gru *o)
{
    const int groups = 3 * n / 8, tiles = (n + LPCN_DRED_FAST_TILE - 1) / LPCN_DRED_FAST_TILE;
    memset(o, 0, sizeof(*o));
    if (n < 8 || n % 8 || n_in < 4) return -2;
    /* where every group's list begins: its first position in idx and its first block */
    int *at = (int *)malloc(sizeof(int) * 2 * (size_t)(groups + 1));
    char *seen = (char *)malloc((size_t)n_in + 4);
    if (!at || !seen) { free(at); free(seen); return -1; }
    int p = 0, blk = 0, rc = 0;
    for (int g = 0; g < groups && !rc; g++) {
        at[2 * g] = p; at[2 * g + 1] = blk;
        const int cnt = idx[p++];
        for (int k = 0; k < cnt; k++, p++)
            if (idx[p] < 0 || idx[p] + 4 > n_in || (k && idx[p] <= idx[p - 1])) rc = -2;
        blk += cnt;
    }
    at[2 * groups] = p; at[2 * groups + 1] = blk;
    o->n_in = n_in; o->n = n; o->tiles = tiles;
    o->start = (int *)calloc((size_t)3 * tiles + 1, sizeof(int));
    if (!rc && !o->start) rc = -1;
    /* two passes: count the unions, then fill them */
    for (int pass = 0; pass < 2 && !rc; pass++) {
        int total = 0;
        for (int t = 0; t < tiles; t++)
            for (int gate = 0; gate < 3; gate++) {
                const int subs = (n - 32 * t + 7) / 8 < 4 ? (n - 32 * t + 7) / 8 : 4;      /* 8-row groups of this tile */
                const int g0 = (gate * n + 32 * t) / 8;
                memset(seen, 0, (size_t)n_in + 4);
                for (int s = 0; s < subs; s++)
                    for (int k = 0, q = at[2 * (g0 + s)] + 1; k < idx[at[2 * (g0 + s)]]; k++, q++) seen[idx[q]] = 1;
                if (pass) o->start[3 * t + gate] = total;
                const int first = total;
                for (int c = 0; c < n_in; c++)
                    if (seen[c]) { if (pass) o->pos[total] = c; total++; }
                if (!pass) continue;
                for (int s = 0; s < subs; s++) {
                    int u = first;
                    for (int k = 0, q = at[2 * (g0 + s)] + 1; k < idx[at[2 * (g0 + s)]]; k++, q++) {
                        while (o->pos[u] != idx[q]) u++;            /* (both ascending: the union holds every block of the list) */
                        const float *src = w + 32 * (size_t)(at[2 * (g0 + s) + 1] + k);
                        for (int c = 0; c < 4; c++)
                            for (int r = 0; r < 8; r++) o->w[((size_t)u * 4 + c) * 32 + 8 * s + r] = src[8 * c + r];
                    }
                }
            }
        if (!pass) {
            o->pos = (int *)malloc(sizeof(int) * (size_t)(total ? total : 1));
            o->w = (float *)calloc((size_t)(total ? total : 1) * 128, sizeof(float));
            if (!o->pos || !o->w) rc = -1;
        } else o->start[3 * tiles] = total;
    }
    free(at); free(seen);
    if (rc) lpcn_dred_fast_release(o);
    return rc;
}

/* the image read back as the matrix it stands for: dense [3 n][n_in], zero where no block is (for the packer's test) */
static inline void lpcn_dred_fast_unpack(const lpcn_dred_fast_gru *o, float *dense)
{
    memset(dense, 0, sizeof(float) * 3 * (size_t)o->n * o->n_in);
    for (int t = 0; t < o->tiles; t++)
        for (int gate = 0; gate < 3; gate++)
            for (int u = o->start[3 * t + gate]; u < o->start[3 * t + gate + 1]; u++)
                for (int c = 0; c < 4; c++)
                    for (int i = 0; i < 32 && 32 * t + i < o->n; i++) {
                        const float v = o->w[((size_t)u * 4 + c) * 32 + i];
                        if (v != 0.f) dense[(size_t)(gate * o->n + 32 * t + i) * o->n_in + o->pos[u] + c] = v;
                    }
}
