/* Stream snapshots (include/lpcnet_batch.h: lpcnet_batch_snapshot): the record of one stream, the layout that describes it, the rule by which a
 * layout fits a batch, and the header of a snapshot blob.  Plain C with no HIP include, like api_roster.h and encode_plan.h: engine_snapshot.hip
 * builds its copy tables from these layouts, api_batch.c writes and parses blobs with them, and api_tools.c reports them without a device.
 *
 * A RECORD is every per-stream array of the batch (engine_roster.hip: each_stream_array) end to end, one SECTION each, in the order of the section
 * ids, every section on a 16-byte boundary; the two host halves -- the PLC's control ints and the kept products' flag -- are sections too.  The
 * record's length is a multiple of 16.  Nothing is re-encoded: a section's bytes are the device array's.
 * A LAYOUT is an int array: {record bytes, sections k, the head fields below, k x {id, bytes per stream, offset}}.
 * A BLOB is ints {magic, version, m}, the layout, meta [m][LPCNET_SNAP_META] ints (the host halves), zeros up to a 16-byte boundary, m records. */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "lpcnet_batch.h"
#include "lpcnet_engine.h"

#define LPCN_SNAP_MAGIC   0x5343504C      /* "LPCS" as the blob's first four bytes */
#define LPCN_SNAP_VERSION 1
#define LPCN_SNAP_MAX_SECTIONS 26         /* roster_kernels.hip.h: ROSTER_MAX_ROWS device arrays and the two host halves */
/* the layout's ints */
enum { SNAP_L_RECORD, SNAP_L_SECTIONS, SNAP_L_FLAVOUR, SNAP_L_PLC, SNAP_L_PLC_OPTIONS, SNAP_L_G1, SNAP_L_G2, SNAP_L_DENC_FLOATS, SNAP_L_DENC_DFRAMES,
       SNAP_L_STATE_SIZE, SNAP_L_AN_SIZE, SNAP_L_PLC_SIZE, SNAP_L_HASH_LO, SNAP_L_HASH_HI, SNAP_L_HEAD };
#define LPCN_SNAP_LAYOUT_MAX LPCNET_SNAP_LAYOUT_INTS
#define LPCN_SNAP_BLOB_HEAD 3             /* magic, version, m in front of the layout */
/* a configuration (lpcnet_hip_snapshot_layout): which subsystems exist and the sizes that depend on the model */
enum { SNAP_C_FLAVOUR, SNAP_C_ANALYSIS, SNAP_C_ENCODER, SNAP_C_KEEP, SNAP_C_PLC, SNAP_C_PLC_OPTIONS, SNAP_C_G1, SNAP_C_G2, SNAP_C_DENC_FLOATS, SNAP_C_DENC_DFRAMES,
       SNAP_C_COUNT };
#ifdef __cplusplus
#define SNAP_STATIC_ASSERT static_assert
#else
#define SNAP_STATIC_ASSERT _Static_assert
#endif
SNAP_STATIC_ASSERT(SNAP_C_COUNT == LPCNET_SNAP_CONFIG, "include/lpcnet_batch.h: LPCNET_SNAP_CONFIG is stale");
SNAP_STATIC_ASSERT(sizeof(lpcn_plc_ctl) == sizeof(int) * (LPCNET_SNAP_META - 1), "include/lpcnet_batch.h: LPCNET_SNAP_META is stale");
SNAP_STATIC_ASSERT(SNAP_L_HEAD + 3 * LPCN_SNAP_MAX_SECTIONS == LPCNET_SNAP_LAYOUT_INTS, "include/lpcnet_batch.h: LPCNET_SNAP_LAYOUT_INTS is stale");

static inline const int *snap_section(const int *lay, int k) { return lay + SNAP_L_HEAD + 3 * k; }
static inline int snap_layout_ints(const int *lay) { return SNAP_L_HEAD + 3 * lay[SNAP_L_SECTIONS]; }
/* the section with this id, or NULL */
static inline const int *snap_find(const int *lay, int id)
{
    for (int k = 0; k < lay[SNAP_L_SECTIONS]; k++) if (snap_section(lay, k)[0] == id) return snap_section(lay, k);
    return NULL;
}
static inline const char *snap_section_name(int id)
{
    static const char *const name[] = {"?", "SYNTH", "DEC_VQ", "AN", "ENC_VQ", "KEEP_A", "KEEP_B", "KEEP_LPC", "KEEP_FLAG", "PLC_Q", "PLC_FEAT", "PLC_NET", "PLC_DC",
                                       "PLC_DELTA", "PLC_FEC", "PLC_FBUF", "PLC_LP", "PLC_BURG", "PLC_AN", "PLC_CTL", "DRED_ENC", "DRED_DEC"};
    return id >= 1 && id <= LPCNET_SNAP_DRED_DEC ? name[id] : name[0];
}
static inline int snap_is_plc(int id) { return id >= LPCNET_SNAP_PLC_Q && id <= LPCNET_SNAP_PLC_CTL; }
static inline int snap_is_host_half(int id) { return id == LPCNET_SNAP_KEEP_FLAG || id == LPCNET_SNAP_PLC_CTL; }

/* The layout of a configuration; the three struct sizes are the library's own.  Returns the layout's ints, or -1 for a configuration that has
 * no layout (negative or odd sizes, PLC widths beyond the engine's).  ddec: floats of the DRED decoder's record (0: the batch has none) -- no field
 * of the public ten-int configuration and none of the head: the section's own size says it, and a configuration describes a batch without it. */
static inline int snap_layout_build_dec(const int *cfg, int ddec, unsigned long long model_hash, int *lay)
{
    int k = 0;
    long long off = 0;
    const int plc = cfg[SNAP_C_PLC] != 0, g1 = plc ? cfg[SNAP_C_G1] : 0, g2 = plc ? cfg[SNAP_C_G2] : 0, denc = cfg[SNAP_C_DENC_FLOATS];
    if (denc < 0 || ddec < 0 || (plc && (g1 < 1 || g2 < 1 || g1 > LPCN_PLC_MAX_UNITS || g2 > LPCN_PLC_MAX_UNITS))) return -1;
#define SNAP_ADD(id, nbytes) do { int *s_ = lay + SNAP_L_HEAD + 3 * k++; s_[0] = (id); s_[1] = (int)(nbytes); s_[2] = (int)off; off = (off + s_[1] + 15) / 16 * 16; } while (0)
    SNAP_ADD(LPCNET_SNAP_SYNTH, sizeof(lpcn_stream_state));
    SNAP_ADD(LPCNET_SNAP_DEC_VQ, sizeof(float) * LPCN_NB_BANDS);
    if (cfg[SNAP_C_ANALYSIS] || cfg[SNAP_C_ENCODER] || plc) SNAP_ADD(LPCNET_SNAP_AN, sizeof(lpcn_analysis_state));      /* (the encoder and the PLC imply the analysis) */
    if (cfg[SNAP_C_ENCODER]) SNAP_ADD(LPCNET_SNAP_ENC_VQ, sizeof(float) * LPCN_NB_BANDS);
    if (cfg[SNAP_C_KEEP] || plc) {                                                                                      /* (... and the PLC the kept products) */
        SNAP_ADD(LPCNET_SNAP_KEEP_A, sizeof(float) * LPCN_ROWS_A); SNAP_ADD(LPCNET_SNAP_KEEP_B, sizeof(float) * LPCN_ROWS_B);
        SNAP_ADD(LPCNET_SNAP_KEEP_LPC, sizeof(float) * LPCN_LPC_ORDER);
    }
    SNAP_ADD(LPCNET_SNAP_KEEP_FLAG, sizeof(int));
    if (plc) {
        SNAP_ADD(LPCNET_SNAP_PLC_Q, sizeof(short) * LPCN_PLC_QUEUE); SNAP_ADD(LPCNET_SNAP_PLC_FEAT, sizeof(float) * LPCN_NB_FEAT);
        SNAP_ADD(LPCNET_SNAP_PLC_NET, sizeof(float) * 4 * ((size_t)g1 + g2)); SNAP_ADD(LPCNET_SNAP_PLC_DC, sizeof(double) * 2);
        SNAP_ADD(LPCNET_SNAP_PLC_DELTA, sizeof(int)); SNAP_ADD(LPCNET_SNAP_PLC_FEC, sizeof(float) * LPCN_PLC_MAX_FEC * LPCN_NB_FEAT);
        SNAP_ADD(LPCNET_SNAP_PLC_FBUF, sizeof(float) * LPCN_PLC_FBUF * LPCN_NB_FEAT); SNAP_ADD(LPCNET_SNAP_PLC_LP, sizeof(short) * LPCN_FRAME_SIZE);
        SNAP_ADD(LPCNET_SNAP_PLC_BURG, sizeof(float) * 2 * LPCN_NB_BANDS); SNAP_ADD(LPCNET_SNAP_PLC_AN, sizeof(float) * LPCN_AN_NB_FEATURES);
        SNAP_ADD(LPCNET_SNAP_PLC_CTL, sizeof(lpcn_plc_ctl));
    }
    if (denc) SNAP_ADD(LPCNET_SNAP_DRED_ENC, sizeof(float) * (size_t)denc);
    if (ddec) SNAP_ADD(LPCNET_SNAP_DRED_DEC, sizeof(float) * (size_t)ddec);
#undef SNAP_ADD
    if (off > 0x7ffffff0LL) return -1;
    lay[SNAP_L_RECORD] = (int)off; lay[SNAP_L_SECTIONS] = k;
    lay[SNAP_L_FLAVOUR] = cfg[SNAP_C_FLAVOUR] != 0; lay[SNAP_L_PLC] = plc; lay[SNAP_L_PLC_OPTIONS] = plc ? cfg[SNAP_C_PLC_OPTIONS] : 0;
    lay[SNAP_L_G1] = g1; lay[SNAP_L_G2] = g2; lay[SNAP_L_DENC_FLOATS] = denc; lay[SNAP_L_DENC_DFRAMES] = denc ? cfg[SNAP_C_DENC_DFRAMES] : 0;
    lay[SNAP_L_STATE_SIZE] = (int)sizeof(lpcn_stream_state); lay[SNAP_L_AN_SIZE] = (int)sizeof(lpcn_analysis_state); lay[SNAP_L_PLC_SIZE] = (int)sizeof(lpcn_plc_state_rec);
    lay[SNAP_L_HASH_LO] = (int)(unsigned)(model_hash & 0xffffffffu); lay[SNAP_L_HASH_HI] = (int)(unsigned)(model_hash >> 32);
    return SNAP_L_HEAD + 3 * k;
}
static inline int snap_layout_build(const int *cfg, unsigned long long model_hash, int *lay) { return snap_layout_build_dec(cfg, 0, model_hash, lay); }

/* Is this int array of `n` ints a layout?  Known ids in rising order, sizes that are whole ints, every section at the rounded end of the one before it, the record
 * the rounded end of the last. */
static inline int snap_layout_valid(const int *lay, int n)
{
    if (n < SNAP_L_HEAD) return 0;
    const int k = lay[SNAP_L_SECTIONS];
    if (k < 1 || k > LPCN_SNAP_MAX_SECTIONS || n < SNAP_L_HEAD + 3 * k) return 0;
    long long end = 0;
    int last = 0;
    for (int i = 0; i < k; i++) {
        const int *s = snap_section(lay, i);
        if (s[0] <= last || s[0] > LPCNET_SNAP_DRED_DEC || s[1] < 4 || s[1] % 4 || s[2] != end) return 0;
        last = s[0];
        end = ((long long)s[2] + s[1] + 15) / 16 * 16;
    }
    return end == lay[SNAP_L_RECORD];
}

/* Does a snapshot of layout `snap` fit a batch of layout `mine`?  0: yes (a section only the batch has receives a fresh stream's record).
 * 1: yes once the batch has enabled the subsystems whose sections only the snapshot has -- the host forms do that; with enqueue_only it is a
 * refusal like the rest.  -1: no, with the reason in msg and the section it is about in *section (0: none). */
static inline int snap_layout_match(const int *snap, const int *mine, int enqueue_only, int *section, char *msg, size_t msg_len)
{
    int need = 0, sec = 0;
    if (section) *section = 0;
    if (snap[SNAP_L_STATE_SIZE] != mine[SNAP_L_STATE_SIZE] || snap[SNAP_L_AN_SIZE] != mine[SNAP_L_AN_SIZE] || snap[SNAP_L_PLC_SIZE] != mine[SNAP_L_PLC_SIZE]) {
        snprintf(msg, msg_len, "snapshot: taken by a build with other state structs (%d / %d / %d bytes, this one %d / %d / %d)", snap[SNAP_L_STATE_SIZE],
                 snap[SNAP_L_AN_SIZE], snap[SNAP_L_PLC_SIZE], mine[SNAP_L_STATE_SIZE], mine[SNAP_L_AN_SIZE], mine[SNAP_L_PLC_SIZE]);
        return -1;
    }
    if (snap[SNAP_L_FLAVOUR] != mine[SNAP_L_FLAVOUR]) {
        snprintf(msg, msg_len, "snapshot: taken from %s model, the batch runs %s one", snap[SNAP_L_FLAVOUR] ? "an int8" : "a float", mine[SNAP_L_FLAVOUR] ? "an int8" : "a float");
        return -1;
    }
    if (snap[SNAP_L_PLC] != mine[SNAP_L_PLC] || snap[SNAP_L_PLC_OPTIONS] != mine[SNAP_L_PLC_OPTIONS] || snap[SNAP_L_G1] != mine[SNAP_L_G1] || snap[SNAP_L_G2] != mine[SNAP_L_G2]) {
        sec = !snap[SNAP_L_PLC] || !mine[SNAP_L_PLC] || snap[SNAP_L_PLC_OPTIONS] != mine[SNAP_L_PLC_OPTIONS] ? LPCNET_SNAP_PLC_CTL : LPCNET_SNAP_PLC_NET;
        if (section) *section = sec;
        snprintf(msg, msg_len, "snapshot: the packet-loss concealment differs (section %s: snapshot %s, options %d, widths %d / %d; batch %s, options %d, widths %d / %d)",
                 snap_section_name(sec), snap[SNAP_L_PLC] ? "on" : "off", snap[SNAP_L_PLC_OPTIONS], snap[SNAP_L_G1], snap[SNAP_L_G2],
                 mine[SNAP_L_PLC] ? "on" : "off", mine[SNAP_L_PLC_OPTIONS], mine[SNAP_L_G1], mine[SNAP_L_G2]);
        return -1;
    }
    for (int k = 0; k < snap[SNAP_L_SECTIONS]; k++) {
        const int *s = snap_section(snap, k), *t = snap_find(mine, s[0]);
        if (t && t[1] != s[1]) {
            if (section) *section = s[0];
            snprintf(msg, msg_len, "snapshot: section %s has %d bytes per stream, the batch's %d", snap_section_name(s[0]), s[1], t[1]);
            return -1;
        }
        if (!t && !need) { need = 1; sec = s[0]; }
    }
    if (need && enqueue_only) {
        if (section) *section = sec;
        snprintf(msg, msg_len, "snapshot: section %s is not allocated in the batch (enable the subsystem first, or restore through the host form)", snap_section_name(sec));
        return -1;
    }
    return need;
}

/* ---- the blob ---- */
static inline size_t snap_blob_records_at(const int *lay, int m)
{
    const size_t head = sizeof(int) * ((size_t)LPCN_SNAP_BLOB_HEAD + (size_t)snap_layout_ints(lay) + (size_t)m * LPCNET_SNAP_META);
    return (head + 15) / 16 * 16;
}
static inline size_t snap_blob_bytes(const int *lay, int m) { return snap_blob_records_at(lay, m) + (size_t)m * (size_t)lay[SNAP_L_RECORD]; }
/* header and layout into buf (cap bytes); *meta and *records point at the two areas the caller fills.  0, or -1 when cap is too small */
static inline int snap_blob_begin(void *buf, size_t cap, const int *lay, int m, int **meta, char **records)
{
    if (!buf || (uintptr_t)buf % sizeof(int) || m < 0 || cap < snap_blob_bytes(lay, m)) return -1;
    int *h = (int *)buf;
    const size_t at = snap_blob_records_at(lay, m);
    memset(buf, 0, at);
    h[0] = LPCN_SNAP_MAGIC; h[1] = LPCN_SNAP_VERSION; h[2] = m;
    memcpy(h + LPCN_SNAP_BLOB_HEAD, lay, sizeof(int) * (size_t)snap_layout_ints(lay));
    *meta = h + LPCN_SNAP_BLOB_HEAD + snap_layout_ints(lay);
    *records = (char *)buf + at;
    return 0;
}
/* a blob of len bytes: its m, layout (into lay, LPCN_SNAP_LAYOUT_MAX ints), meta and records.  0, or -1 for a NULL, truncated, wrong-magic or
 * wrong-version buffer or one whose lengths do not add up; every length is checked against len before anything behind it is read */
static inline int snap_blob_parse(const void *buf, size_t len, int *m, int *lay, const int **meta, const char **records)
{
    int h[LPCN_SNAP_BLOB_HEAD + SNAP_L_HEAD];
    if (!buf || (uintptr_t)buf % sizeof(int) || len < sizeof(h)) return -1;
    memcpy(h, buf, sizeof(h));
    if (h[0] != LPCN_SNAP_MAGIC || h[1] != LPCN_SNAP_VERSION || h[2] < 0) return -1;
    const int k = h[LPCN_SNAP_BLOB_HEAD + SNAP_L_SECTIONS];
    if (k < 1 || k > LPCN_SNAP_MAX_SECTIONS || len < sizeof(int) * ((size_t)LPCN_SNAP_BLOB_HEAD + SNAP_L_HEAD + 3 * (size_t)k)) return -1;
    memcpy(lay, (const char *)buf + sizeof(int) * LPCN_SNAP_BLOB_HEAD, sizeof(int) * ((size_t)SNAP_L_HEAD + 3 * (size_t)k));
    if (!snap_layout_valid(lay, SNAP_L_HEAD + 3 * k)) return -1;
    {   /* a blob's head and sections say the same about the DRED encoder: the section is there with the head's floats, or neither is */
        const int *d = snap_find(lay, LPCNET_SNAP_DRED_ENC);
        if (lay[SNAP_L_DENC_FLOATS] ? (!d || d[1] != 4 * lay[SNAP_L_DENC_FLOATS]) : d != NULL) return -1;
    }
    if ((size_t)h[2] > (len - sizeof(h)) / ((size_t)lay[SNAP_L_RECORD] + sizeof(int) * LPCNET_SNAP_META) || len < snap_blob_bytes(lay, h[2])) return -1;
    *m = h[2];
    if (meta) *meta = (const int *)buf + LPCN_SNAP_BLOB_HEAD + snap_layout_ints(lay);
    if (records) *records = (const char *)buf + snap_blob_records_at(lay, h[2]);
    return 0;
}
