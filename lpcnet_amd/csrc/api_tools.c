/* C host shell of the LPCNet HIP engine, the seams for tools and tests that need no batch (include/lpcnet_batch.h): host-only views of a
 * weight blob, the PLC planners without a device, and the device probes of the arithmetic. */
#include "api_internal.h"
#include "sample_variants.h"
#include "encode_plan.h"
#include "snapshot_plan.h"

/* what the caller did to each stream's FEC ring before the step: fec_op [n] (may be NULL): 1 = a vector was added, 2 = a NULL skip, 3 = fec_clear,
 * 4 = two vectors */
static void apply_fec_ops(lpcn_plc_ctl *c, int n, const unsigned char *fec_op)
{
    for (int s = 0; fec_op && s < n; s++) {
        if (fec_op[s] == 1) (void)lpcn_plc_ctl_fec_add(&c[s], 0);
        else if (fec_op[s] == 2) (void)lpcn_plc_ctl_fec_add(&c[s], 1);
        else if (fec_op[s] == 3) c[s].fec_keep = c[s].fec_read = c[s].fec_fill = c[s].fec_skip = 0;
        else if (fec_op[s] == 4) { (void)lpcn_plc_ctl_fec_add(&c[s], 0); (void)lpcn_plc_ctl_fec_add(&c[s], 0); }
    }
}

/* the planner alone (no device): ctl [n][9] ints in and out (pcm_fill, skip_analysis, blend, loss_count, fec_fill, fec_keep, fec_read, fec_skip,
 * deferred-queue fill; all zero but pcm_fill = 400 after a reset), fec_op as above; summary [n][10] */
int lpcnet_hip_plc_plan(int options, int n, int *ctl, const unsigned char *lost, const unsigned char *fec_op, int *summary)
{
    if (n < 1 || !ctl || !lost) { set_err("lpcnet_hip_plc_plan: bad arguments"); return LPCN_E_ARG; }
    lpcn_plc_ctl *c = (lpcn_plc_ctl *)ctl;
    apply_fec_ops(c, n, fec_op);
    FWD(lpcn_plc_plan(options, n, c, lost, summary));
}
/* the same with lanes: the launches and the control lists come back as well (include/lpcnet_batch.h) */
int lpcnet_hip_plc_plan_lanes(int options, int n, int lanes, int *ctl, const unsigned char *lost, const unsigned char *fec_op, int *summary,
                              int *launch, int launch_cap, int *lists, int lists_cap)
{
    char err[256] = "";
    if (n < 1 || !ctl || !lost) { set_err("lpcnet_hip_plc_plan_lanes: bad arguments"); return LPCN_E_ARG; }
    if (lanes < 1 || lanes > 4) { set_err("lpcnet_hip_plc_plan_lanes: lanes must be 1 .. 4"); return LPCN_E_ARG; }      /* (before fec_op changes ctl) */
    lpcn_plc_ctl *c = (lpcn_plc_ctl *)ctl;
    lpcn_plc_ctl *before = (lpcn_plc_ctl *)malloc(sizeof(*c) * (size_t)n);
    if (!before) { set_err("lpcnet_hip_plc_plan_lanes: out of memory"); return LPCN_E_ARG; }
    memcpy(before, c, sizeof(*c) * (size_t)n);
    apply_fec_ops(c, n, fec_op);
    const int rc = lpcn_plc_plan_lanes(options, n, lanes, c, lost, summary, launch, launch_cap, lists, lists_cap, err, sizeof(err));
    if (rc < 0) { memcpy(c, before, sizeof(*c) * (size_t)n); set_err(err); }
    free(before);
    return rc;
}
/* the prediction kernels' form rule alone (no device): include/lpcnet_batch.h */
int lpcnet_hip_plc_pred_form(int n_records, int cus, int d1, int g1, int g2, int int8, int pinned)
{
    const int rc = lpcn_plc_pred_form(n_records, cus, d1, g1, g2, int8, pinned);
    if (rc < 0) set_err("lpcnet_hip_plc_pred_form: pinned must be 0, 1, 2, 4 or 8, n_records at least 0, cus and the widths at least 1");
    return rc;
}
/* the FEC feed's planner alone (no device): ctl as above, count [n], skip / clear [n] or NULL, rec [n][8] out (one record per stream that stores
 * something: stream, first source row, rows a, their ring row, move-from row, rows moved, rows b, their ring row), dropped [n] or NULL.  Returns
 * the number of records. */
int lpcnet_hip_plc_fec_feed_plan(int n, int *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped)
{
    const int rc = lpcn_plc_fec_feed_plan(n, (lpcn_plc_ctl *)ctl, count, skip, clear, rec, dropped);
    if (rc < 0) take_engine_err();
    return rc;
}

/* tools (include/lpcnet_batch.h): lpcnet_decode's unpacker alone, on the host, under the codebooks' read lock (no device) */
int lpcnet_hip_packet_features(const unsigned char *buf8, float *vq_mem18, float *features4x36)
{
    if (!buf8 || !vq_mem18 || !features4x36) { set_err("lpcnet_hip_packet_features: bad arguments"); return LPCN_E_ARG; }
    const float *const *cb = codebooks_rdlock(NULL);
    const int rc = packet_to_features(cb, (float (*)[NB_TOTAL_FEATURES])features4x36, vq_mem18, buf8);
    codebooks_unlock();
    if (rc) { set_err("lpcnet_hip_packet_features: no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    return 0;
}

/* tools (include/lpcnet_batch.h): the launches of one lpcnet_batch_encode / lpcnet_batch_analyze call by the engine's own rules (encode_plan.h), no device */
int lpcnet_hip_encode_plan(int n, int active, int count, int analysis, int *out, int cap)
{
    if (n < 1 || active < 0 || active > n || count < 1 || cap < 0 || (cap && !out)) { set_err("lpcnet_hip_encode_plan: bad arguments"); return LPCN_E_ARG; }
    const int chunk = analysis ? lpcn_analysis_chunk(n, count) : lpcn_encode_chunk(n, count);
    int k = 0;
    for (int c0 = 0; active && c0 < count; c0 += chunk, k++) {
        if (k >= cap) continue;
        int *r = out + 8 * k;
        const size_t items = (size_t)active * (count - c0 < chunk ? count - c0 : chunk);
        memset(r, 0, sizeof(int) * 8);
        r[0] = count - c0 < chunk ? count - c0 : chunk;
        r[1] = (int)items;
        if (analysis) continue;
        r[2] = lpcn_encode_ipw(items, LPCN_ENC_END_IPW);
        r[3] = lpcn_encode_ipw(items, LPCN_ENC_MID_IPW);
        for (int v = 0; v < 2; v++) {
            const size_t per = (size_t)LPCN_ENC_VQ_WAVES * r[2 + v], wg = (items + per - 1) / per;
            r[4 + 2 * v] = (int)wg;
            r[5 + 2 * v] = (int)(items - (wg - 1) * per);
        }
    }
    return k;
}

/* stream snapshots without a device (include/lpcnet_batch.h; snapshot_plan.h): the layout of a configuration, a blob's header, the match rule */
int lpcnet_hip_snapshot_layout(const int *config, int *out, int cap)
{
    int lay[LPCN_SNAP_LAYOUT_MAX];
    if (!config || cap < 0 || (cap && !out) || snap_layout_build(config, 0, lay) < 0) { set_err("lpcnet_hip_snapshot_layout: bad configuration"); return LPCN_E_ARG; }
    const int k = lay[SNAP_L_SECTIONS];
    for (int i = 0; i < 3 * k && i < cap; i++) out[i] = lay[SNAP_L_HEAD + i];
    if (cap > 3 * k) out[3 * k] = lay[SNAP_L_RECORD];
    return k;
}
int lpcnet_hip_snapshot_info(const void *buf, size_t len, int *info, int cap)
{
    int lay[LPCN_SNAP_LAYOUT_MAX], m = 0, n = 0;
    if (cap < 0 || (cap && !info)) { set_err("lpcnet_hip_snapshot_info: bad arguments"); return LPCN_E_ARG; }
    if (snap_blob_parse(buf, len, &m, lay, NULL, NULL)) { set_err("lpcnet_hip_snapshot_info: not a snapshot blob (NULL, truncated, wrong magic or version, or lengths that do not add up)"); return LPCN_E_ARG; }
    const int head[4] = {LPCN_SNAP_VERSION, m, lay[SNAP_L_RECORD], lay[SNAP_L_SECTIONS]};
    for (int i = 0; i < 4 && n < cap; i++) info[n++] = head[i];
    for (int i = SNAP_L_FLAVOUR; i < snap_layout_ints(lay) && n < cap; i++) info[n++] = lay[i];
    return n;
}
int lpcnet_hip_snapshot_match(const int *config_snap, const int *config_batch, int enqueue_only, int *section)
{
    int snap[LPCN_SNAP_LAYOUT_MAX], mine[LPCN_SNAP_LAYOUT_MAX];
    char msg[400];
    if (!config_snap || !config_batch || snap_layout_build(config_snap, 0, snap) < 0 || snap_layout_build(config_batch, 0, mine) < 0) { set_err("lpcnet_hip_snapshot_match: bad configuration"); return LPCN_E_ARG; }
    const int fit = snap_layout_match(snap, mine, enqueue_only, section, msg, sizeof(msg));
    if (fit < 0) { set_err(msg); return LPCN_E_MODEL; }
    return fit;
}

/* tools: how GRU-A's rows were dealt to the 8 waves of the sample kernel: out[0] = items per lane, then per wave
 * {bound[0..3], allh[0..2]} (item index where each slot starts / slot holds only candidate rows), then out[57 + wave] =
 * items of slot 0's chains computed one sample ahead (stored end-aligned, [nw - head, nw)) */
int lpcnet_hip_model_layout(const unsigned char *data, int len, int *out)
{
    lpcn_model_host m;
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return -1; }
    out[0] = m.nw;
    for (int w = 0; w < LPCN_WAVES; w++) {
        for (int k = 0; k < 4; k++) out[1 + w * 7 + k] = m.pk_a_bound[w][k];
        for (int k = 0; k < 3; k++) out[1 + w * 7 + 4 + k] = m.pk_a_allh[w][k];
        out[57 + w] = m.pk_a_head[w];
    }
    lpcn_model_release(&m);
    return 0;
}

int lpcnet_hip_exp10_device(const float *x, double *out, int n)
{
    if (!x || !out || n <= 0) { set_err("lpcnet_hip_exp10_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_debug_exp10(single_stream_device(), x, out, (size_t)n));
}

/* test seam (include/lpcnet_batch.h): the arithmetic identities the PARITY kernels rest on, on the device */
int lpcnet_hip_arith_identities_device(const float *a, const float *b, unsigned *out_mfma, unsigned *out_mul, unsigned *out_pk, unsigned *out_sc, int n)
{
    if (!a || !b || !out_mfma || !out_mul || !out_pk || !out_sc || n <= 0) { set_err("lpcnet_hip_arith_identities_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_debug_arith_identities(single_stream_device(), a, b, out_mfma, out_mul, out_pk, out_sc, (size_t)n));
}

/* test seam (include/lpcnet_batch.h): the int8 kernels' one-instruction re-quantisation against the reference's formula, exhaustively */
int lpcnet_hip_quant_sweep_device(unsigned long long *out3)
{
    if (!out3) { set_err("lpcnet_hip_quant_sweep_device: bad arguments"); return LPCN_E_ARG; }
    FWD(lpcn_debug_quant_sweep(single_stream_device(), out3));
}

/* Host-only view of a blob's PLC network (no GPU needed): info[0..6] = {present (0 none, 1 float arrays, 2 int8 arrays, -1 incomplete or
 * inconsistent), servable (the arrays are in the blob's own flavour: lpcnet_batch_plc_enable accepts the blob), d1, g1, g2, blocks of the
 * two GRU input matrices}.  Returns 0, LPCN_E_ARG without `info`, LPCN_E_MODEL when the blob does not load as an LPCNet model at all. */
int lpcnet_hip_plc_model_info(const unsigned char *data, int len, int *info)
{
    lpcn_model_host m;
    if (!info) { set_err("lpcnet_hip_plc_model_info: bad arguments"); return LPCN_E_ARG; }
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return LPCN_E_MODEL; }
    info[0] = m.plc.present; info[1] = lpcn_plc_servable(&m);
    info[2] = m.plc.dense1.n_out; info[3] = m.plc.gru[0].n; info[4] = m.plc.gru[1].n; info[5] = m.plc.gru[0].nb; info[6] = m.plc.gru[1].nb;
    lpcn_model_release(&m);
    return 0;
}

/* Host-only view of a blob's DRED decoder (no GPU needed): info[0..11] = {present (0 none, 1 float arrays, 2 int8 arrays, -1 incomplete or
 * inconsistent), servable (lpcnet_batch_dred_enable accepts the blob), latent dimension, state dimension, the widths of dec_dense1 .. dec_dense8}.
 * Returns 0, LPCN_E_ARG without `info`, LPCN_E_MODEL when the blob does not load as an LPCNet model at all. */
int lpcnet_hip_dred_model_info(const unsigned char *data, int len, int *info)
{
    lpcn_model_host m;
    if (!info) { set_err("lpcnet_hip_dred_model_info: bad arguments"); return LPCN_E_ARG; }
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return LPCN_E_MODEL; }
    info[0] = m.dred.present; info[1] = lpcn_dred_servable(&m);
    info[2] = m.dred.latent_dim; info[3] = m.dred.state_dim;
    for (int k = 0; k < 8; k++) info[4 + k] = m.dred.width[k];
    lpcn_model_release(&m);
    return 0;
}

/* Host-only view of a blob's DRED encoder (no GPU needed): info[0..14] = {present (0 none, 1 float arrays, 2 int8 arrays, -1 incomplete or
 * inconsistent), servable (lpcnet_batch_dred_enc_enable accepts the blob), latent dimension, state dimension, taps of bits_dense, width of gdense1,
 * floats of one stream's state, the widths of enc_dense1 .. enc_dense8}.  Returns like lpcnet_hip_dred_model_info. */
int lpcnet_hip_dred_enc_model_info(const unsigned char *data, int len, int *info)
{
    lpcn_model_host m;
    if (!info) { set_err("lpcnet_hip_dred_enc_model_info: bad arguments"); return LPCN_E_ARG; }
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return LPCN_E_MODEL; }
    const lpcn_dred_enc_model *p = &m.dred_enc;
    int total = 0;
    for (int k = 0; k < 8; k++) total += p->width[k];
    info[0] = p->present; info[1] = lpcn_dred_enc_servable(&m);
    info[2] = p->latent_dim; info[3] = p->state_dim; info[4] = p->taps; info[5] = p->gdense1;
    info[6] = p->present > 0 ? p->width[1] + p->width[3] + p->width[5] + (p->taps - 1) * total : 0;
    for (int k = 0; k < 8; k++) info[7 + k] = p->width[k];
    lpcn_model_release(&m);
    return 0;
}

/* Host-only model check (no GPU needed): parses the blob with the loader's rules, builds the device
 * packings and verifies them.  info[0..5] = {is_int8, blocks GRU-A, blocks GRU-B, items per lane,
 * padded GRU-B blocks, selftest code}.  Returns 0 if the blob is loadable by the engine (float or
 * int8 flavour, see info[0]), -1 if it is malformed (lpcnet_load_model would fail). */
int lpcnet_hip_check_model(const unsigned char *data, int len, int *info)
{
    lpcn_model_host m;
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return -1; }
    int st = lpcn_model_selftest(&m);
    if (!st) {                                           /* the FAST arithmetic's own GRU-A packing, where there is one (int8 blobs) */
        lpcn_model_host f;
        const int pf = lpcn_model_pack_fast(&m, &f);
        if (pf < 0) st = 100;
        else if (pf == 0) {
            f.pk_b_w = m.pk_b_w; f.pk_b_wq = m.pk_b_wq; f.pk_b_start = m.pk_b_start; f.pk_b_blk = m.pk_b_blk;      /* (the check reads GRU-B's packing too: shared) */
            const int sf = lpcn_model_selftest(&f);
            if (sf) st = 100 + sf;
            f.pk_b_w = NULL; f.pk_b_wq = NULL; f.pk_b_start = NULL; f.pk_b_blk = NULL;
            lpcn_model_release(&f);
        }
    }
    if (!st && !m.is_int8) {                             /* the two-group kernel's own GRU-A packing (float blobs that fit it) */
        lpcn_model_host f;
        if (lpcn_model_pack_x2(&m, &f) == 0) {
            f.pk_b_w = m.pk_b_w; f.pk_b_start = m.pk_b_start; f.pk_b_blk = m.pk_b_blk;
            const int sf = lpcn_model_selftest(&f);
            if (sf) st = 200 + sf;
            f.pk_b_w = NULL; f.pk_b_start = NULL; f.pk_b_blk = NULL;
            lpcn_model_release(&f);
        }
    }
    if (!st) {                                           /* the twelve-wave image, where the model fits it (a model that does not is run by the other kernels) */
        lpcn_x3_image im;
        if (lpcn_model_pack_x3(&m, &im) == 0) {
            const int sf = lpcn_x3_image_selftest(&m, &im);
            if (sf) st = 300 + sf;
            lpcn_x3_image_release(&im);
        }
    }
    if (info) { info[0] = m.is_int8; info[1] = m.nb_a; info[2] = m.nb_b; info[3] = m.nw; info[4] = m.nb_b_padded; info[5] = st; }
    lpcn_model_release(&m);
    if (st) { set_err("internal error: device packing inconsistent with blob"); return -1; }
    return 0;
}

/* Host-only view of the two-group kernel's WIDE image of a blob (sample_kernel_x2.hip.h, the streamed variants of sample_x2w.hip): returns 1 when the
 * model gets one -- a float blob with a dense GRU-B input matrix and 33 .. 96 items per lane in the two-group dealing --, 0 when it does not (the
 * ordinary image serves it, or no two-group kernel runs it), -1 for a malformed blob.  info[21] (may be NULL) = {fits, items per lane of the
 * two-group dealing (0 for int8 blobs), compiled variant, register-resident items of that variant, self-test code, items of waves 0..7 in P1 (b3),
 * candidate-head items of waves 0..7}; variant, resident items and self-test code are -1 without an image. */
int lpcnet_hip_x2_wide_info(const unsigned char *data, int len, int *info)
{
    static const int variants[] = {
#define LPCN_LIST_ITEM(n) n,
        LPCN_VARIANTS_X2W(LPCN_LIST_ITEM)
#undef LPCN_LIST_ITEM
        0};
    lpcn_model_host m, f;
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return -1; }
    int out[21];
    memset(out, 0, sizeof(out));
    out[2] = out[3] = out[4] = -1;
    int have = lpcn_model_pack_x2_wide(&m, &f) == 0;
    if (have) {
        out[1] = f.nw;
        for (int w = 0; w < LPCN_WAVES; w++) { out[5 + w] = f.pk_a_bound[w][LPCN_MAX_SLOTS]; out[5 + LPCN_WAVES + w] = f.pk_a_head[w]; }
        for (const int *v = variants; *v && out[2] < 0; v++) if (f.nw <= *v) out[2] = *v;
        out[3] = LPCN_X2W_NR;
        f.pk_b_w = m.pk_b_w; f.pk_b_start = m.pk_b_start; f.pk_b_blk = m.pk_b_blk;      /* (the check reads GRU-B's packing too: shared) */
        out[4] = lpcn_model_selftest(&f);
        f.pk_b_w = NULL; f.pk_b_start = NULL; f.pk_b_blk = NULL;
        lpcn_model_release(&f);
        have = m.b_dense && out[2] > 0 && out[4] == 0;
    } else if (!m.is_int8 && lpcn_model_pack_x2(&m, &f) == 0) {      /* (the ordinary image: its item count, for the caller's information) */
        out[1] = f.nw;
        lpcn_model_release(&f);
    }
    out[0] = have;
    if (info) memcpy(info, out, sizeof(out));
    lpcn_model_release(&m);
    return have;
}

/* Host-only view of the twelve-wave image of a blob (sample_kernel_x3.hip.h): returns 1 when the model has one, 0 when it does not fit
 * (int8, block-sparse GRU-B, an update / reset slot of more than 16 items, a candidate slot of more than 32, no room left), -1 for a
 * malformed blob.  desc (may be NULL) receives [12 waves][5 segments]{kind, first item, items, blocks summed before it}, rows (may be
 * NULL) [12][5][64] GRU-A rows, selftest (may be NULL) the code of lpcn_x3_image_selftest. */
int lpcnet_hip_x3_image_info(const unsigned char *data, int len, int *desc, int *rows, int *selftest)
{
    lpcn_model_host m;
    lpcn_x3_image im;
    if (lpcn_model_parse(&m, data, len) != 0) { set_err("malformed or incomplete DNNw weight blob"); return -1; }
    const int have = lpcn_model_pack_x3(&m, &im) == 0;
    if (have) {
        if (selftest) *selftest = lpcn_x3_image_selftest(&m, &im);
        for (int w = 0; w < LPCN_X3_WAVES; w++)
            for (int k = 0; k <= LPCN_X3_SEGS; k++) {
                int *d = desc ? desc + (w * (1 + LPCN_X3_SEGS) + k) * 4 : NULL;
                if (d) { d[0] = im.kind[w][k]; d[1] = im.first[w][k]; d[2] = im.count[w][k]; d[3] = im.skip[w][k]; }
                if (rows) memcpy(rows + (w * (1 + LPCN_X3_SEGS) + k) * 64, im.row[w][k], sizeof(int) * 64);
            }
        lpcn_x3_image_release(&im);
    }
    lpcn_model_release(&m);
    return have;
}
