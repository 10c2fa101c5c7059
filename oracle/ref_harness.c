/* TEST INFRASTRUCTURE ONLY -- never linked into the product library.
 *
 * Thin accessor layer compiled *together with* the unmodified reference sources
 * (/root/reference/src, read-only) into oracle/_ref/liblpcnet_ref_<flavour>.so so that Python
 * tests can reach the reference's internal functions and its private LPCNetState without
 * hard-coding struct offsets.  Everything here only forwards to reference code; no algorithm
 * is restated in this file (the restatement lives in oracle/lpcnet_oracle.c).
 */
#include <string.h>
#include "lpcnet_private.h"   /* reference: struct LPCNetState (src/lpcnet_private.h:28-48) */
#include "nnet.h"
#include "common.h"
#include "freq.h"

extern float ceps_codebook1[], ceps_codebook2[], ceps_codebook3[], ceps_codebook_diff4[];

int ref_flavour(void)
{
    int f = 0;
#ifdef DOT_PROD
    f |= 1;            /* int8 weights */
#endif
#ifdef USE_SU_BIAS
    f |= 2;            /* unsigned activations + subias (AVX2 int8) */
#endif
#ifdef NO_OPTIMIZATIONS
    f |= 4;            /* generic C kernels (vec.h:42-409) */
#endif
    return f;
}

void ref_set_codebooks(const float *c1, const float *c2, const float *c3, const float *d4)
{
    memcpy(ceps_codebook1, c1, sizeof(float)*1024*17);
    memcpy(ceps_codebook2, c2, sizeof(float)*1024*17);
    memcpy(ceps_codebook3, c3, sizeof(float)*1024*17);
    memcpy(ceps_codebook_diff4, d4, sizeof(float)*4096*18);
}

/* ---- state access ------------------------------------------------------------------ */
void ref_get_nnet_state(const LPCNetState *st, float *conv1, float *conv2, float *gru_a, float *gru_b)
{
    if (conv1) memcpy(conv1, st->nnet.feature_conv1_state, sizeof(st->nnet.feature_conv1_state));
    if (conv2) memcpy(conv2, st->nnet.feature_conv2_state, sizeof(st->nnet.feature_conv2_state));
    if (gru_a) memcpy(gru_a, st->nnet.gru_a_state, sizeof(st->nnet.gru_a_state));
    if (gru_b) memcpy(gru_b, st->nnet.gru_b_state, sizeof(st->nnet.gru_b_state));
}

void ref_set_gru_state(LPCNetState *st, const float *gru_a, const float *gru_b)
{
    if (gru_a) memcpy(st->nnet.gru_a_state, gru_a, sizeof(st->nnet.gru_a_state));
    if (gru_b) memcpy(st->nnet.gru_b_state, gru_b, sizeof(st->nnet.gru_b_state));
}

/* frame-side products as left in the state by run_frame_network (src/lpcnet.c:275) */
void ref_get_frame_products(const LPCNetState *st, float *lpc, float *cond_a, float *cond_b)
{
    memcpy(lpc, st->lpc, sizeof(st->lpc));
    memcpy(cond_a, st->gru_a_condition, sizeof(st->gru_a_condition));
    memcpy(cond_b, st->gru_b_condition, sizeof(st->gru_b_condition));
}

void ref_get_signal_state(const LPCNetState *st, float *last_sig, int *last_exc, float *deemph_mem,
                          int *frame_count, unsigned *rng4)
{
    memcpy(last_sig, st->last_sig, sizeof(st->last_sig));
    *last_exc = st->last_exc;
    *deemph_mem = st->deemph_mem;
    *frame_count = st->frame_count;
    rng4[0] = st->rng.z; rng4[1] = st->rng.w; rng4[2] = st->rng.jsr; rng4[3] = st->rng.jcong;
}

void ref_get_logit_table(const LPCNetState *st, float *table256)
{
    memcpy(table256, st->sampling_logit_table, sizeof(st->sampling_logit_table));
}

/* ---- entry points with internal linkage-visible names -------------------------------- */
void ref_synthesize_impl(LPCNetState *st, const float *features, short *output, int N, int preload)
{
    lpcnet_synthesize_impl(st, features, output, N, preload);   /* src/lpcnet.c:273 */
}

void ref_run_frame_network(LPCNetState *st, const float *features, float *cond_a, float *cond_b, float *lpc)
{
    run_frame_network(st, cond_a, cond_b, lpc, features);        /* src/lpcnet.c:82 */
}

/* the tail alone on frame products supplied by the caller (the counterpart of the engine's lpcnet_batch_run_tail and of the
 * oracle's orc_synthesize_tail): the products are put where run_frame_network leaves them, the loop is the reference's */
void ref_synthesize_tail(LPCNetState *st, const float *cond_a, const float *cond_b, const float *lpc,
                         short *output, int N, int preload)
{
    memcpy(st->gru_a_condition, cond_a, sizeof(st->gru_a_condition));
    memcpy(st->gru_b_condition, cond_b, sizeof(st->gru_b_condition));
    memcpy(st->lpc, lpc, sizeof(st->lpc));
    lpcnet_synthesize_tail_impl(st, output, N, preload);         /* src/lpcnet.c:235 */
}

int ref_run_sample_network(LPCNetState *st, const float *cond_a, const float *cond_b,
                           int last_exc, int last_sig, int pred)
{
    return run_sample_network(st, cond_a, cond_b, last_exc, last_sig, pred,
                              st->sampling_logit_table, &st->rng);  /* src/lpcnet.c:146 */
}

/* ---- layer-level known-answer hooks (use the model bound inside `st`) ----------------- */
void ref_gru_a_input(const LPCNetState *st, float *out, const float *cond, int sig, int pred, int exc)
{
    compute_gru_a_input(out, cond, GRU_A_STATE_SIZE, &st->model.gru_a_embed_sig, sig,
                        &st->model.gru_a_embed_pred, pred, &st->model.gru_a_embed_exc, exc);
}
void ref_sparse_gru_a(const LPCNetState *st, float *state, const float *input)
{
    compute_sparse_gru(&st->model.sparse_gru_a, state, input);
}
void ref_gru_b(const LPCNetState *st, const float *cond_b, float *state, const float *input)
{
    compute_gruB(&st->model.gru_b, cond_b, state, input);
}
int ref_sample_mdense(const LPCNetState *st, const float *input, unsigned *rng4)
{
    kiss99_ctx r; int v;
    r.z = rng4[0]; r.w = rng4[1]; r.jsr = rng4[2]; r.jcong = rng4[3];
    v = sample_mdense(&st->model.dual_fc, input, st->sampling_logit_table, &r);
    rng4[0] = r.z; rng4[1] = r.w; rng4[2] = r.jsr; rng4[3] = r.jcong;
    return v;
}
void ref_mdense_logits(const LPCNetState *st, float *out256, const float *input)
{
    compute_mdense(&st->model.dual_fc, out256, input);   /* SOFTMAX_HACK: sigmoid'ed outputs */
}

/* ---- scalar helpers ------------------------------------------------------------------ */
int   ref_lin2ulaw(float x)       { return lin2ulaw(x); }
float ref_ulaw2lin(float u)       { return ulaw2lin(u); }
float ref_tanh_approx(float x)    { float y; vec_tanh(&y, &x, 1); return y; }
float ref_sigmoid_approx(float x) { float y; vec_sigmoid(&y, &x, 1); return y; }
void  ref_vec_tanh(float *y, const float *x, int n)    { vec_tanh(y, x, n); }
void  ref_vec_sigmoid(float *y, const float *x, int n) { vec_sigmoid(y, x, n); }
float ref_lpc_from_cepstrum(float *lpc, const float *ceps) { return lpc_from_cepstrum(lpc, ceps); }
void  ref_lpc_weighting(float *lpc, float gamma) { lpc_weighting(lpc, gamma); }
void  ref_decode_packet(float *features4x36, float *vq_mem, const unsigned char *buf)
{
    decode_packet((float (*)[NB_TOTAL_FEATURES])features4x36, vq_mem, buf);
}

/* ---- packet-loss concealment: the state of an LPCNetPLCState (src/lpcnet_private.h:78-106), copied out field by field -------- */
LPCNetState    *ref_plc_lpcnet(LPCNetPLCState *st) { return &st->lpcnet; }
LPCNetEncState *ref_plc_enc(LPCNetPLCState *st)    { return &st->enc; }

/* widths of the PLC network's two GRU states as this build has them (generated plc_data.h) */
void ref_plc_net_units(int *g1, int *g2)
{
    *g1 = (int)(sizeof(((PLCNetState *)0)->plc_gru1_state)/sizeof(float));
    *g2 = (int)(sizeof(((PLCNetState *)0)->plc_gru2_state)/sizeof(float));
}

static float *put_net(float *out, const PLCNetState *n)
{
    memcpy(out, n->plc_gru1_state, sizeof(n->plc_gru1_state)); out += sizeof(n->plc_gru1_state)/sizeof(float);
    memcpy(out, n->plc_gru2_state, sizeof(n->plc_gru2_state)); out += sizeof(n->plc_gru2_state)/sizeof(float);
    return out;
}

/* ctl9 = {pcm_fill, skip_analysis, blend, loss_count, fec_fill_pos, fec_keep_pos, fec_read_pos, fec_skip, lpcnet.feature_buffer_fill};
 * any of the array arguments may be NULL.  net = plc_net, plc_copy[0..2], each gru1 then gru2 state; dc2 = {dc_mem, syn_dc} */
void ref_plc_get_state(const LPCNetPLCState *st, int *ctl9, short *pcm560, float *features20, float *net, double *dc2, float *fec100x20)
{
    int i;
    if (ctl9) {
        ctl9[0] = st->pcm_fill; ctl9[1] = st->skip_analysis; ctl9[2] = st->blend; ctl9[3] = st->loss_count;
        ctl9[4] = st->fec_fill_pos; ctl9[5] = st->fec_keep_pos; ctl9[6] = st->fec_read_pos; ctl9[7] = st->fec_skip;
        ctl9[8] = st->lpcnet.feature_buffer_fill;
    }
    if (pcm560) memcpy(pcm560, st->pcm, sizeof(st->pcm));
    if (features20) memcpy(features20, st->features, sizeof(float)*NB_FEATURES);
    if (net) {
        net = put_net(net, &st->plc_net);
        for (i=0;i<FEATURES_DELAY+1;i++) net = put_net(net, &st->plc_copy[i]);
    }
    if (dc2) { dc2[0] = st->dc_mem; dc2[1] = st->syn_dc; }
    if (fec100x20) memcpy(fec100x20, st->fec, sizeof(st->fec));
}

/* the members of LPCNetState that ref_get_nnet_state / ref_get_signal_state / ref_get_frame_products do not return */
void ref_get_deferred_state(const LPCNetState *st, float *old_lpc2x16, float *feature_buffer80)
{
    memcpy(old_lpc2x16, st->old_lpc, sizeof(st->old_lpc));
    memcpy(feature_buffer80, st->feature_buffer, sizeof(st->feature_buffer));
}

/* LPCNetEncState (src/lpcnet_private.h:55-75) in the order of the engine's analysis-state record: analysis_mem[160], mem_preemph, pcount,
 * pitch_mem[16], pitch_filt, exc_buf[576], pitch_max_path[0][0..224) (the rows the pitch search reads), pitch_max_path_all, best_i:
 * 981 four-byte cells.  Returns the number of bytes written (out == NULL: just the size). */
int ref_enc_get_state(const LPCNetEncState *st, void *out)
{
    char *p = (char *)out;
    const int paths = PITCH_MAX_PERIOD-PITCH_MIN_PERIOD;
    const int size = (int)(sizeof(st->analysis_mem) + sizeof(st->mem_preemph) + sizeof(st->pcount) + sizeof(st->pitch_mem) + sizeof(st->pitch_filt)
                     + sizeof(st->exc_buf) + sizeof(float)*paths + sizeof(st->pitch_max_path_all) + sizeof(st->best_i));
    if (!out) return size;
#define PUT(src, n) do { memcpy(p, src, n); p += n; } while (0)
    PUT(st->analysis_mem, sizeof(st->analysis_mem));
    PUT(&st->mem_preemph, sizeof(st->mem_preemph));
    PUT(&st->pcount, sizeof(st->pcount));
    PUT(st->pitch_mem, sizeof(st->pitch_mem));
    PUT(&st->pitch_filt, sizeof(st->pitch_filt));
    PUT(st->exc_buf, sizeof(st->exc_buf));
    PUT(st->pitch_max_path[0], sizeof(float)*paths);
    PUT(&st->pitch_max_path_all, sizeof(st->pitch_max_path_all));
    PUT(&st->best_i, sizeof(st->best_i));
#undef PUT
    return size;
}
