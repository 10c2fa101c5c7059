/* The one header that crosses from the C host shell into the HIP device runtime.
 * Plain C ABI: pointers, sizes and ints only.
 *
 * Layers:
 *   api.c (C)          public include/lpcnet.h + include/lpcnet_batch.h entry points
 *   model_pack.c (C)   DNNw blob -> validated host model + device-friendly packings
 *   engine*.hip (HIP)  device memory, uploads, kernel launches  <-- declared here (engine_core.h: what the units share)
 */
#ifndef LPCNET_ENGINE_H
#define LPCNET_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fixed architecture of the default model (what the reference's generated nnet_data.h
 *      hard-codes) ---------------------------------------------------- */
#define LPCN_N_A        384
#define LPCN_N_B        16
#define LPCN_COND       128
#define LPCN_NB_FEAT    20
#define LPCN_PITCH_EMB  64
#define LPCN_FRAME_IN   (LPCN_NB_FEAT + LPCN_PITCH_EMB)
#define LPCN_LPC_ORDER  16
#define LPCN_NB_BANDS   18
#define LPCN_FRAME_SIZE 160
#define LPCN_FEATURES_DELAY 2
#define LPCN_ROWS_A     (3 * LPCN_N_A)
#define LPCN_ROWS_B     (3 * LPCN_N_B)

/* ---- sample-kernel geometry --------------------------------------------------------------
 * One workgroup = 8 wavefronts = 512 lanes runs S interleaved streams.  GRU-A's recurrent rows
 * are dealt to lanes in "slots" of 64 rows (8 row-groups of the 8x4 block structure); each wave
 * owns up to LPCN_MAX_SLOTS slots and keeps their weights resident in VGPRs as `nw` items of
 * float4 (one item = the lane's row x one 4-wide input block). */
#define LPCN_WG_THREADS 512
#define LPCN_WAVES      8
#define LPCN_MAX_SLOTS  3
#define LPCN_EARLY_MAX  24     /* most items of a candidate slot that waves 4..7 may compute one sample ahead (float blobs) */
#define LPCN_DEAL_EH_F32 24    /* float blobs: head length of the early candidate items (round 4, matrix-pipe items: 20 / 22 / 24 -> 121.3 / 123.5 / 123.9 M samples/s) */
#define LPCN_DEAL_HW_I8 3      /* int8 blobs: first wave that may carry a candidate head (model_pack.c; 4 / 3 / 2 -> 153.4 / 156.2 / 154.1 M samples/s; round 5: superseded by the mask below) */
/* int8 blobs, PARITY, <= 2 streams per workgroup (two workgroups per CU -- the operating point of a full GPU): GRU-B's chain waves are
 * LPCN_I8_GBWA (stream 0) and LPCN_I8_GBWB (stream 1), NOT waves 0 and 1.  Waves w and w + 4 share a SIMD and wave 0 also leads the
 * streams (tree walk, LPC, mu-law: ~380 VALU instructions per sample that no other wave has); with GRU-B (~410 per stream) on waves
 * 0 / 1 as well, the SIMD of waves 0 / 4 issues 1.9 k VALU instructions per step against 1.2 k on the SIMDs of waves 2 / 6 and 3 / 7
 * (tools/valu_census.py --int8), and two co-resident workgroups are bound by the busiest SIMD (tools/ubench/hwid.hip: the second
 * workgroup's wave w lands one SIMD further than the first one's).  Every other wave is idle in GRU-B's phase and carries a
 * candidate head (LPCN_DEAL_HMASK_I8: bit w = wave w may), LPCN_DEAL_EH_I8 items long.  Measured (1024 streams, bit-exact):
 * waves 0,1 / 2,3 / 1,3 / 1,2 -> 157.6 / 163.3 / 160.7 / 160.1 M samples/s; head 10 / 14 / 16 / 18 / 20 / 22 / 24 items with 2,3 ->
 * 157.3 / 163.3 / 166.1 / 167.9 / 164.6 / 169.0 / 168.3 M (gpurun_out of round 5, two runs each within 0.2 M). */
#define LPCN_I8_GBWA 2
#define LPCN_I8_GBWB 3
#define LPCN_DEAL_HMASK_I8 (0xFFu & ~((1u << LPCN_I8_GBWA) | (1u << LPCN_I8_GBWB)))
#define LPCN_DEAL_EH_I8 22
/* the two-group float kernel (sample_kernel_x2.hip.h): GRU-B's chains -- one stream each -- run on waves 0 .. LPCN_X2_CHAIN_WAVES - 1; waves LPCN_X2_P0_FIRST .. 7
 * carry one candidate slot each (its head runs in the chains' shadow) and run the start-value pass, wave LPCN_X2_P0_FIRST also leads the streams; at most
 * LPCN_X2_NW_MAX register-resident items per lane */
#define LPCN_X2_CHAIN_WAVES 4
#define LPCN_X2_P0_FIRST 4
#define LPCN_X2_NW_MAX 32
/* ... its streamed variants (a batch's opt-in, lpcn_batch_dev_set_x2_streamed): up to LPCN_X2W_NW_MAX items per lane, of which the first LPCN_X2W_NR
 * are register-resident and the others come from L2 every sample (model_pack.c: lpcn_model_pack_x2_wide) */
#define LPCN_X2W_NW_MAX 96
#define LPCN_X2W_NR 24
/* the twelve-wave form of the two-group kernel (sample_kernel_x3.hip.h): three waves per SIMD, at most LPCN_X3_NW register-resident items per lane.
 * Waves 0 .. LPCN_X3_CHAIN_WAVES - 1 carry GRU-B's chains, the other eight the candidate heads and the start-value pass; every wave runs up to
 * LPCN_X3_SEGS row segments in P1.  Wave LPCN_X3_LW leads the streams; it and wave LPCN_X3_FREE carry no head (model_pack.c: lpcn_model_pack_x3). */
#define LPCN_X3_WAVES 12
#define LPCN_X3_THREADS (64 * LPCN_X3_WAVES)
#define LPCN_X3_CHAIN_WAVES 4
#define LPCN_X3_NW 16
#define LPCN_X3_SEGS 4
#define LPCN_X3_LW 4
#define LPCN_X3_FREE 9
#define LPCN_DEAL_EH_FAST_I8 0 /* head length of the FAST arithmetic's own image of int8 blobs (model_pack.c: lpcn_model_pack_fast) */

/* ---- the packet-loss concealment's own network (compute_plc_pred, src/lpcnet_plc.c:135-146): dense 57 -> d1 tanh, GRU d1 -> g1,
 * GRU g1 -> g2, dense g2 -> 20 linear, bound by name like the reference's init_plc_model.  The widths are read from the bias lengths. */
#define LPCN_PLC_IN       (2 * LPCN_NB_BANDS + LPCN_NB_FEAT + 1)
#define LPCN_PLC_MAX_UNITS 512
#define LPCN_PLC_MAX_FEC   100      /* PLC_MAX_FEC, src/lpcnet_private.h:25 */
#define LPCN_PLC_BUF_SIZE  (LPCN_FEATURES_DELAY * LPCN_FRAME_SIZE + 80)      /* PLC_BUF_SIZE, src/lpcnet_private.h:77 */
#define LPCN_PLC_QUEUE     (LPCN_PLC_BUF_SIZE + LPCN_FRAME_SIZE)
#define LPCN_PLC_FBUF      4        /* MAX_FEATURE_BUFFER_SIZE, src/lpcnet_private.h:26 */
/* One layer of a frame-rate network as the blob has it (pointers into the blob): what the PLC network and the DRED decoder are built from.  The widths
 * are read from the bias lengths; `idx` is the index stream {count, pos...} per 8-row group (src/vec.h:347-360), `nb` its 8x4 blocks.  An int8 (DOT_PROD)
 * GRU has signed char behind `w` and `rec`: blocks [nb][8][4] and [3 n / 8][n / 4][8][4]. */
typedef struct lpcn_dense_layer { const float *w, *b; int n_in, n_out; } lpcn_dense_layer;                      /* [n_in][n_out], [n_out] */
typedef struct lpcn_gru_layer { const float *w, *rec, *bias; const int *idx; int n_in, n, nb; } lpcn_gru_layer;  /* blocks [nb][4][8], [n][3 n], [2][3 n] */
typedef struct lpcn_plc_model {
    int present;                 /* 0: the blob has no plc_* arrays; 1: float arrays; 2: int8 arrays (DOT_PROD GRUs); -1: incomplete or
                                  * inconsistent arrays.  Served in the blob's own flavour only (lpcn_plc_servable) */
    lpcn_dense_layer dense1;     /* [57][d1], tanh */
    lpcn_gru_layer gru[2];       /* d1 -> g1, g1 -> g2 */
    lpcn_dense_layer out;        /* [g2][20], linear */
} lpcn_plc_model;

/* ---- the DRED decoder of the same blob (DRED_rdovae_decode_all, src/dred_rdovae.c:38-52; src/dred_rdovae_dec.c:37-98): three dense layers that turn the
 * initial state into the GRU states, then per latent dense 1 -> GRU 2 -> dense 3 -> GRU 4 -> dense 5 -> GRU 6 -> dense 7 -> dense 8, every output appended
 * to one buffer, and a linear layer over the whole buffer that gives four 20-float frames.  Bound by the names torch/rdovae/export_rdovae_weights.py and
 * training_tf2/dump_rdovae.py emit; the widths are read from the bias lengths, the latent and state dimensions from the first matrices. */
#define LPCN_DRED_MAX_UNITS 256      /* most units of a layer, and most inputs of the first layers (latent, initial state) */
#define LPCN_DRED_FRAMES    4        /* frames per latent */
#define LPCN_DRED_OUT       (LPCN_DRED_FRAMES * LPCN_NB_FEAT)
typedef struct lpcn_dred_model {
    int present;                 /* 0: the blob has none of the decoder's arrays; 1: float arrays; 2: int8 GRU arrays (DOT_PROD); -1: incomplete or inconsistent */
    int latent_dim, state_dim;
    int width[8];                /* dec_dense1 .. dec_dense8 */
    lpcn_dense_layer state[3];    /* state1 .. state3: tanh */
    lpcn_dense_layer dense[5];    /* dec_dense1, 3, 5, 7, 8: tanh */
    lpcn_gru_layer gru[3];        /* dec_dense2, 4, 6 */
    lpcn_dense_layer final;       /* dec_final: [sum of the widths][80], linear */
} lpcn_dred_model;

/* ---- the DRED encoder of the same blob (DRED_rdovae_encode_dframe, src/dred_rdovae.c:102-105; src/dred_rdovae_enc.c:38-95): per double frame (two 20-float
 * feature frames, 40 inputs) dense 1 -> GRU 2 -> dense 3 -> GRU 4 -> dense 5 -> GRU 6 -> dense 7 -> dense 8, every output appended to one buffer; the
 * latents are the conv1d bits_dense over the last `taps` buffers (linear), the initial state is gdense2(gdense1(buffer)), both tanh.  The widths are read
 * from the bias lengths, the taps from bits_dense_weights: [taps * sum of the widths][latent], oldest tap first. */
#define LPCN_DRED_ENC_IN       (2 * LPCN_NB_FEAT)
#define LPCN_DRED_ENC_MAX_TAPS 8
typedef struct lpcn_dred_enc_model {
    int present;                 /* 0: the blob has none of the encoder's arrays; 1: float arrays; 2: int8 GRU arrays (DOT_PROD); -1: incomplete or inconsistent */
    int latent_dim, state_dim, taps, gdense1;
    int width[8];                /* enc_dense1 .. enc_dense8 */
    lpcn_dense_layer dense[5];    /* enc_dense1, 3, 5, 7, 8: tanh */
    lpcn_gru_layer gru[3];        /* enc_dense2, 4, 6 */
    lpcn_dense_layer bits;        /* bits_dense: [taps * sum of the widths][latent], linear */
    lpcn_dense_layer gdense[2];   /* gdense1: [sum of the widths][gdense1], gdense2: [gdense1][state], tanh */
} lpcn_dred_enc_model;

typedef struct lpcn_model_host {
    int is_int8;                 /* blob flavour: 0 = float qweights (DISABLE_DOT_PROD), 1 = int8 (DOT_PROD)  */
    int b_dense;                 /* GRU-B input matrix lists every input block for every row group */
    int nb_a, nb_b;              /* 8x4 blocks in GRU-A recurrent / GRU-B input matrices       */
    int nw;                      /* items per lane needed by the register-resident packing     */
    int nb_b_padded;             /* GRU-B blocks after padding every row group to a multiple of 4 */
    float lpc_gamma;

    /* plain arrays (pointers into the caller's blob, reference layouts) */
    const float *emb_sig, *emb_pred, *emb_exc;      /* [256][1152]                             */
    const float *a_dense_w, *a_dense_b;             /* [128][1152], [1152]                     */
    const float *b_dense_w, *b_dense_b;             /* [128][48], [48]                         */
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b;
    const float *pitch_emb;                         /* [256][64]                               */
    const float *dense1_w, *dense1_b, *dense2_w, *dense2_b;
    const float *fc_w, *fc_b, *fc_f;                /* [256][2][16], [2][256], [2][256]        */
    const float *a_bias, *a_diag;                   /* [2][1152], [1152]                       */
    const float *a_w; const int *a_idx;             /* float blocks [in4][out8] + index stream */
    const float *b_bias;                            /* [2][48]                                 */
    const float *b_w; const int *b_idx;
    const float *b_rec;                             /* [16][48]                                */

    /* device-oriented packings built by lpcn_model_pack() (malloc'ed, owned by the model)     */
    float   *pk_a_w;      /* [8 waves][nw][64 lanes][4]     row weights per item (float blobs)  */
    int32_t *pk_a_wq;     /* [8 waves][nw][64 lanes]        4 int8 row weights per item (int8)  */
    int32_t *pk_b_wq;     /* [blk/4][row-in-group 8][blk%4] 4 int8 per row and block (int8)     */
    uint8_t *pk_a_blk;    /* [8][nw][64]                    input block index p = pos/4        */
    int32_t *pk_a_row;    /* [8][3 slots][64]               GRU-A row (0..1151) or -1          */
    int32_t  pk_a_bound[LPCN_WAVES][LPCN_MAX_SLOTS + 1];    /* item index where each slot starts */
    int32_t  pk_a_allh[LPCN_WAVES][LPCN_MAX_SLOTS];        /* 1 if every live row of the slot is a candidate-state row */
    int32_t  pk_a_head[LPCN_WAVES];   /* float blobs: chain items [0, head) of slot 0's rows sit at items [nw - head, nw) (computed one sample ahead) */
    float   *pk_b_w;      /* GRU-B input weights re-blocked [blk][row-in-group 8][k 4] per group */
    int32_t *pk_b_start;  /* [6 groups + 1] first block of each group in pk_b_w                */
    uint8_t *pk_b_blk;    /* [nb_b] input block index per block                                */
    float   *pk_emb[3];   /* sig/pred/exc tables re-ordered to [256][3 slots][512 threads] */
    lpcn_plc_model plc;   /* the PLC network of the same blob, when it has one (pointers into the blob) */
    lpcn_dred_model dred; /* the DRED decoder of the same blob, when it has one (pointers into the blob) */
    lpcn_dred_enc_model dred_enc;   /* the DRED encoder of the same blob, when it has one (pointers into the blob) */
} lpcn_model_host;

/* GRU-A dealt to the twelve waves of sample_kernel_x3 (float blobs).  A wave holds LPCN_X3_NW items per lane: segment 0 -- the HEAD of a candidate
 * slot (its first blocks, summed onto bias + diag*h one sample ahead and parked in the rows' pre-activation cells; a slot of <= LPCN_X3_NW items
 * is WHOLE there) -- END-ALIGNED at items [LPCN_X3_NW - count, LPCN_X3_NW), and segments 1 .. LPCN_X3_SEGS, run in P1 from the value the rows' cells hold
 * (WHOLE update / reset slots: the start value; the TAIL of a candidate slot: its head's partial sums), at items [first, first + count). */
enum { LPCN_X3_NONE = 0, LPCN_X3_WHOLE = 1, LPCN_X3_HEAD = 2, LPCN_X3_TAIL = 3 };
typedef struct lpcn_x3_image {
    float   *w;                                             /* [12 waves][16 items][64 lanes][4] */
    uint8_t *blk;                                           /* [12][16][64] input block of the item */
    int32_t  row[LPCN_X3_WAVES][1 + LPCN_X3_SEGS][64];      /* GRU-A row of the lane in the segment, or -1 */
    int32_t  kind[LPCN_X3_WAVES][1 + LPCN_X3_SEGS];
    int32_t  first[LPCN_X3_WAVES][1 + LPCN_X3_SEGS];        /* first item of the segment */
    int32_t  count[LPCN_X3_WAVES][1 + LPCN_X3_SEGS];        /* its items */
    int32_t  skip[LPCN_X3_WAVES][1 + LPCN_X3_SEGS];         /* blocks of its rows that another segment sums first (TAIL: the head's length) */
} lpcn_x3_image;

/* model_pack.c -------------------------------------------------------------------------------
 * Parse + validate a DNNw blob exactly like the reference loader does
 * (src/parse_lpcnet_weights.c:53-113, :124-220) and build the packings.  Returns 0, or -1 on a
 * malformed / incomplete blob (same condition under which lpcnet_load_model returns -1). */
int  lpcn_model_parse(lpcn_model_host *m, const unsigned char *blob, int len);
void lpcn_model_release(lpcn_model_host *m);
int  lpcn_model_pack_x2(const lpcn_model_host *m, lpcn_model_host *f);     /* 0: f holds the two-group kernel's own GRU-A packing; -1: the model does not fit it */
int  lpcn_model_pack_x2_wide(const lpcn_model_host *m, lpcn_model_host *f); /* the same for LPCN_X2_NW_MAX < items per lane <= LPCN_X2W_NW_MAX (the streamed variants); -1: int8, fewer, more */
int  lpcn_model_pack_fast(const lpcn_model_host *m, lpcn_model_host *f);   /* 1: FAST shares PARITY's image; 0: f holds FAST's own GRU-A packing */
int  lpcn_model_pack_x3(const lpcn_model_host *m, lpcn_x3_image *im);      /* 0: im holds the twelve-wave image; -1: the model does not fit it (not an error: the other kernels run it) */
void lpcn_x3_image_release(lpcn_x3_image *im);
int  lpcn_x3_image_selftest(const lpcn_model_host *m, const lpcn_x3_image *im);      /* 0 = every block of GRU-A exactly once, in its row's order, within the bounds */
/* re-expand the packings and compare them with the blob (0 = consistent) */
int  lpcn_model_selftest(const lpcn_model_host *m);
int  lpcn_plc_servable(const lpcn_model_host *m);                           /* 1: the blob's PLC network is in the blob's own flavour (float / int8) */
int  lpcn_dred_servable(const lpcn_model_host *m);                          /* 1: the blob's DRED decoder is float beside a float LPCNet model */
int  lpcn_dred_enc_servable(const lpcn_model_host *m);                      /* 1: the blob's DRED encoder is float beside a float LPCNet model */
void lpcn_plc_pack_rec_i8(const signed char *rec, int N, int32_t *out);     /* int8 recurrent weights of a PLC GRU, one dword per (row, block): out [N / 4][3 N] */

/* ---- per-stream state as the device keeps it (AoS, one record per stream) ------------------ */
typedef struct lpcn_stream_state {
    float gru_a[LPCN_N_A];
    float gru_b[LPCN_N_B];
    float conv1_mem[2 * LPCN_FRAME_IN];
    float conv2_mem[2 * LPCN_COND];
    float old_lpc[LPCN_FEATURES_DELAY][LPCN_LPC_ORDER];
    float last_sig[LPCN_LPC_ORDER];
    float deemph_mem;
    int32_t last_exc;
    int32_t frame_count;
    uint32_t rng[4];
    float lpc[LPCN_LPC_ORDER];          /* products of the most recent frame (for export)       */
    int32_t pad[3];
} lpcn_stream_state;

/* ---- per-stream ANALYSIS state (feature extraction, analysis_kernels.hip.h): the fields of the reference's LPCNetEncState
 * (src/lpcnet_private.h:55-75) that lpcnet_compute_single_frame_features reads or writes, in the reference's order; all zero after
 * lpcnet_encoder_init.  Separate from the synthesis state, as LPCNetEncState is from LPCNetState.  The encoder (encode_kernels.hip.h)
 * works on this same record; its vq_mem lives in an array of its own and xc[0..1] / frame_weight[0..1] are read by no path, so the
 * record does not grow. */
#define LPCN_AN_OVERLAP         160
#define LPCN_AN_TRAINING_OFFSET 80
#define LPCN_PITCH_MIN_PERIOD   32
#define LPCN_PITCH_MAX_PERIOD   256
#define LPCN_PITCH_BUF_SIZE     (LPCN_PITCH_MAX_PERIOD + 320)
#define LPCN_AN_NB_FEATURES     36
typedef struct lpcn_analysis_state {
    float analysis_mem[LPCN_AN_OVERLAP];    /* the last 160 pre-emphasised input samples                                       */
    float mem_preemph;                      /* -0.85f * the last raw input sample                                              */
    int32_t pcount;                         /* always 0 in single-frame analysis                                               */
    float pitch_mem[LPCN_LPC_ORDER];        /* = analysis_mem[79 - j]: kept for the layout, the kernels read analysis_mem      */
    float pitch_filt;                       /* LPC residual of the last sample before the one-tap filter                       */
    float exc_buf[LPCN_PITCH_BUF_SIZE];     /* [0, 416) live: the last 416 excitation samples; the rest stays zero             */
    float pitch_max_path[LPCN_PITCH_MAX_PERIOD - LPCN_PITCH_MIN_PERIOD];
    float pitch_max_path_all;
    int32_t best_i;
} lpcn_analysis_state;

/* ---- engine*.hip ---------------------------------------------------------------------------- */
typedef struct lpcn_engine lpcn_engine;      /* one per (process, HIP device, model)            */

/* All functions return 0 on success or a negative LPCN_E_* code; the message of the last failure
 * on the calling thread is available from lpcn_last_error(). */
#define LPCN_E_NODEVICE  (-2)
#define LPCN_E_HIP       (-3)
#define LPCN_E_ARG       (-4)
#define LPCN_E_MODEL     (-5)
const char *lpcn_last_error(void);

int  lpcn_engine_create(lpcn_engine **out, int device, const lpcn_model_host *m);
void lpcn_engine_destroy(lpcn_engine *e);
int  lpcn_engine_device(const lpcn_engine *e);

/* Device buffers for a set of n streams processed together. */
typedef struct lpcn_batch_dev lpcn_batch_dev;
int  lpcn_batch_dev_create(lpcn_batch_dev **out, lpcn_engine *e, int n_streams, int max_chunk_frames);
void lpcn_batch_dev_destroy(lpcn_batch_dev *b);
int  lpcn_batch_dev_reset(lpcn_batch_dev *b, int first, int count);           /* lpcnet_reset   */
/* The active prefix (include/lpcnet_batch.h: lpcnet_batch_set_active): every call that advances streams works on streams [0, active) of the batch;
 * the arrays keep their [n_streams][...] layout and the rows of the other streams are neither read nor written.  Host-only, no wait. */
int  lpcn_batch_dev_set_active(lpcn_batch_dev *b, int active);                /* 0 .. n_streams (the default) */
int  lpcn_batch_dev_active(const lpcn_batch_dev *b);
/* Stream src[i] -> stream dst[i], i < m, on the device: everything the batch keeps per stream that is allocated now (engine_roster.hip).  One upload
 * of the pair list and one launch, enqueued on hip_stream (NULL = the engine's own; not a capturing one); the host halves (the PLC's control state,
 * the kept products' flag) are copied now.  The lists must be valid (api_roster.h: roster_check): this function checks the range only. */
int  lpcn_batch_dev_copy_streams(lpcn_batch_dev *b, const int *src, const int *dst, int m, void *hip_stream);
/* Stream snapshots (include/lpcnet_batch.h: lpcnet_batch_snapshot; engine_snapshot.hip, snapshot_plan.h).  A layout is LPCNET_SNAP_LAYOUT_INTS ints at
 * most; snapshot_layout writes the batch's present one (model hash 0: the shell knows it) and returns its ints.  snapshot / restore: one upload of the
 * list and one launch, enqueued on hip_stream (NULL = the engine's own; not a capturing one); they check the list (inside the capacity, distinct), meta
 * [m][LPCNET_SNAP_META] is a host array written / read before the call returns, d_records is 16-byte aligned.  restore refuses a layout that does not
 * match with nothing allocated (LPCN_E_MODEL); snapshot_match is that check alone (0, 1 = fits once snapshot_enable has allocated the subsystems only
 * the snapshot has, LPCN_E_MODEL).  The _host forms move records [.][record bytes] and meta rows of a blob: entry j of the list is record pos[j]
 * (NULL: j); they synchronise.  copy_streams_to: gather, transfer, scatter between two batches, only enqueued. */
int  lpcn_batch_dev_snapshot_layout(const lpcn_batch_dev *b, int *layout);
int  lpcn_batch_dev_snapshot(lpcn_batch_dev *b, const int *streams, int m, void *d_records, int *meta, void *hip_stream);
int  lpcn_batch_dev_restore(lpcn_batch_dev *b, const int *streams, int m, const void *d_records, const int *meta, const int *layout, void *hip_stream);
int  lpcn_batch_dev_snapshot_match(const lpcn_batch_dev *b, const int *layout, int enqueue_only);
int  lpcn_batch_dev_snapshot_enable(lpcn_batch_dev *b, const int *layout);
int  lpcn_batch_dev_snapshot_host(lpcn_batch_dev *b, const int *streams, const int *pos, int m, void *records, int *meta);
int  lpcn_batch_dev_restore_host(lpcn_batch_dev *b, const int *streams, const int *pos, int m, const void *records, const int *meta, const int *layout);
int  lpcn_batch_dev_copy_streams_to(lpcn_batch_dev *from, const int *src, lpcn_batch_dev *to, const int *dst, int m);
int  lpcn_batch_dev_get_decoder_vq_mem(lpcn_batch_dev *b, int stream, float *out18);
int  lpcn_batch_dev_set_decoder_vq_mem(lpcn_batch_dev *b, int stream, const float *in18);
int  lpcn_batch_dev_get_state(lpcn_batch_dev *b, int stream, lpcn_stream_state *host);
/* k independent streams with their callers' POD states in ONE pass and one synchronisation (engine_synth.hip): frame network + samples,
 * samples from the callers' frame products, or the frame network alone */
#define LPCN_GROUP_FRAMES        0
#define LPCN_GROUP_FRAME_SAMPLES 1
#define LPCN_GROUP_TAIL          2
int  lpcn_batch_dev_run_group(lpcn_batch_dev *b, int k, int kind, int frame_len, int preload, const lpcn_stream_state *const *st_in,
                              const float *const *feat, short *const *pcm, lpcn_stream_state *const *st_out,
                              float *const *ga, float *const *gb, float *const *lpc);
int  lpcn_batch_dev_tune(lpcn_batch_dev *b);              /* measure the streams per workgroup now, on the engine's own stream */
int  lpcn_batch_dev_set_state(lpcn_batch_dev *b, int stream, const lpcn_stream_state *host);
int  lpcn_batch_dev_streams_per_wg(const lpcn_batch_dev *b);
int  lpcn_batch_dev_set_streams_per_wg(lpcn_batch_dev *b, int s);              /* 1,2,4 (0=auto) */
int  lpcn_batch_dev_set_x2_streamed(lpcn_batch_dev *b, int on);                /* the two-group kernel's streamed variants for this batch (33 .. 96 items per lane); 0 also where the model has the ordinary image */
int  lpcn_batch_dev_x2_streamed(const lpcn_batch_dev *b);
int  lpcn_batch_dev_set_x2_fast(lpcn_batch_dev *b, int on);                    /* the two-group kernel under FAST fp32 arithmetic for this batch (ordinary two-group image only; LPCN_E_MODEL otherwise) */
int  lpcn_batch_dev_x2_fast(const lpcn_batch_dev *b);
int  lpcn_batch_dev_set_x3(lpcn_batch_dev *b, int mode);                       /* twelve-wave form of the two-group kernel: 0 never, 1 always (needs the image), -1 measured / table */
int  lpcn_batch_dev_x3(const lpcn_batch_dev *b);                                /* what a whole-batch launch runs now */
int  lpcn_batch_dev_retune(lpcn_batch_dev *b);                                 /* after lpcn_engine_set_fast: auto value again */

/* Run n_frames frames (frame network + LPC + 160-sample loop each) for every stream.
 *   features : [n_streams][n_frames][feat_stride] floats, only [0..19] of each frame are read
 *   pcm      : [n_streams][n_frames*160] int16
 *   preload  : teacher forcing, 0..160 leading samples of every frame are taken from pcm
 *              (semantics of lpcnet_synthesize_impl, src/lpcnet.c:256-259)
 * *_dev variants take device pointers and only enqueue work on `hip_stream` (NULL = the
 * engine's own stream); the host variant copies in/out and synchronises. */
int  lpcn_batch_dev_run(lpcn_batch_dev *b, const float *d_features, int feat_stride,
                        short *d_pcm, int n_frames, int preload, void *hip_stream);
int  lpcn_batch_dev_run_host(lpcn_batch_dev *b, const float *features, int feat_stride,
                             short *pcm, int n_frames, int preload);
int  lpcn_batch_dev_sync(lpcn_batch_dev *b);
/* Legacy per-frame API on a batch of ONE stream: one frame-network step on feat[0..19] + frame_len samples with a single
 * host synchronisation.  st_in == NULL: the device copy of the state is current (no upload); st_out receives the new state. */
int  lpcn_batch_dev_run_single(lpcn_batch_dev *b, const lpcn_stream_state *st_in, const float *feat, short *pcm,
                               lpcn_stream_state *st_out);

/* Codec path (src/lpcnet_dec.c:81-155 on the device): packets [n][n_packets][8] -> pcm [n][n_packets*640].
 * The VQ memory of every stream lives on the device and is cleared by lpcn_batch_dev_reset. */
int  lpcn_engine_set_codebooks(lpcn_engine *e, const float *cb1, const float *cb2, const float *cb3, const float *cb_diff4);
int  lpcn_engine_has_codebooks(const lpcn_engine *e);
int  lpcn_engine_set_end2end(lpcn_engine *e, int on);              /* END2END of the model's nnet_data.h (default off) */
int  lpcn_engine_set_lpc_gamma(lpcn_engine *e, float gamma);     /* LPC_GAMMA of the model's nnet_data.h (default 1) */
int  lpcn_engine_set_fast(lpcn_engine *e, int on);                /* FAST arithmetic (not bit-exact; default off = PARITY) */
int  lpcn_batch_dev_decode(lpcn_batch_dev *b, const unsigned char *d_packets, short *d_pcm, int n_packets, void *hip_stream);
int  lpcn_batch_dev_decode_host(lpcn_batch_dev *b, const unsigned char *packets, short *pcm, int n_packets);
/* Parity seam: the unpacker alone (host pointers): packets [n][n_packets][8] -> features [n][4 n_packets][20].  Advances the VQ memory only. */
int  lpcn_batch_dev_run_decode_host(lpcn_batch_dev *b, const unsigned char *packets, float *features, int n_packets);

/* Parity seam (SURVEY.md §7 hard part 9): run only the sample loop with caller-provided frame
 * products (host pointers): cond_a [n][f][1152], cond_b [n][f][48], lpc [n][f][16]. */
int  lpcn_batch_dev_run_tail_host(lpcn_batch_dev *b, const float *cond_a, const float *cond_b,
                                  const float *lpc, short *pcm, int n_frames, int preload);
/* Frame network + LPC only (host pointers); outputs like above (any may be NULL). */
int  lpcn_batch_dev_run_frames_host(lpcn_batch_dev *b, const float *features, int feat_stride,
                                    float *cond_a, float *cond_b, float *lpc, int n_frames);

/* One frame step with per-stream arguments (host pointers, see engine_plc.hip): mode[s] 0 = skip, 1 = frame network + n_samples[s]
 * samples, 2 = n_samples[s] samples from the stream's most recent frame products; preload[s] leading samples of pcm[s] imposed.
 * features [n][feat_stride], pcm [n][160]. */
int  lpcn_batch_dev_step_host(lpcn_batch_dev *b, const float *features, int feat_stride, short *pcm,
                              const int *n_samples, const int *preload, const int *mode);

/* Feature analysis (lpcnet_compute_single_frame_features per stream and frame, analysis_kernels.hip.h):
 *   pcm [n_streams][n_frames*160] shorts (pcm_is_float = 0) or floats -> features [n_streams][n_frames][feat_stride >= 36], floats 0..35.
 * The analysis state and the kernels' scratch are allocated by lpcn_batch_dev_analysis_enable (max_frames = the longest call that
 * must not allocate: longer calls grow the scratch) or by the first call; a call on a stream that is being captured allocates nothing
 * and returns LPCN_E_ARG when something is missing.  lpcn_batch_dev_reset does not touch the analysis state. */
int  lpcn_batch_dev_analysis_enable(lpcn_batch_dev *b, int max_frames);
int  lpcn_batch_dev_analyze(lpcn_batch_dev *b, const void *d_pcm, int pcm_is_float, float *d_features, int feat_stride, int n_frames,
                            void *hip_stream);
int  lpcn_batch_dev_analyze_host(lpcn_batch_dev *b, const void *pcm, int pcm_is_float, float *features, int feat_stride, int n_frames);
int  lpcn_batch_dev_analysis_reset(lpcn_batch_dev *b, int first, int count);      /* lpcnet_encoder_init */
int  lpcn_batch_dev_get_analysis_state(lpcn_batch_dev *b, int stream, lpcn_analysis_state *host);
int  lpcn_batch_dev_set_analysis_state(lpcn_batch_dev *b, int stream, const lpcn_analysis_state *host);

/* Encoder (lpcnet_encode / lpcnet_compute_features per stream and packet, encode_kernels.hip.h): pcm [n_streams][n_packets*640] shorts ->
 * packets [n_streams][n_packets][8], or features [n_streams][n_packets*4][feat_stride >= 36].  Both act on the analysis state above; the
 * encoder's one further carried field, vq_mem[18], is a device array of its own ([n_streams][18], zero on allocation, cleared by
 * lpcn_batch_dev_analysis_reset where it exists).  lpcn_batch_dev_encoder_enable allocates it, the analysis state and the scratch for calls
 * of up to max_packets packets; capture rules as for the analysis.  _host: packets != NULL encodes, else features are computed. */
int  lpcn_batch_dev_encoder_enable(lpcn_batch_dev *b, int max_packets);
int  lpcn_batch_dev_encode(lpcn_batch_dev *b, const short *d_pcm, unsigned char *d_packets, int n_packets, void *hip_stream);
int  lpcn_batch_dev_compute_features(lpcn_batch_dev *b, const short *d_pcm, float *d_features, int feat_stride, int n_packets, void *hip_stream);
int  lpcn_batch_dev_encode_host(lpcn_batch_dev *b, const short *pcm, unsigned char *packets, float *features, int feat_stride, int n_packets);
int  lpcn_batch_dev_get_encoder_vq_mem(lpcn_batch_dev *b, int stream, float *out18);
int  lpcn_batch_dev_set_encoder_vq_mem(lpcn_batch_dev *b, int stream, const float *in18);

/* Packet-loss concealment (lpcnet_plc_update / lpcnet_plc_conceal in causal mode per stream, plc_kernels.hip.h).
 * The control state of a stream -- everything src/lpcnet_plc.c:188-340 branches on -- is a function of the loss flags and the FEC calls
 * alone and lives on the host; samples, features and network states live on the device. */
typedef struct lpcn_plc_ctl {
    int32_t pcm_fill, skip_analysis, blend, loss_count;      /* LPCNetPLCState, src/lpcnet_private.h:79-105 */
    int32_t fec_fill, fec_keep, fec_read, fec_skip;
    int32_t fbuf_fill;                                        /* feature_buffer_fill of the stream's LPCNetState */
} lpcn_plc_ctl;
/* one stream's PLC state as lpcnet_batch_get_plc_state / _set_plc_state carry it: both halves, and the frame products of the synthesis state */
typedef struct lpcn_plc_state_rec {
    lpcn_plc_ctl ctl;
    int32_t g1, g2, delta;
    double dc[2];                                             /* dc_mem, syn_dc */
    short q[LPCN_PLC_QUEUE];
    float feat[LPCN_NB_FEAT];
    float net[4][2 * LPCN_PLC_MAX_UNITS];                     /* plc_net, plc_copy[0..2]: g1 + g2 floats each */
    float fec[LPCN_PLC_MAX_FEC][LPCN_NB_FEAT];
    float fbuf[LPCN_PLC_FBUF][LPCN_NB_FEAT];
    float keep_a[LPCN_ROWS_A], keep_b[LPCN_ROWS_B], keep_lpc[LPCN_LPC_ORDER];
} lpcn_plc_state_rec;
#define LPCN_PLC_SUMMARY 10
/* The planner alone, without a device: advances ctl[0..n) by one step with the given loss flags and writes per stream
 * {lost, flushed queue entries, queue rounds, their samples, FEC vectors used, first frame after a loss (1 cross-fade, 2 codec restore),
 *  queue operation (1 tail, 2 append, 3 push and shift), prediction kept on a received frame, deferred features appended, loss_count after}. */
int  lpcn_plc_plan(int options, int n, lpcn_plc_ctl *ctl, const unsigned char *lost, int *summary);
/* ... with lanes (plc_plan.cpp): launch [.][10] and the control lists out; returns the number of launches, or LPCN_E_ARG with the message in err */
int  lpcn_plc_plan_lanes(int options, int n, int lanes, lpcn_plc_ctl *ctl, const unsigned char *lost, int *summary, int *launch, int launch_cap,
                         int *lists, int lists_cap, char *err, size_t err_len);
/* The group schedule of a batch (include/lpcnet_batch.h: lpcnet_batch_set_group_schedule): form 0 / 1, lanes 1 .. 4 */
int  lpcn_batch_dev_set_group_schedule(lpcn_batch_dev *b, int form, int lanes);
int  lpcn_batch_dev_get_group_schedule(const lpcn_batch_dev *b, int *form, int *lanes);
int  lpcn_batch_dev_group_form(const lpcn_batch_dev *b, int cnt);             /* streams per workgroup of a group of cnt streams */
int  lpcn_batch_dev_last_groups(const lpcn_batch_dev *b, int *rec, int cap);  /* [.][8] of the most recent PLC / per-stream step; returns their number */
void lpcn_plc_ctl_reset(lpcn_plc_ctl *c);
int  lpcn_plc_ctl_fec_add(lpcn_plc_ctl *c, int is_null);     /* host half of lpcnet_plc_fec_add: 0 stored / skipped, 1 dropped (ring full), 2 stored after a compaction */
int  lpcn_engine_plc_present(const lpcn_engine *e);           /* lpcn_plc_model.present of the engine's blob */
int  lpcn_batch_dev_plc_enable(lpcn_batch_dev *b, int options);
int  lpcn_batch_dev_plc_enabled(const lpcn_batch_dev *b);
int  lpcn_batch_dev_plc_flavour(const lpcn_batch_dev *b);     /* 0 float network, 1 int8; LPCN_E_MODEL before plc_enable */
int  lpcn_batch_dev_plc_reset(lpcn_batch_dev *b, int first, int count);
int  lpcn_batch_dev_plc_step(lpcn_batch_dev *b, short *d_pcm, const unsigned char *lost, void *hip_stream);      /* enqueue only; lost is a host array */
int  lpcn_batch_dev_plc_step_host(lpcn_batch_dev *b, short *pcm, const unsigned char *lost);
int  lpcn_batch_dev_plc_fec_add(lpcn_batch_dev *b, int stream, const float *features20);
int  lpcn_batch_dev_plc_fec_clear(lpcn_batch_dev *b, int stream);
/* every stream's FEC traffic in one call: clear[s], then skip[s] NULL adds, then count[s] vectors of the packed [sum(count)][20] features (host arrays
 * [n]; skip, clear, dropped may be NULL).  0, or 1 when vectors were dropped (dropped[s]: how many, the tail of the stream's list).  The device form only
 * enqueues (not on a capturing stream); _plan is the planner alone: ctl in and out, rec [n][8] out, returns the number of records. */
int  lpcn_batch_dev_plc_fec_feed(lpcn_batch_dev *b, const float *d_features, const int *count, const int *skip, const unsigned char *clear, int *dropped, void *hip_stream);
int  lpcn_batch_dev_plc_fec_feed_host(lpcn_batch_dev *b, const float *features, const int *count, const int *skip, const unsigned char *clear, int *dropped);
int  lpcn_plc_fec_feed_plan(int n, lpcn_plc_ctl *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped);
int  lpcn_batch_dev_get_plc_state(lpcn_batch_dev *b, int stream, lpcn_plc_state_rec *host);
int  lpcn_batch_dev_set_plc_state(lpcn_batch_dev *b, int stream, const lpcn_plc_state_rec *host);
int  lpcn_batch_dev_plc_burg_host(lpcn_batch_dev *b, const float *x, float *ceps36);
int  lpcn_batch_dev_plc_pred_host(lpcn_batch_dev *b, const float *in57, float *out20);
/* Records per workgroup of the prediction kernels (plc_kernels.hip.h: plc_pred_kernel at 1, plc_pred_s_kernel<S> at 2, 4, 8; the output bits are the
 * same in every form).  set_form pins it (0 = the table's choice); form: what a launch over n records runs with -- the pinned or the table's value,
 * halved until its LDS fits.  lpcn_plc_pred_form is that rule alone (plc_plan.cpp, no device): LPCN_E_ARG for a pinned value other than 0, 1, 2, 4, 8. */
int  lpcn_batch_dev_plc_pred_set_form(lpcn_batch_dev *b, int S);
int  lpcn_batch_dev_plc_pred_form(const lpcn_batch_dev *b, int n);
int  lpcn_plc_pred_form(int n_records, int cus, int d1, int g1, int g2, int int8, int pinned);

/* DRED decoder (DRED_rdovae_decode_all per stream, dred_kernels.hip.h): one launch decodes every active stream's whole latent chain.
 * Nothing is kept per stream between calls.  state [n][state_dim], latents [n][max_latents][latent_dim], count [n] (host, 0 .. max_latents),
 * features [n][4 max_latents][20]: rows 4 count[s] and beyond of a stream are not written.  The device forms only enqueue (not on a capturing stream:
 * the launch depends on the host arrays); the packed form writes rows first[s] .. first[s] + take[s] - 1 of every stream in reverse order into one
 * [sum(take)][20] array, stream 0's first -- the layout lpcn_batch_dev_plc_fec_feed reads. */
int  lpcn_engine_dred_present(const lpcn_engine *e);          /* lpcn_dred_model.present of the engine's blob */
int  lpcn_batch_dev_dred_enable(lpcn_batch_dev *b, int max_latents);
int  lpcn_batch_dev_dred_enabled(const lpcn_batch_dev *b);    /* max_latents, 0 before lpcn_batch_dev_dred_enable */
int  lpcn_batch_dev_dred_dims(const lpcn_batch_dev *b, int *latent_dim, int *state_dim);
int  lpcn_batch_dev_dred_flavour(const lpcn_batch_dev *b);    /* 0 float decoder, 1 int8; LPCN_E_MODEL before dred_enable */
int  lpcn_batch_dev_dred_set_form(lpcn_batch_dev *b, int S);  /* streams per workgroup: 1, 2, 4, 8; 0 = the table's choice */
int  lpcn_batch_dev_dred_form(const lpcn_batch_dev *b, int n);/* what a launch over n streams runs with */
int  lpcn_batch_dev_dred_set_fast(lpcn_batch_dev *b, int mode);   /* 0 PARITY, 1 FAST at the engine's tile, 16 / 32 FAST at that tile; LPCN_E_MODEL on an int8 decoder */
int  lpcn_batch_dev_dred_get_fast(const lpcn_batch_dev *b);
int  lpcn_batch_dev_dred_check(const lpcn_batch_dev *b, const int *count, const int *first, const int *take, long long *rows);   /* the argument checks alone; *rows = sum(take) */
int  lpcn_batch_dev_dred_decode(lpcn_batch_dev *b, const float *d_state, const float *d_latents, const int *count, float *d_features, void *hip_stream);
int  lpcn_batch_dev_dred_decode_packed(lpcn_batch_dev *b, const float *d_state, const float *d_latents, const int *count, const int *first, const int *take,
                                       float *d_packed, void *hip_stream);
int  lpcn_batch_dev_dred_decode_host(lpcn_batch_dev *b, const float *state, const float *latents, const int *count, float *features);
/* ... and the decoder as a per-stream state (DRED_rdovae_dec_init_states / DRED_rdovae_decode_qframe): a float record per stream, one
 * of the batch's per-stream arrays.  init: state -> the records of the selected streams (which == NULL: every active one).  step: latents start ..
 * start + count - 1 from the record, feature rows 4 start .. 4 (start + count) - 1 (start == count == NULL: first_latent / n_latents for every active
 * stream -- nothing of the launch depends on the host, so it can be captured). */
int  lpcn_batch_dev_dred_state_enable(lpcn_batch_dev *b);                     /* after dred_enable; LPCN_E_MODEL before it */
int  lpcn_batch_dev_dred_state_enabled(const lpcn_batch_dev *b);              /* floats of one stream's three states, 0 before dred_state_enable */
int  lpcn_batch_dev_dred_get_dec_state(lpcn_batch_dev *b, int stream, float *out);      /* dense2_state, dense4_state, dense6_state */
int  lpcn_batch_dev_dred_set_dec_state(lpcn_batch_dev *b, int stream, const float *in);
int  lpcn_batch_dev_dred_init_check(const lpcn_batch_dev *b, const int *which);         /* the argument checks alone */
int  lpcn_batch_dev_dred_step_check(const lpcn_batch_dev *b, const int *start, const int *count, int first_latent, int n_latents, const int *first, const int *take,
                                    long long *rows);
int  lpcn_batch_dev_dred_init(lpcn_batch_dev *b, const float *d_state, const int *which, void *hip_stream);
int  lpcn_batch_dev_dred_step(lpcn_batch_dev *b, const float *d_latents, const int *start, const int *count, int first_latent, int n_latents, float *d_features,
                              void *hip_stream);
int  lpcn_batch_dev_dred_step_packed(lpcn_batch_dev *b, const float *d_latents, const int *start, const int *count, const int *first, const int *take,
                                     float *d_packed, void *hip_stream);
int  lpcn_batch_dev_dred_init_host(lpcn_batch_dev *b, const float *state, const int *which);
int  lpcn_batch_dev_dred_step_host(lpcn_batch_dev *b, const float *latents, const int *start, const int *count, float *features);

/* DRED encoder (DRED_rdovae_encode_dframe per stream and double frame, rdovae_enc_kernels.hip.h): one launch encodes every active
 * stream's double frames of a call.  Per stream the batch keeps the three GRU states and the conv memory: zero when the encoder is enabled, zeroed by
 * lpcn_batch_dev_reset, carried by the stream copies.  features [n][2 max_dframes][stride] (stride >= 20: the first 20 floats of a row are read),
 * count [n] (host, 0 .. max_dframes; NULL: n_dframes for every active stream), latents [n][max_dframes][latent_dim], initial [n][max_dframes]
 * [state_dim]: rows count[s] and beyond of a stream are not written, and a stream with count 0 keeps its state.  The device form only enqueues; with a
 * count array not on a capturing stream (the launch depends on it). */
int  lpcn_batch_dev_dred_enc_enable(lpcn_batch_dev *b, int max_dframes);
int  lpcn_batch_dev_dred_enc_enabled(const lpcn_batch_dev *b);/* max_dframes, 0 before lpcn_batch_dev_dred_enc_enable */
int  lpcn_batch_dev_dred_enc_flavour(const lpcn_batch_dev *b);                /* 0 float encoder, 1 int8; LPCN_E_MODEL before dred_enc_enable */
int  lpcn_batch_dev_dred_enc_info(const lpcn_batch_dev *b, int *info7);        /* {max_dframes, 40, latent, state, taps, sum of the widths, floats of a stream's state} */
int  lpcn_batch_dev_dred_enc_set_form(lpcn_batch_dev *b, int S);      /* streams per workgroup: 1, 2, 4, 8 where the buffers fit the LDS; 0 = the table's choice */
int  lpcn_batch_dev_dred_enc_form(const lpcn_batch_dev *b, int n);    /* what a launch over n streams runs with */
int  lpcn_batch_dev_dred_enc_set_fast(lpcn_batch_dev *b, int mode);   /* 0 PARITY, 1 FAST at the engine's tile, 16 / 32 FAST at that tile; LPCN_E_MODEL on an int8 encoder */
int  lpcn_batch_dev_dred_enc_get_fast(const lpcn_batch_dev *b);
int  lpcn_batch_dev_dred_enc_check(const lpcn_batch_dev *b, const int *count, int n_dframes, int stride);      /* the argument checks alone */
int  lpcn_batch_dev_dred_encode(lpcn_batch_dev *b, const float *d_features, int stride, const int *count, int n_dframes, float *d_latents, float *d_initial,
                                void *hip_stream);
int  lpcn_batch_dev_dred_encode_host(lpcn_batch_dev *b, const float *features, int stride, const int *count, float *latents, float *initial);
int  lpcn_batch_dev_dred_enc_get_state(lpcn_batch_dev *b, int stream, float *out);      /* dense2_state, dense4_state, dense6_state, bits_dense_state (oldest tap first) */
int  lpcn_batch_dev_dred_enc_set_state(lpcn_batch_dev *b, int stream, const float *in);

/* Timing of the most recent run: kernel-only milliseconds measured with HIP events on the
 * stream the kernels were launched on (sample kernel, frame kernels). */
int  lpcn_batch_dev_last_timing(lpcn_batch_dev *b, float *ms_sample, float *ms_frame);
int  lpcn_batch_dev_enable_timing(lpcn_batch_dev *b, int on);
/* samples produced per frame (default 160); lpcnet_synthesize(st, f, out, N) maps to N here */
int  lpcn_batch_dev_set_frame_len(lpcn_batch_dev *b, int n);
/* tests only: per-sample trace of workgroup 0 / stream 0 (host_out == NULL: (re)allocate n_samples records) */
int  lpcn_batch_dev_debug_trace(lpcn_batch_dev *b, int n_samples, float *host_out);
/* per-phase shader-clock totals of workgroup 0 (out == NULL: enable and zero; else fetch 8 values) */
int  lpcn_batch_dev_profile(lpcn_batch_dev *b, unsigned long long *out);

/* test seam: this engine's own 10^x (lpcnet_exp10.h) evaluated on the device for host arrays */
int  lpcn_debug_exp10(int device, const float *x, double *out, size_t n);
/* test seam: v_mfma_f32_4x4x1 with C = -0.0 against v_mul_f32, and the halves of v_pk_mul_f32 / v_pk_add_f32 against the scalar
 * instructions, as bit patterns (engine_probe.hip: lpcn_arith_identity_kernel); n = operand count, a multiple of 64; outputs [n][4] each */
/* test seam: v_cvt_rpi_i32_f32 against (int)floor(.5 + (double)t) on all 2^32 bit patterns (engine_probe.hip: lpcn_quant_sweep_kernel);
 * out3 = {mismatches among finite |t| < 2^31, mismatches with |t| <= 127.5, one mismatching pattern} */
int  lpcn_debug_quant_sweep(int device, unsigned long long *out3);
int  lpcn_debug_arith_identities(int device, const float *a, const float *b, uint32_t *out_mfma, uint32_t *out_mul,
                                 uint32_t *out_pk, uint32_t *out_sc, size_t n);

#ifdef __cplusplus
}
#endif
#endif
