// The plain argument records of the engine's kernels, as the host stores them (engine_core.h) and the kernel headers take them.  No kernels and no
// device functions: any unit may include this.
#pragma once
#include "lpcnet_engine.h"

struct LpcnFrameModel {
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b;   // [3][in][128]
    const float *pitch_emb;                               // [256][64]
    const float *dense1_w, *dense1_b, *dense2_w, *dense2_b;
    const float *a_dense_w, *a_dense_b;                   // [128][1152]
    const float *b_dense_w, *b_dense_b;                   // [128][48]
    const float *tab_tansig, *tab_idct, *tab_tw;
    const short *tab_bitrev;
    float lpc_gamma;
    int end2end;                 // END2END model: LPC = rc2lpc(first 16 conditioning outputs), no cepstral LPC, no delay line
};

namespace lpcn {

struct DecodeTables {
    const float *cb1, *cb2, *cb3;     // [1024][17] each (ceps_codebook1..3)
    const float *cb_diff4;            // [4096][18]
    const float *pitch;               // [64] = (float)(pow(2.f, k/21.)*32), evaluated by the host libm (src/lpcnet_dec.c:107)
};

struct EncodeTables {
    const float *cb1, *cb2, *cb3, *cb_diff4;   // row-major, the decode kernel's copies
    const float *cb1_t, *cb2_t, *cb3_t;        // [17][1024]
    const float *cbd_t;                        // [4][18][1024]: quarter q holds entries 1024 q ..
};

// the PLC network on the device (widths from the blob; the sparse GRU input matrices as the blob has them plus per-row-group starts)
struct PlcNet {
    int d1, g1, g2;
    const float *dense1_w, *dense1_b;
    const float *gru1_w, *gru1_rec, *gru1_bias;
    const int *gru1_start, *gru1_pos;            // [3 g1 / 8 + 1] first block of a row group, [blocks] input position of a block
    const float *gru2_w, *gru2_rec, *gru2_bias;
    const int *gru2_start, *gru2_pos;
    const float *out_w, *out_b;
    const float *tansig;
};

// per-stream PLC data (the fields of LPCNetPLCState that hold samples, features and network state; src/lpcnet_private.h:79-105)
struct PlcData {
    short *q;            // [n][560] st->pcm
    float *feat;         // [n][20]  st->features
    float *net;          // [n][4][g1 + g2]: plc_net, plc_copy[0..2]
    double *dc;          // [n][2]   dc_mem, syn_dc
    int *delta;          // [n]      the step's `delta` (src/lpcnet_plc.c:198)
    float *fec;          // [n][100][20]
    float *fbuf;         // [n][4][20] the synthesis state's deferred feature queue (src/lpcnet.c:122-144)
    short *lp;           // [n][160] the step's low-pass samples
    float *burg;         // [n][36]
    float *an;           // [n][36]  analysis of the step's frame
};

// ... of an int8 blob (plc_pred_i8_kernel)
struct PlcNetQ {
    int d1, g1, g2;
    const float *dense1_w, *dense1_b;
    const int *gru1_w, *gru1_rec;                // [blocks][8 rows] and [g1 / 4][3 g1] dwords: the four int8 weights of (row, block)
    const float *gru1_bias;
    const int *gru1_start, *gru1_pos;            // [3 g1 / 8 + 1] first block of a row group, [blocks] input DWORD (position / 4) of a block
    const int *gru2_w, *gru2_rec;
    const float *gru2_bias;
    const int *gru2_start, *gru2_pos;
    const float *out_w, *out_b;
    const float *tansig;
};

// the DRED decoder on the device (dred_decode_kernel), a device-resident block the kernel walks step by step: three dense layers from the initial
// state to the GRU states, the eight layers of a latent, dec_final.  The blob's arrays as they are, the sparse GRU input matrices with per-row-group
// starts like the PLC network's.  x / out: where a step reads and writes in the concatenated buffer, in cells of S floats (x < 0: the input vector)
struct DredStep {
    int gru;                         // 0: dense, tanh; 1: GRU (out = its state's segment)
    int n_in, n_out, x, out;
    const float *w, *b, *rec;        // dense [n_in][n_out], [n_out]; GRU blocks [nb][4][8], bias [2][3 n_out], recurrent [n_out][3 n_out]
    const int *start, *pos;          // GRU: [3 n_out / 8 + 1] first block of a row group, [blocks] input position of a block
};
struct DredNet {
    int latent_dim, state_dim, max_gru, total;       // (total: the buffer's length = dec_final's inputs)
    DredStep init[3], step[8];
    const float *final_w, *final_b;                  // [total][80], [80]
    const float *tansig;
};

// a compacted group's rows in and out (group_gather_kernel, group_scatter_kernel)
struct GroupRows {
    const int *map;
    int cnt;
    lpcn_stream_state *states, *gstates;       // every stream's record; the group's
    const float *feat;                         // gather: every stream's features (NULL: none)
    size_t feat_stride;
    float *gfeat;
    float *keep_a, *keep_b, *keep_lpc;         // every stream's kept frame products ...
    float *cond_a, *cond_b, *lpc;              // ... and the group's rows of the frame products
    short *pcm;                                // gather: the samples to impose; scatter: where the N samples go (NULL: nothing moves)
    size_t pcm_stride;
    short *gpcm;
    int N;
    int feat_vec, pcm_vec;
    int keep;                                  // gather: the kept products come in; scatter: the group's products are kept
    int state_back;                            // scatter: the states go back
};

}  // namespace lpcn
