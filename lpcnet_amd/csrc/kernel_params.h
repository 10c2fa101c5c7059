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

// A GRU-B layer on the device: the blob's arrays plus, for the sparse input matrix, the first block of every 8-row group and the blocks' input positions
// (the index stream {count, pos...} of src/vec.h:347-360 without its counts).  W = float: blocks [nb][4][8], recurrent [n][3 n], pos = the input position
// of a block (gru_b, frame_nets.hip.h).  W = int, an int8 (DOT_PROD) layer: one dword holds the four int8 weights of (row, block) -- blocks [nb][8 rows],
// recurrent block-major [n / 4][3 n] -- and pos = the input DWORD (position / 4) of a block (plc_gru_i8).
template <typename W>
struct GruLayer {
    int n_in, n;
    const W *w, *rec;
    const float *bias;                           // [2][3 n]
    const int *start, *pos;                      // [3 n / 8 + 1], [blocks]
};

// the PLC network on the device, widths from the blob: dense 57 -> d1 tanh, GRU d1 -> g1, GRU g1 -> g2, dense g2 -> 20 linear.  The dense layers are
// float in both flavours; PlcNet is a float blob's (plc_pred_kernel), PlcNetQ an int8 blob's (plc_pred_i8_kernel)
template <typename W>
struct PlcNetT {
    int d1;
    const float *dense1_w, *dense1_b;
    GruLayer<W> gru[2];
    const float *out_w, *out_b;
    const float *tansig;
};
using PlcNet = PlcNetT<float>;
using PlcNetQ = PlcNetT<int>;

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

// the DRED decoder on the device (dred_decode_kernel), a device-resident block the kernel walks step by step: three dense layers from the initial
// state to the GRU states, the eight layers of a latent, dec_final.  The blob's arrays as they are, the sparse GRU input matrices with per-row-group
// starts (GruLayer).  x / out: where a step reads and writes in the concatenated buffer, in cells of S floats (x < 0: the input vector).  W = float:
// a float blob's (DredStep, DredNet); W = int: an int8 (DOT_PROD) blob's, whose dense layers are float too and whose GRUs are GruLayer<int>'s
// (dred_decode_i8_kernel).  The float record's layout is the same in both
template <typename W>
struct DredStepT {
    int gru;                         // 0: dense, tanh; 1: GRU (out = its state's segment)
    int n_in, n_out, x, out;
    union {
        const float *w;              // dense [n_in][n_out]
        const W *gw;                 // GRU blocks: float [nb][4][8], int [nb][8 rows]
    };
    const float *b;                  // dense [n_out]; GRU bias [2][3 n_out]
    const W *rec;                    // GRU recurrent: float [n_out][3 n_out], int block-major [n_out / 4][3 n_out]
    const int *start, *pos;          // GRU: [3 n_out / 8 + 1] first block of a row group, [blocks] input position (int: input dword) of a block
};
using DredStep = DredStepT<float>;
template <typename W>
struct DredNetT {
    int latent_dim, state_dim, max_gru, total;       // (total: the buffer's length = dec_final's inputs)
    DredStepT<W> init[3], step[8];
    const float *final_w, *final_b;                  // [total][80], [80]
    const float *tansig;
};
using DredNet = DredNetT<float>;
using DredNetQ = DredNetT<int>;
// the FAST decoder's image of the three GRUs' sparse input matrices (dred_fast_kernel; dred_fast_pack.h): per (unit tile of 32, gate) the union of the
// tile's row groups' blocks.  start [3 tiles + 1], pos [blocks], w [blocks][4][32].  A device-resident block beside the DredNet, which FAST reads too
struct DredFastGru { const int *start, *pos; const float *w; };
struct DredFastImage { DredFastGru gru[3]; };

// the DRED encoder on the device (rdovae_enc_kernel), walked like the decoder's block: the eight layers of a double frame, gdense1 (from the buffer's
// start to the cells behind it), then the two layers that read no DredStep cell range: bits_dense over the window and gdense2, straight to the outputs.
// A stream's state record in global memory: the three GRU states (gru_floats, at gru_off[g] of the buffer), the conv memory as a ring of taps - 1
// slots of `total` floats, and the ring's head (int): the slot of the oldest tap.  W as in DredNetT (int: rdovae_enc_i8_kernel); the state record is
// float in both
template <typename W>
struct DredEncNetT {
    int latent_dim, state_dim, max_gru, total, taps, gd1, gru_floats;
    int gru_off[3], gru_n[3];
    DredStepT<W> step[9];                            // (step[8]: gdense1)
    const float *bits_w, *bits_b;                    // [taps total][latent], [latent]
    const float *g2_w, *g2_b;                        // [gd1][state], [state]
    const float *tansig;
};
using DredEncNet = DredEncNetT<float>;
using DredEncNetQ = DredEncNetT<int>;

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
