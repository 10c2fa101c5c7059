/* What the units of the C host shell share (api_core.c, api_stream.c, api_batch.c, api_tools.c): the real layout of the public
 * state types, the per-thread error words and the read side of the VQ codebook store.  Private to the shell: nothing declared
 * here is exported from the library. */
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "lpcnet.h"
#include "lpcnet_batch.h"
#include "lpcnet_engine.h"
#include "api_shards.h"

#define LPCN_MAGIC 0x4C50434Eu   /* "LPCN" */

#define MAX_FEATURE_BUFFER_SIZE 4     /* src/lpcnet_private.h:26 */

struct LPCNetState {
    uint32_t magic;
    int32_t model_id;                 /* index into the registry, -1 = no model bound */
    lpcn_stream_state s;
    /* the frame products live in the state like in the reference (src/lpcnet_private.h:36-38), so that
     * run_frame_network and lpcnet_synthesize_tail_impl can be called separately (PLC, src/lpcnet_plc.c) */
    float gru_a_condition[LPCN_ROWS_A];
    float gru_b_condition[LPCN_ROWS_B];
    float feature_buffer[NB_FEATURES * MAX_FEATURE_BUFFER_SIZE];   /* run_frame_network_deferred queue */
    int32_t feature_buffer_fill;
};

_Static_assert(sizeof(struct LPCNetState) == LPCNET_HIP_STATE_BYTES, "include/lpcnet.h: LPCNET_HIP_STATE_BYTES is stale");

/* include/lpcnet_hip_state.h publishes this layout with the reference's member names (the unmodified src/lpcnet_plc.c is
 * compiled against it, integration/lpcnet_private_hip.h): every member the PLC touches must sit where that header says */
#define LPCNetState LPCNetState_published
#include "../../include/lpcnet_hip_state.h"
#undef LPCNetState
#define SAME_OFF(pub, mine) _Static_assert(offsetof(struct LPCNetState_published, pub) == offsetof(struct LPCNetState, mine), "include/lpcnet_hip_state.h is stale: " #pub)
_Static_assert(sizeof(struct LPCNetState_published) == sizeof(struct LPCNetState), "include/lpcnet_hip_state.h is stale");
SAME_OFF(nnet.gru_a_state, s.gru_a); SAME_OFF(nnet.gru_b_state, s.gru_b); SAME_OFF(nnet.feature_conv1_state, s.conv1_mem);
SAME_OFF(nnet.feature_conv2_state, s.conv2_mem); SAME_OFF(old_lpc, s.old_lpc); SAME_OFF(last_sig, s.last_sig);
SAME_OFF(deemph_mem, s.deemph_mem); SAME_OFF(last_exc, s.last_exc); SAME_OFF(frame_count, s.frame_count); SAME_OFF(hip_rng, s.rng);
SAME_OFF(lpc, s.lpc); SAME_OFF(gru_a_condition, gru_a_condition); SAME_OFF(gru_b_condition, gru_b_condition);
SAME_OFF(feature_buffer, feature_buffer); SAME_OFF(feature_buffer_fill, feature_buffer_fill);
#undef SAME_OFF

struct LPCNetDecState {
    LPCNetState lpcnet_state;         /* reference: src/lpcnet_private.h:50-53 */
    float vq_mem[LPCN_NB_BANDS];
};

/* A batch is one or more shards: contiguous blocks of streams (api_shards.h), each on its own HIP device with its own engine,
 * device buffers and stream (streams are independent, so shards never communicate). */
typedef struct {
    int device;
    lpcn_engine *engine;
    lpcn_batch_dev *dev;
    int cb_version;                   /* version of the codebooks on the device (0 = none) */
} batch_shard;

struct LPCNetBatch {
    int n, n_shards;
    shard_span at[LPCN_MAX_SHARDS];   /* the streams of shard k ... */
    batch_shard sh[LPCN_MAX_SHARDS];  /* ... and where they live */
    unsigned long long model_hash;    /* FNV-1a of the model blob (lpcnet_batch_load_model): travels in a snapshot's layout, for information */
};

#pragma GCC visibility push(hidden)
extern __thread char tl_err[512];     /* (api_core.c) */
extern __thread int tl_status;        /* sticky: code of the first failed void entry point on this thread since lpcnet_hip_clear_error() */
static inline void set_err(const char *msg) { snprintf(tl_err, sizeof(tl_err), "%s", msg); }
static inline void take_engine_err(void) { snprintf(tl_err, sizeof(tl_err), "%s", lpcn_last_error()); }
#define FWD(call) do { int rc_ = (call); if (rc_) take_engine_err(); return rc_; } while (0)

/* whole file into malloc'ed memory (NULL if absent / unreadable / empty) */
unsigned char *read_file(const char *path, long *len);

/* The four VQ codebooks, read-locked (shared) until codebooks_unlock(): cb[0] is NULL when none are installed; *version moves
 * with every lpcnet_hip_set_codebooks (a batch re-uploads lazily). */
const float *const *codebooks_rdlock(int *version);
void codebooks_unlock(void);

/* lpcnet_decode's unpacker (api_stream.c): one packet and the stream's VQ memory -> 4 feature vectors; -1 when cb[0] is NULL */
int packet_to_features(const float *const *cb, float feat[4][NB_TOTAL_FEATURES], float *vq_mem, const unsigned char *buf);

/* device of the single-stream API: lpcnet_hip_set_device(), $LPCNET_HIP_DEVICE, else 0 (api_stream.c) */
int single_stream_device(void);
#pragma GCC visibility pop
