/* lpcnet_batch.h -- batched multi-stream extension of the LPCNet C API (additive).
 *
 * The reference library is one-state-one-stream and single threaded (src/lpcnet.c has no
 * threading); the MI355X engine gets its throughput from thousands of independent streams, so
 * this header adds a batch object that owns the per-stream state on the device.  A batch is
 * semantically n independent LPCNetState objects driven in lock step:
 *   lpcnet_batch_synthesize(b, F, stride, P, T)  ==  for every stream s, for t < T:
 *       lpcnet_synthesize(state[s], &F[(s*T + t)*stride], &P[(s*T + t)*160], 160)
 * Streams never interact, so several batches (one per GPU, one process per GPU) shard a workload
 * with no communication.
 */
#ifndef LPCNET_BATCH_H_
#define LPCNET_BATCH_H_

#include "lpcnet.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct LPCNetBatch LPCNetBatch;

/* n_streams independent synthesis states on HIP device `device`; NULL on failure. */
LPCNET_EXPORT LPCNetBatch *lpcnet_batch_create(int n_streams, int device);
/* The same, sharded over several HIP devices of one node: device k of `devices[0..n_devices)` owns a
 * contiguous block of streams (sizes differ by at most one), with its own copy of the model, its own device buffers
 * and HIP stream; host-pointer calls (synthesize, decode) run one host thread per shard concurrently and involve no
 * communication between devices.  A device may be listed more than once (several shards on one GPU). */
LPCNET_EXPORT LPCNetBatch *lpcnet_batch_create_sharded(int n_streams, const int *devices, int n_devices);
LPCNET_EXPORT int lpcnet_batch_shards(const LPCNetBatch *b);
/* block of streams [first, first+count) and device of one shard (any output may be NULL) */
LPCNET_EXPORT int lpcnet_batch_shard_info(const LPCNetBatch *b, int shard, int *first, int *count, int *device);
LPCNET_EXPORT void lpcnet_batch_destroy(LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_streams(const LPCNetBatch *b);
/* like lpcnet_load_model(): 0 or -1.  The blob is copied; it may be freed afterwards. */
LPCNET_EXPORT int lpcnet_batch_load_model(LPCNetBatch *b, const unsigned char *data, int len);
/* lpcnet_reset() on streams [first, first+count) */
LPCNET_EXPORT int lpcnet_batch_reset(LPCNetBatch *b, int first, int count);

/* Host-pointer synthesis: features [n_streams][n_frames][feat_stride] (only [0..19] of a frame are
 * read, feat_stride >= 20; 36 = `lpcnet_demo -synthesis` file layout), pcm [n_streams][n_frames*160].
 * Copies in, runs, copies out, synchronises.  Returns 0 or a negative error code. */
LPCNET_EXPORT int lpcnet_batch_synthesize(LPCNetBatch *b, const float *features, int feat_stride, short *pcm, int n_frames);
/* Device-pointer synthesis: same layouts in device memory of the batch's device; only enqueues on
 * `hip_stream` (a hipStream_t; NULL = the batch's own stream).  lpcnet_batch_sync() waits.
 * Ordering: calls on different streams are ordered by the batch (an event chain); the batch's buffers and stream states are
 * shared by all of them.  HIP graphs: the call may be issued on a stream that is being CAPTURED (nothing runs, nothing is
 * allocated or synchronised; any number of launches may be captured, the kernels' arguments travel inside the graph).  The
 * event chain does not see a capture, so REPLAYS of such a graph are not ordered against other work on the same batch --
 * eager calls, other graphs, state export / import, reset: put them on the replay's stream or order them with events, exactly
 * as for two kernels that share a buffer. */
LPCNET_EXPORT int lpcnet_batch_synthesize_device(LPCNetBatch *b, const float *d_features, int feat_stride, short *d_pcm,
                                                 int n_frames, void *hip_stream);
/* device-pointer synthesis on ONE shard of a sharded batch: pointers are on that shard's device and cover only its
 * `count` streams ([count][n_frames][feat_stride] / [count][n_frames*160]) */
LPCNET_EXPORT int lpcnet_batch_synthesize_device_shard(LPCNetBatch *b, int shard, const float *d_features, int feat_stride,
                                                       short *d_pcm, int n_frames, void *hip_stream);
/* waits for everything enqueued for this batch, on whichever stream(s) it was enqueued */
LPCNET_EXPORT int lpcnet_batch_sync(LPCNetBatch *b);
/* Teacher-forced variant = lpcnet_synthesize_impl(..., preload) of the reference
 * (src/lpcnet.c:256-259,273): the first `preload` samples of every frame are read from pcm. */
LPCNET_EXPORT int lpcnet_batch_synthesize_preload(LPCNetBatch *b, const float *features, int feat_stride, short *pcm,
                                                  int n_frames, int preload);
/* ONE frame step with PER-STREAM arguments -- what a batched packet-loss concealment needs (src/lpcnet_plc.c drives each of
 * its streams with lpcnet_synthesize_impl(N, preload), lpcnet_synthesize_tail_impl(N, preload) or nothing, depending on that
 * stream's losses).  features [n_streams][feat_stride], pcm [n_streams][160]; per stream s:
 *   mode[s] = 0  leave the stream alone
 *   mode[s] = 1  frame network on features[s], then n_samples[s] samples      (lpcnet_synthesize_impl, src/lpcnet.c:273-277)
 *   mode[s] = 2  n_samples[s] samples from the products of the stream's most recent mode-1 step
 *                                                                          (lpcnet_synthesize_tail_impl, src/lpcnet.c:235-271)
 *   n_samples[s] in 1..160; the first preload[s] <= n_samples[s] samples of pcm[s] are imposed on the synthesis filter
 *   (teacher forcing, src/lpcnet.c:256-259) and returned unchanged; samples n_samples[s]..159 of pcm[s] are not touched.
 * Streams with equal (mode, n_samples, preload) run together; results are bit-identical to driving each stream alone through
 * the single-stream entry points.  Meant for occasional use (it compacts and scatters the groups), not for throughput.
 * A mode-2 step needs a mode-1 step of THIS call as the stream's most recent frame step: the products are kept per stream
 * only here, so after lpcnet_batch_synthesize* / _decode* / a reset / a state import the call returns -4 (bad argument) for
 * such a stream (checked for all streams before anything runs).  The call is not atomic across groups: if a later group
 * fails on the device, earlier groups of the same call have already advanced. */
LPCNET_EXPORT int lpcnet_batch_synthesize_step(LPCNetBatch *b, const float *features, int feat_stride, short *pcm,
                                               const int *n_samples, const int *preload, const int *mode);
/* Codec path: packets [n_streams][n_packets][8] -> pcm [n_streams][n_packets*640] (lpcnet_decode per stream) */
LPCNET_EXPORT int lpcnet_batch_decode(LPCNetBatch *b, const unsigned char *packets, short *pcm, int n_packets);
/* the same with device pointers (packets [n][n_packets][8], pcm [n][n_packets*640]), only enqueued on `hip_stream`
 * (NULL = the batch's own stream): bit unpacking, VQ lookup and interpolation (decode_packet, src/lpcnet_dec.c:81-155)
 * run in a device kernel; the per-stream VQ memory lives on the device and is cleared by lpcnet_batch_reset */
/* LPC_GAMMA (bandwidth expansion of the LPC filter, lpc_weighting src/freq.c:299-308) is a compile-time constant of the
 * reference's generated nnet_data.h, not part of the weight blob; models trained with --lpc-gamma != 1 set it after
 * lpcnet_batch_load_model.  gamma in (0, 1], default 1; any other value (NaN included) returns LPCNET_HIP_E_ARG and leaves the batch as it
 * was.  The value reaches every shard's engine.  It weights the coefficients the synthesis filter CONSUMES (synthesize*, decode*, the PLC's
 * frame networks); the stored delay line stays unweighted, and analysis and the encoder, which the reference never weights, are unaffected.
 * lpcnet_batch_load_model builds new engines: a later call of it puts gamma back to 1 (set it again).  Without a model: LPCNET_HIP_E_MODEL. */
LPCNET_EXPORT int lpcnet_batch_set_lpc_gamma(LPCNetBatch *b, float gamma);
/* END2END models: the reference's compile-time END2END (src/lpcnet.c:56-80,107-108) -- the LPC filter comes from the
 * first 16 conditioning outputs (reflection coefficients, rc2lpc) instead of the cepstrum, weighted by LPC_GAMMA like the cepstral ones and
 * without the two-frame delay line, which is left alone; set after lpcnet_batch_load_model.  Default off; lpcnet_batch_load_model builds new
 * engines, so a later call of it switches END2END off again (set it again).  Without a model: LPCNET_HIP_E_MODEL. */
LPCNET_EXPORT int lpcnet_batch_set_end2end(LPCNetBatch *b, int on);
/* Arithmetic flavour of the sample loop.  0 = PARITY (default): every product and sum rounded like the reference's
 * generic-C build, results bit-identical to it.  1 = FAST: the arithmetic of the reference's own SIMD builds -- fused
 * multiply-add for float blobs (src/vec_avx.h:790-858), int32 block accumulation for int8 blobs (src/vec_avx.h:690-750) --
 * not bit-identical to any reference build (those differ among themselves as well); tests/test_gpu_fast.py keeps its
 * teacher-forced deviation inside the reference's own AVX2-vs-generic envelope.
 * 2 = FAST with the dual fully-connected layer of the sampler in fp16 (weights and GRU-B state as halves, fp32 accumulation,
 * v_dot2_f32_f16): BASELINE.json config 4's "fp16 dual-FC".  The reference has no fp16 arithmetic, so the pin is to a stated
 * definition: the oracle restates it (oracle/lpcnet_oracle.c: orc_mdense_f16_path -- binary16 weights and GRU-B state, fp32
 * sums, both v_dot2 rounding orders) and replays every tree decision of the engine from the traced GRU-B state against the
 * reference RNG's thresholds, within a 2e-4 x max(1, |logit|) band (tests/test_gpu_fast.py::
 * test_fp16_dual_fc_against_the_oracle_restatement; fewer than 1 % of the decisions may fall inside the band).
 * Both FAST flavours run at up to four streams per workgroup; FAST = 1 runs the two-group kernel (eight) for a batch that asked with
 * lpcnet_batch_set_fast_two_group. */
LPCNET_EXPORT int lpcnet_batch_set_fast(LPCNetBatch *b, int on);
LPCNET_EXPORT int lpcnet_batch_decode_device(LPCNetBatch *b, const unsigned char *d_packets, short *d_pcm, int n_packets,
                                             void *hip_stream);

/* Feature analysis: lpcnet_compute_single_frame_features (src/lpcnet_enc.c:919; _float: :927) for every stream and frame, on the
 * device, bit-identical to the reference's generic-C float build:
 *   pcm [n_streams][n_frames*160] -> features [n_streams][n_frames][feat_stride], feat_stride >= 36, floats 0..35 of a frame written:
 *   [0..17] cepstrum, [18] pitch, [19] pitch correlation, [20..35] LPC -- what `lpcnet_demo -features` writes and
 *   lpcnet_batch_synthesize* reads with feat_stride 36.
 * A batch is n independent LPCNetEncState objects as well: the analysis state (per stream, on the device) is separate from the
 * synthesis state -- lpcnet_batch_reset does not touch it, lpcnet_batch_analysis_reset is lpcnet_encoder_init on a range of streams.
 * It is allocated (all zero) by the first analysis call or by lpcnet_batch_analysis_enable; batches that never analyse allocate nothing.
 * Analysis needs no weights, but the device side of a batch (engine, stream, buffers) is created by lpcnet_batch_load_model: on a
 * batch without a model every call below returns LPCNET_HIP_E_MODEL with a message.
 * Host-pointer calls copy in, run, copy out and synchronise (one host thread per shard); any n_frames >= 1. */
LPCNET_EXPORT int lpcnet_batch_analyze(LPCNetBatch *b, const short *pcm, float *features, int feat_stride, int n_frames);
LPCNET_EXPORT int lpcnet_batch_analyze_float(LPCNetBatch *b, const float *pcm, float *features, int feat_stride, int n_frames);
/* Device pointers (d_pcm: shorts, or floats when pcm_is_float != 0), enqueue only, on `hip_stream` (NULL = the batch's own): the same
 * ordering and capture rules as lpcnet_batch_synthesize_device.  Issued on a stream that is being captured the call executes,
 * allocates and synchronises nothing, so the analysis state and the kernels' scratch for n_frames per call must exist before the
 * capture starts (lpcnet_batch_analysis_enable, or an earlier eager call of at least that length): otherwise LPCNET_HIP_E_ARG. */
LPCNET_EXPORT int lpcnet_batch_analyze_device(LPCNetBatch *b, const void *d_pcm, int pcm_is_float, float *d_features, int feat_stride,
                                              int n_frames, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_analyze_device_shard(LPCNetBatch *b, int shard, const void *d_pcm, int pcm_is_float, float *d_features,
                                                    int feat_stride, int n_frames, void *hip_stream);
/* allocate the analysis state (if absent) and scratch for calls of up to max_frames frames; keeps an existing state */
LPCNET_EXPORT int lpcnet_batch_analysis_enable(LPCNetBatch *b, int max_frames);
LPCNET_EXPORT int lpcnet_batch_analysis_reset(LPCNetBatch *b, int first, int count);
/* raw per-stream analysis state (layout = struct lpcn_analysis_state in lpcnet_amd/csrc/lpcnet_engine.h): snapshot / rollback */
LPCNET_EXPORT int lpcnet_batch_analysis_state_size(void);
LPCNET_EXPORT int lpcnet_batch_get_analysis_state(LPCNetBatch *b, int stream, void *out);
LPCNET_EXPORT int lpcnet_batch_set_analysis_state(LPCNetBatch *b, int stream, const void *in);

/* The encoder of the 1.6 kb/s codec, on the device, bit-identical to the reference's generic-C float build:
 *   lpcnet_batch_encode*            lpcnet_encode (src/lpcnet_enc.c:882) per stream and packet:
 *                                   pcm [n_streams][n_packets*640] -> packets [n_streams][n_packets][8], what lpcnet_batch_decode* reads
 *   lpcnet_batch_compute_features*  lpcnet_compute_features (:895; process_superframe with encode = 0, quantize = 0):
 *                                   pcm [n_streams][n_packets*640] -> features [n_streams][n_packets*4][feat_stride], feat_stride >= 36
 * analyze, encode and compute_features act on the SAME per-stream analysis state, as the reference's three entry points act on one
 * LPCNetEncState, and may be interleaved on a stream: encode and compute_features in any order, and analyze followed by either, give the
 * reference's result.  One quirk of the reference is not reproduced: lpcnet_compute_single_frame_features never sets pcount, so after a
 * four-frame call (pcount left at 3) it analyses into features[3] and returns the stale features[0]; lpcnet_batch_analyze keeps behaving
 * as with pcount = 0.  The state evolves identically either way (no carried field depends on the slot), so a four-frame call after such
 * an analyze equals the reference again.
 * The encoder's one further carried field, vq_mem[18], is kept beside the analysis state (all zero when allocated):
 * lpcnet_batch_analysis_reset (lpcnet_encoder_init) clears it as well, lpcnet_batch_reset touches neither; a snapshot of a stream is its
 * analysis state plus its vq_mem.
 * Codebooks: as for lpcnet_batch_decode (lpcnet_hip_set_codebooks or the default file); without them encode returns what decode returns.
 * Codebooks installed while a batch exists reach its device tables with the batch's next encode or decode call.
 * compute_features needs none.  A batch without a model returns LPCNET_HIP_E_MODEL.  Host-pointer calls copy in, run, copy out and
 * synchronise (one host thread per shard); device-pointer calls only enqueue on `hip_stream` (NULL = the batch's own) under the ordering
 * and capture rules of lpcnet_batch_analyze_device: on a stream that is being captured nothing is executed, allocated or synchronised,
 * so lpcnet_batch_encoder_enable(max_packets) (state, vq_mem and scratch for calls of up to max_packets packets; implies
 * lpcnet_batch_analysis_enable(4 * max_packets)) or an earlier eager call of that length must come first: otherwise LPCNET_HIP_E_ARG. */
LPCNET_EXPORT int lpcnet_batch_encode(LPCNetBatch *b, const short *pcm, unsigned char *packets, int n_packets);
LPCNET_EXPORT int lpcnet_batch_encode_device(LPCNetBatch *b, const short *d_pcm, unsigned char *d_packets, int n_packets, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_encode_device_shard(LPCNetBatch *b, int shard, const short *d_pcm, unsigned char *d_packets, int n_packets,
                                                   void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_compute_features(LPCNetBatch *b, const short *pcm, float *features, int feat_stride, int n_packets);
LPCNET_EXPORT int lpcnet_batch_compute_features_device(LPCNetBatch *b, const short *d_pcm, float *d_features, int feat_stride, int n_packets,
                                                       void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_encoder_enable(LPCNetBatch *b, int max_packets);
LPCNET_EXPORT int lpcnet_batch_get_encoder_vq_mem(LPCNetBatch *b, int stream, float *out18);
LPCNET_EXPORT int lpcnet_batch_set_encoder_vq_mem(LPCNetBatch *b, int stream, const float *in18);

/* Packet-loss concealment on the device, bit-identical to the reference's generic-C builds (src/lpcnet_plc.c) in CAUSAL mode: the float build
 * (DISABLE_DOT_PROD) for a float blob, the int8 build (DOT_PROD, the reference's default) for an int8 blob.
 * With lpcnet_batch_plc_enable a batch is, in addition, n independent LPCNetPLCState objects: the `lpcnet` member of stream s is the
 * stream's synthesis state, the `enc` member its analysis state, everything else is per-stream PLC state.  One step advances every
 * stream by one 10-ms frame: pcm [n_streams][160] in and out, lost [n_streams] (a HOST array in every form of the call);
 *   lost[s] == 0: pcm[s] holds the received frame                 -> lpcnet_plc_update(st[s], pcm[s])
 *   lost[s] != 0: pcm[s] is ignored and receives the concealment  -> lpcnet_plc_conceal(st[s], pcm[s])
 * The PLC network comes from the same blob as the LPCNet model, as in lpcnet_plc_load_model (src/lpcnet_plc.c:88-97): arrays
 * plc_dense1_*, plc_gru1_*, plc_gru2_*, plc_out_* (training_tf2/dump_plc.py).  Its widths are read from the bias lengths (each up to 512).
 * It is served in the flavour of its blob, which is what one dump of the reference produces: float GRU arrays with a float LPCNet model,
 * int8 GRU arrays with an int8 one (src/vec.h:274-339 without USE_SU_BIAS: per 8x4 block one exact integer sum, one rounded float add).
 * plc_enable: options = LPCNET_PLC_CAUSAL or LPCNET_PLC_CODEC, optionally | LPCNET_PLC_DC_FILTER.  LPCNET_PLC_NONCAUSAL returns
 *   LPCNET_HIP_E_ARG: the reference stops in that mode when FEATURES_DELAY > 0 (src/lpcnet_plc.c:357-361) and this engine's model format has 2.
 *   A blob without the PLC arrays, with incomplete or inconsistent ones, or with a mix no reference build has -- int8 PLC arrays beside a float
 *   LPCNet model, float PLC arrays beside an int8 one -- returns LPCNET_HIP_E_MODEL with a message; so does every other call below before plc_enable.  It allocates the PLC state, implies lpcnet_batch_analysis_enable(1) and
 *   performs lpcnet_plc_reset on every stream, which resets the stream's synthesis and analysis states as the reference does (:46-60).
 * The PLC owns the streams it drives: mixing its steps with lpcnet_batch_synthesize* / _analyze* on the same streams gives what the
 * same mix gives on the reference's member states, except that a tail step after a foreign frame step uses the PLC's own last products.
 * plc_step copies in, runs, copies out and synchronises (one host thread per shard).  plc_step_device* only enqueues on `hip_stream`
 * (NULL = the batch's own) under the ordering rules of lpcnet_batch_analyze_device; `lost` is read before the call returns.  The launch
 * sequence depends on the loss flags, so on a stream that is being captured the call returns LPCNET_HIP_E_ARG and enqueues nothing.
 * plc_fec_add(features20 == NULL) is lpcnet_plc_fec_add(st, NULL): one skip.  With a full ring (100 vectors, none consumed) the vector is
 *   dropped as in the reference and the call returns 1.  fec_add waits for the batch's enqueued work.
 * plc_fec_feed is every stream's FEC traffic in one call and one launch per shard.  Per stream s it is lpcnet_plc_fec_clear(st[s]) if clear[s],
 *   then skip[s] calls of lpcnet_plc_fec_add(st[s], NULL), then lpcnet_plc_fec_add(st[s], v) for the stream's count[s] vectors in order.  count,
 *   skip, clear and dropped are host arrays [n_streams] (skip, clear, dropped may be NULL) and are read / written before the call returns;
 *   features is packed [sum(count)][20], stream 0's vectors first.  dropped[s] receives how many of the stream's vectors the reference would
 *   drop with "FEC buffer full" (always the tail of its list); the call returns 1 if any were and 0 otherwise, LPCNET_HIP_E_ARG for a negative
 *   count (nothing has changed then).  plc_fec_feed uploads, enqueues and synchronises (one host thread per shard).  plc_fec_feed_device*
 *   takes a device pointer and only enqueues on `hip_stream`, like plc_step_device: no wait for enqueued work, LPCNET_HIP_E_ARG on a capturing
 *   stream (the launch depends on the rings' positions, which the host keeps).  The _shard form covers that shard's streams, in arrays and packing.
 * get / set_plc_state: one stream's PLC state, both halves (layout = struct lpcn_plc_state_rec in lpcnet_amd/csrc/lpcnet_engine.h); with the
 *   synthesis state (get / set_raw_state) and the analysis state it is a snapshot a stream can be rolled back to. */
#ifndef LPCNET_PLC_CAUSAL
#define LPCNET_PLC_CAUSAL 0
#define LPCNET_PLC_NONCAUSAL 1
#define LPCNET_PLC_CODEC 2
#define LPCNET_PLC_DC_FILTER 4
#endif
LPCNET_EXPORT int lpcnet_batch_plc_enable(LPCNetBatch *b, int options);
LPCNET_EXPORT int lpcnet_batch_plc_flavour(const LPCNetBatch *b);      /* 0: the float PLC network runs, 1: the int8 one; LPCNET_HIP_E_MODEL before plc_enable */
LPCNET_EXPORT int lpcnet_batch_plc_reset(LPCNetBatch *b, int first, int count);
LPCNET_EXPORT int lpcnet_batch_plc_step(LPCNetBatch *b, short *pcm, const unsigned char *lost);
LPCNET_EXPORT int lpcnet_batch_plc_step_device(LPCNetBatch *b, short *d_pcm, const unsigned char *lost, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_plc_step_device_shard(LPCNetBatch *b, int shard, short *d_pcm, const unsigned char *lost, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_plc_fec_add(LPCNetBatch *b, int stream, const float *features20);
LPCNET_EXPORT int lpcnet_batch_plc_fec_clear(LPCNetBatch *b, int stream);
LPCNET_EXPORT int lpcnet_batch_plc_fec_feed(LPCNetBatch *b, const float *features, const int *count, const int *skip, const unsigned char *clear, int *dropped);
LPCNET_EXPORT int lpcnet_batch_plc_fec_feed_device(LPCNetBatch *b, const float *d_features, const int *count, const int *skip, const unsigned char *clear,
                                                   int *dropped, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_plc_fec_feed_device_shard(LPCNetBatch *b, int shard, const float *d_features, const int *count, const int *skip,
                                                         const unsigned char *clear, int *dropped, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_plc_state_size(void);
LPCNET_EXPORT int lpcnet_batch_get_plc_state(LPCNetBatch *b, int stream, void *out);
LPCNET_EXPORT int lpcnet_batch_set_plc_state(LPCNetBatch *b, int stream, const void *in);
/* parity seams: burg_cepstral_analysis (src/freq.c:190-199) of one frame per stream, x [n][160] holding int16 values as the PLC feeds
 * them -> ceps36 [n][36]; compute_plc_pred (src/lpcnet_plc.c:135-146) on every stream's network state (which advances): in57 [n][57] -> out20 [n][20] */
LPCNET_EXPORT int lpcnet_batch_plc_burg(LPCNetBatch *b, const float *x, float *ceps36);
LPCNET_EXPORT int lpcnet_batch_plc_pred(LPCNetBatch *b, const float *in57, float *out20);
/* The PLC network runs with 1, 2, 4 or 8 streams per workgroup: a workgroup loads a weight once for all its streams, and every stream's flags and
 * output bits are what they are at one stream per workgroup.  plc_set_pred_form pins S (0 = the engine's table; anything else is LPCNET_HIP_E_ARG)
 * on every shard, for tests and tools; plc_get_pred_form: what a prediction launch over n_streams streams runs with on shard 0 -- the pinned or the
 * table's value, halved until the form's LDS fits the network's widths.  lpcnet_hip_plc_pred_form is that rule alone, no device: n_records records
 * on a device of `cus` compute units, a network of widths d1 / g1 / g2, int8 != 0 for an int8 blob, pinned as above -> S, or LPCNET_HIP_E_ARG. */
LPCNET_EXPORT int lpcnet_batch_plc_set_pred_form(LPCNetBatch *b, int S);
LPCNET_EXPORT int lpcnet_batch_plc_get_pred_form(const LPCNetBatch *b, int n_streams);
LPCNET_EXPORT int lpcnet_hip_plc_pred_form(int n_records, int cus, int d1, int g1, int g2, int int8, int pinned);
/* How one lpcnet_batch_encode* call (analysis == 0, count packets) or one lpcnet_batch_analyze* call (analysis != 0, count frames) is cut into
 * launches on a shard of capacity n of whose streams the first `active` run, by the engine's own rules and without a device.  A call runs in
 * chunks that keep capacity x frames within 65 536 (the chunk follows the capacity, not the active count, and is at least one packet / one
 * frame); per chunk the two VQ kernels of the encoder give a wavefront 1 .. 4 (vq_end) and 1 .. 2 (vq_mid) of the chunk's active x packets items,
 * more than one from 8 192 items; a workgroup has eight wavefronts.  out [cap][8] receives per launch {packets or frames, items, items per
 * wavefront of vq_end, of vq_mid, workgroups of vq_end, items in its last workgroup, workgroups of vq_mid, items in its last workgroup} (the
 * last six are 0 for the analysis; lpcnet_batch_compute_features* runs the encoder's chunks without the VQ kernels).  Returns the number of
 * launches (records beyond `cap` are not written), 0 when no stream is active, LPCNET_HIP_E_ARG for n < 1, active outside 0 .. n, count < 1. */
LPCNET_EXPORT int lpcnet_hip_encode_plan(int n, int active, int count, int analysis, int *out, int cap);
/* the host planner alone, no device (tests): ctl [n][9] ints in and out, fec_op [n] or NULL (1 vector added, 2 NULL skip, 3 clear, 4 two vectors
 * added, before the step), summary [n][10] out: {lost, flushed deferred features, queue rounds, their samples, FEC vectors used, first frame after a
 * loss (1 cross-fade, 2 codec restore), queue operation (1 tail, 2 append, 3 push), prediction kept, deferred features appended, loss_count} */
LPCNET_EXPORT int lpcnet_hip_plc_plan(int options, int n, int *ctl, const unsigned char *lost, const unsigned char *fec_op, int *summary);
/* the planner alone with lanes, no device (tests).  `ctl`, `lost`, `fec_op`, `summary`: as lpcnet_hip_plc_plan.
 * launch[k] = {type (0 Burg analysis, 1 prediction, 2 element-wise operation, 3 group, 4 the frame analysis), op, lane, slot, cnt, offset of its
 * records in lists, ints per record, kind (0 frame network, 1 frame network and samples, 2 samples), N, preload}; `lists` receives the control
 * lists.  With lanes == 1 these are the launches and lists of a PLC step today; launches of different lanes in front of the type-4 launch name
 * disjoint streams, a group works in rows [slot, slot + cnt) of n, and the rows of different lanes are disjoint.  Returns the number of
 * launches, or LPCNET_HIP_E_ARG (lanes outside 1 .. 4, an array too short: ctl is unchanged then). */
LPCNET_EXPORT int lpcnet_hip_plc_plan_lanes(int options, int n, int lanes, int *ctl, const unsigned char *lost, const unsigned char *fec_op,
                                            int *summary, int *launch, int launch_cap, int *lists, int lists_cap);
/* plc_fec_feed's planner alone, no device (tests): ctl [n][9] in and out, count [n], skip / clear [n] or NULL, dropped [n] or NULL; rec [n][8] out,
 * one record per stream that stores something: {stream, first row of the packed vectors, rows a, ring row they go to, first ring row moved to the
 * front, rows moved, rows b appended after the move, ring row they go to}.  Returns the number of records, or LPCNET_HIP_E_ARG. */
LPCNET_EXPORT int lpcnet_hip_plc_fec_feed_plan(int n, int *ctl, const int *count, const int *skip, const unsigned char *clear, int *rec, int *dropped);
/* a blob's PLC network as the loader sees it, no device: info[7] = {present (0 none, 1 float arrays, 2 int8 arrays, -1 incomplete or inconsistent),
 * servable (plc_enable accepts the blob), dense width, GRU widths, 8x4 blocks of the two GRU input matrices}.  Returns 0, LPCNET_HIP_E_ARG without
 * `info`, LPCNET_HIP_E_MODEL when the blob does not load as an LPCNet model at all */
LPCNET_EXPORT int lpcnet_hip_plc_model_info(const unsigned char *data, int len, int *info);

/* The DRED decoder on the device, bit-identical to the reference's generic-C build of the blob's flavour (float, or int8 / DOT_PROD): per stream s,
 *   DRED_rdovae_decode_all(model, features[s], state[s], latents[s], count[s])      (src/dred_rdovae.c:38-52, src/dred_rdovae_dec.c:37-98)
 * -- the producer of the vectors plc_fec_feed consumes: one redundancy packet (an initial state, then one latent per 40 ms) becomes four
 * 20-float feature frames per latent, the newest first.  One launch per shard decodes every active stream's whole latent chain.
 * The decoder comes from the same blob as the LPCNet model, as write_lpcnet_weights.c:72-75 appends it: arrays state{1,2,3}_*, dec_dense{1..8}_*,
 * dec_final_* (torch/rdovae/export_rdovae_weights.py, training_tf2/dump_rdovae.py).  Its widths are read from the bias lengths (each up to 256),
 * the latent and state dimensions from dec_dense1_weights / state1_weights; dec_final has 80 outputs.  The decoder is served in its blob's own
 * flavour: float arrays beside a float LPCNet model, int8 (DOT_PROD) GRU arrays -- dec_dense2 / 4 / 6; the dense layers are float in that build too --
 * beside an int8 one.
 * dred_enable uploads the decoder and sizes the scratch for calls of up to max_latents latents per stream.  Decoder arrays of the other flavour
 *   than the LPCNet model's (int8 beside float, float beside int8), a mix of float and int8 GRUs, incomplete or inconsistent arrays and a blob
 *   without any return LPCNET_HIP_E_MODEL with a message; so does every other call below before dred_enable.
 * dred_flavour: 0 the float decoder runs, 1 the int8 one.
 * dred_decode takes host pointers: state [n][state_dim], latents [n][max_latents][latent_dim], count [n] (each 0 .. max_latents), features
 *   [n][4 max_latents][20].  Rows 4 count[s] and beyond of a stream are not written.  It copies in, runs, copies out and synchronises (one
 *   host thread per shard).  dred_decode_device* takes device pointers and only enqueues on `hip_stream` (NULL = the batch's own) under the
 *   ordering rules of lpcnet_batch_analyze_device; `count` is a host array, read before the call returns.  The launch depends on it, so on a
 *   stream that is being captured the call returns LPCNET_HIP_E_ARG and enqueues nothing.
 * dred_decode_packed_device* decodes the same values and writes rows first[s] .. first[s] + take[s] - 1 of stream s's decoded frames (host
 *   arrays) in REVERSE row order -- the oldest frame first -- into one packed array [sum(take)][20], stream 0's vectors first: the layout
 *   lpcnet_batch_plc_fec_feed_device reads, so redundancy goes from the decoder to the FEC rings without a host hop.  A permutation of
 *   dred_decode's output and nothing else.
 * A count outside 0 .. max_latents, first / take outside the stream's 4 count[s] decoded rows, and a non-zero count on a stream beyond its
 *   shard's active prefix return LPCNET_HIP_E_ARG with nothing written; the rows of inactive streams are untouched.  The _shard forms cover
 *   that shard's streams, in arrays and packing.
 * No per-stream state in dred_decode*: a call keeps nothing between calls (decode_all semantics), and lpcnet_batch_copy_streams, the roster and
 *   the state snapshots do not see it.
 *   The incremental pair underneath, init_states / decode_qframe on a per-stream state, is dred_init / dred_step below.
 *   Which arithmetic runs is the batch's own choice, call by call: lpcnet_batch_set_fast does not change this kernel; its
 *   own switch is dred_set_fast.
 * dred_set_fast(mode) selects the arithmetic of the float decoder, per batch, off by default: 0 = PARITY, the bits above; 1 = FAST with the engine's
 *   choice of tile; 16 or 32 = FAST pinned to a tile of that many streams per workgroup (the tiles that are built; for tests and tools).  FAST is the arithmetic
 *   of the reference's AVX2+FMA float build: every sum one fma chain from its bias in ascending input order (sgemv_accum16 and sparse_sgemv_accum8x4
 *   of src/vec_avx.h), computed on the fp32 matrix pipe with the streams of a workgroup as columns; exp / rcp based activations.  Its output
 *   deviates from PARITY's no more than that build's does on the same inputs, and a stream's bits do not depend on the tile, on the streams that
 *   share it, on their counts, on the active prefix or on the shards.  Every decode call follows the switch; signatures, layouts, refusals and
 *   the absence of per-stream state are the same.  Any other mode returns LPCNET_HIP_E_ARG; on an int8 decoder a non-zero mode returns
 *   LPCNET_HIP_E_MODEL (the int8 decoder has no FAST form yet) and nothing changes.  dred_get_fast: the mode that is set.  dred_set_form /
 *   dred_get_form describe the PARITY forms only.
 * dred_set_form pins the streams one workgroup carries (1, 2, 4, 8; 0 = the engine's table) for tests and tools: the output bits are the same in
 *   every form.  dred_get_form: what a launch over n_streams streams runs with.
 * dred_info: info[3] = {max_latents, latent dimension, state dimension}: the row lengths of the arrays above. */
LPCNET_EXPORT int lpcnet_batch_dred_enable(LPCNetBatch *b, int max_latents);
LPCNET_EXPORT int lpcnet_batch_dred_decode(LPCNetBatch *b, const float *state, const float *latents, const int *count, float *features);
LPCNET_EXPORT int lpcnet_batch_dred_decode_device(LPCNetBatch *b, const float *d_state, const float *d_latents, const int *count, float *d_features,
                                                  void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_decode_device_shard(LPCNetBatch *b, int shard, const float *d_state, const float *d_latents, const int *count,
                                                        float *d_features, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_decode_packed_device(LPCNetBatch *b, const float *d_state, const float *d_latents, const int *count,
                                                         const int *first, const int *take, float *d_packed, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_decode_packed_device_shard(LPCNetBatch *b, int shard, const float *d_state, const float *d_latents, const int *count,
                                                               const int *first, const int *take, float *d_packed, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_info(const LPCNetBatch *b, int *info);
LPCNET_EXPORT int lpcnet_batch_dred_flavour(const LPCNetBatch *b);     /* 0: the float decoder runs, 1: the int8 one; LPCNET_HIP_E_MODEL before dred_enable */
LPCNET_EXPORT int lpcnet_batch_dred_set_form(LPCNetBatch *b, int S);
LPCNET_EXPORT int lpcnet_batch_dred_get_form(const LPCNetBatch *b, int n_streams);
LPCNET_EXPORT int lpcnet_batch_dred_set_fast(LPCNetBatch *b, int mode);
LPCNET_EXPORT int lpcnet_batch_dred_get_fast(const LPCNetBatch *b);
/* The DRED decoder as a per-stream state: DRED_rdovae_dec_init_states and DRED_rdovae_decode_qframe on an RDOVAEDecState (include/dred_rdovae.h;
 * src/dred_rdovae_dec.c:37-98), the pair DRED_rdovae_decode_all is made of.  With consecutive ranges that partition [0, c[s]) for every stream,
 *   dred_init(state, NULL); dred_step(latents, a_0, c_0, features); ... dred_step(latents, a_k, c_k, features)
 * leaves in `features` exactly the bits dred_decode(state, latents, c, features) writes -- in every flavour, mode, form, tile, shard layout and
 * active prefix -- so a receiver decodes as far back as the gap it knows and pays only for the latents a longer gap adds.
 * dred_state_enable, after dred_enable (LPCNET_HIP_E_MODEL before it), allocates one float record per stream: dense2_state, dense4_state,
 *   dense6_state in the reference's member order at their own widths, padded to whole 16 bytes; all zero is DRED_rdovae_init_decoder.  The record
 *   is float for float and int8 blobs, PARITY and FAST: dred_set_fast may change between calls.  It is one of the batch's per-stream arrays:
 *   lpcnet_batch_reset clears it, lpcnet_batch_copy_streams / _copy_streams_to and the roster carry it, snapshots hold it as section
 *   LPCNET_SNAP_DRED_DEC.  Batches that never call it allocate nothing.  Every call below returns LPCNET_HIP_E_MODEL before it.
 * dred_dec_state_size: floats of one stream's three states; get_ / set_dred_dec_state move them in that order.
 * dred_init(state [n][state_dim], which [n] | NULL): init_states into the record of every active stream with which[s] != 0 (NULL: every active
 *   stream); the other records keep their bits.
 * dred_step(latents [n][max_latents][latent_dim], start [n], count [n], features [n][4 max_latents][20]): stream s runs decode_qframe on latents
 *   start[s] .. start[s] + count[s] - 1 from its record, writes rows 4 start[s] .. 4 (start[s] + count[s]) - 1 of its features and stores the
 *   record back.  count[s] == 0: no row written, the record untouched.  The arrays are dred_decode's own.
 * The host forms copy in, run, copy out and synchronise (one host thread per shard).  The _device forms take device pointers and only enqueue on
 *   `hip_stream` (NULL = the batch's own) under the ordering rules of lpcnet_batch_analyze_device; which / start / count are host arrays, read
 *   before the call returns, and with them a capturing stream is refused (LPCNET_HIP_E_ARG).  The UNIFORM forms -- which == NULL; start == count
 *   == NULL with first_latent / n_latents for every active stream -- depend on nothing on the host and are accepted on a capturing stream under
 *   the rules lpcnet_batch_synthesize_device states.
 * dred_step_packed_device* has dred_decode_packed_device's selection and layout (the oldest row first, what lpcnet_batch_plc_fec_feed_device
 *   reads); first / take are in the stream's own (global) row numbers and lie inside the rows this call decodes.
 * start[s] < 0, count[s] < 0, start[s] + count[s] > max_latents, a count or a `which` flag beyond the active prefix and first / take outside the
 *   call's rows return LPCNET_HIP_E_ARG with nothing written.  The _shard forms cover that shard's streams, in arrays and packing. */
LPCNET_EXPORT int lpcnet_batch_dred_state_enable(LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_dred_dec_state_size(const LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_get_dred_dec_state(LPCNetBatch *b, int stream, float *out);
LPCNET_EXPORT int lpcnet_batch_set_dred_dec_state(LPCNetBatch *b, int stream, const float *in);
LPCNET_EXPORT int lpcnet_batch_dred_init(LPCNetBatch *b, const float *state, const int *which);
LPCNET_EXPORT int lpcnet_batch_dred_init_device(LPCNetBatch *b, const float *d_state, const int *which, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_init_device_shard(LPCNetBatch *b, int shard, const float *d_state, const int *which, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_step(LPCNetBatch *b, const float *latents, const int *start, const int *count, float *features);
LPCNET_EXPORT int lpcnet_batch_dred_step_device(LPCNetBatch *b, const float *d_latents, const int *start, const int *count, int first_latent, int n_latents,
                                                float *d_features, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_step_device_shard(LPCNetBatch *b, int shard, const float *d_latents, const int *start, const int *count, int first_latent,
                                                      int n_latents, float *d_features, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_step_packed_device(LPCNetBatch *b, const float *d_latents, const int *start, const int *count, const int *first,
                                                       const int *take, float *d_packed, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_step_packed_device_shard(LPCNetBatch *b, int shard, const float *d_latents, const int *start, const int *count,
                                                             const int *first, const int *take, float *d_packed, void *hip_stream);
/* a blob's DRED decoder as the loader sees it, no device: info[12] = {present (0 none, 1 float arrays, 2 int8 arrays, -1 incomplete or
 * inconsistent), servable (dred_enable accepts the blob: the arrays are in the LPCNet model's own flavour), latent dimension, state dimension, the widths of dec_dense1 .. dec_dense8}.  Returns 0,
 * LPCNET_HIP_E_ARG without `info`, LPCNET_HIP_E_MODEL when the blob does not load as an LPCNet model at all */
LPCNET_EXPORT int lpcnet_hip_dred_model_info(const unsigned char *data, int len, int *info);

/* The DRED encoder on the device, bit-identical to the reference's generic-C build of the blob's flavour (float, or int8 / DOT_PROD): per stream s and
 * double frame d < count[s],
 *   DRED_rdovae_encode_dframe(enc_state[s], model, latents[s][d], initial_state[s][d], features[s][2 d .. 2 d + 1])
 *                                                                                 (src/dred_rdovae.c:102-105, src/dred_rdovae_enc.c:38-95)
 * -- the producer of the latents and initial states dred_decode consumes: two consecutive 20-float feature frames (20 ms) become one latent vector
 * and one initial state.  Quantisation and entropy coding of the latents are not part of it.  One launch per shard encodes every active stream's
 * double frames of a call.
 * The encoder comes from the same blob, found by name wherever its arrays stand: enc_dense{1..8}_*, bits_dense_*, gdense{1,2}_*.  Its widths are read
 * from the bias lengths (each up to 256), the latent dimension from bits_dense_bias, the taps K of the conv1d bits_dense from bits_dense_weights
 * ([K x sum of the widths][latent], oldest tap first, 1 <= K <= 8), the state dimension from gdense2_bias; enc_dense1 has 2 x 20 inputs.  The encoder
 * is served in its blob's own flavour: float arrays beside a float LPCNet model, int8 (DOT_PROD) GRU arrays (enc_dense2 / 4 / 6) beside an int8 one; the
 * per-stream state is float in both.
 * dred_enc_enable uploads the encoder, allocates every stream's state as DRED_rdovae_init_encoder leaves it (zero) -- a later call keeps the states --
 *   and sizes the calls to up to max_dframes double frames per stream.  Encoder arrays of the other flavour than the LPCNet model's, a mix of float and
 *   int8 GRUs, incomplete or inconsistent arrays and a blob without any return LPCNET_HIP_E_MODEL with a message; so does every other call below
 *   before dred_enc_enable.  dred_enc_flavour: 0 the float encoder runs, 1 the int8 one.
 * dred_encode takes host pointers: features [n][2 max_dframes][stride] with stride >= 20 -- only the first 20 floats of a row are read, so the
 *   36-float rows of lpcnet_batch_analyze go in as they are --, count [n] (each 0 .. max_dframes), latents [n][max_dframes][latent] and initial_state
 *   [n][max_dframes][state].  Rows count[s] and beyond of a stream are not written, and a stream with count 0 keeps its state.  It copies in, runs,
 *   copies out and synchronises (one host thread per shard).
 * dred_encode_device* takes device pointers and only enqueues on `hip_stream` (NULL = the batch's own) under the ordering rules of
 *   lpcnet_batch_analyze_device.  `count` is a host array read before the call returns; the launch depends on it, so on a stream that is being
 *   captured the call returns LPCNET_HIP_E_ARG and enqueues nothing.  With count = NULL every active stream encodes n_dframes double frames: that
 *   launch depends on nothing on the host and is accepted on a capturing stream (n_dframes is ignored when count is given).
 * A count outside 0 .. max_dframes, a non-zero count on a stream beyond its shard's active prefix and a stride below 20 return LPCNET_HIP_E_ARG with
 *   nothing written and no state changed; inactive streams are untouched.  The _shard forms cover that shard's streams.
 * Per-stream state: the three GRU states and the conv memory of (K - 1) x sum-of-the-widths floats.  lpcnet_batch_reset zeroes it for the streams it
 *   names, lpcnet_batch_copy_streams carries it.  dred_enc_get_state / _set_state move one stream's state in the reference's member order
 *   (RDOVAEEncState): dense2_state, dense4_state, dense6_state, then bits_dense_state, the oldest tap first -- info[6] floats.
 *   lpcnet_batch_set_fast and dred_set_fast do not change this kernel; its own switch is dred_enc_set_fast.
 * dred_enc_set_fast(mode) selects the arithmetic of the float encoder, per batch, off by default: 0 = PARITY, the bits above; 1 = FAST with the
 *   engine's choice of tile; 16 or 32 = FAST pinned to a tile of that many streams per workgroup (the tiles that are built; for tests and tools).
 *   FAST is the arithmetic dred_set_fast gives the decoder: every sum one fma chain from its bias in ascending input order on the fp32 matrix pipe
 *   -- bits_dense one chain over its whole window, the oldest tap first -- and exp / rcp based activations.  Its outputs and states deviate from
 *   PARITY's no more than the reference's AVX2+FMA float build's do on the same inputs, and a stream's bits do not depend on the tile, on the streams
 *   that share it, on their counts, on the active prefix, on the shards or on how a run of double frames is cut into calls.  Every encode call
 *   follows the switch; signatures, layouts, refusals and the per-stream state record are the same, so a batch may change the mode between calls,
 *   and reset, copy_streams, the snapshots and dred_enc_get_state / _set_state work as before.  Any other mode returns LPCNET_HIP_E_ARG; on an int8
 *   encoder a non-zero mode returns LPCNET_HIP_E_MODEL (the int8 encoder has no FAST form yet), and so does a tile whose buffers do not fit a
 *   workgroup (mode 1 takes 16 streams where 32 do not fit); nothing changes then.  dred_enc_get_fast: the mode that is set.  dred_enc_set_form /
 *   dred_enc_get_form describe the PARITY forms only.
 * dred_enc_set_form pins the streams one workgroup carries (1, 2, 4, 8; 0 = the engine's table) for tests and tools -- a form whose buffers do not
 *   fit a workgroup's LDS returns LPCNET_HIP_E_ARG -- and the output bits are the same in every form.  dred_enc_get_form: what a launch over n_streams
 *   streams runs with.
 * dred_enc_info: info[7] = {max_dframes, 40, latent dimension, state dimension, K, sum of the widths, floats of one stream's state}. */
LPCNET_EXPORT int lpcnet_batch_dred_enc_enable(LPCNetBatch *b, int max_dframes);
LPCNET_EXPORT int lpcnet_batch_dred_enc_info(const LPCNetBatch *b, int *info);
LPCNET_EXPORT int lpcnet_batch_dred_enc_flavour(const LPCNetBatch *b);     /* 0: the float encoder runs, 1: the int8 one; LPCNET_HIP_E_MODEL before dred_enc_enable */
LPCNET_EXPORT int lpcnet_batch_dred_encode(LPCNetBatch *b, const float *features, int stride, const int *count, float *latents, float *initial_state);
LPCNET_EXPORT int lpcnet_batch_dred_encode_device(LPCNetBatch *b, const float *d_features, int stride, const int *count, int n_dframes, float *d_latents,
                                                  float *d_initial_state, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_encode_device_shard(LPCNetBatch *b, int shard, const float *d_features, int stride, const int *count, int n_dframes,
                                                        float *d_latents, float *d_initial_state, void *hip_stream);
LPCNET_EXPORT int lpcnet_batch_dred_enc_get_state(LPCNetBatch *b, int stream, float *out);
LPCNET_EXPORT int lpcnet_batch_dred_enc_set_state(LPCNetBatch *b, int stream, const float *in);
LPCNET_EXPORT int lpcnet_batch_dred_enc_set_form(LPCNetBatch *b, int S);
LPCNET_EXPORT int lpcnet_batch_dred_enc_get_form(const LPCNetBatch *b, int n_streams);
LPCNET_EXPORT int lpcnet_batch_dred_enc_set_fast(LPCNetBatch *b, int mode);
LPCNET_EXPORT int lpcnet_batch_dred_enc_get_fast(const LPCNetBatch *b);
/* a blob's DRED encoder as the loader sees it, no device: info[15] = {present (0 none, 1 float arrays, 2 int8 arrays, -1 incomplete or inconsistent),
 * servable (dred_enc_enable accepts the blob: the arrays are in the LPCNet model's own flavour), latent dimension, state dimension, K, width of gdense1, floats of one stream's state, the widths of
 * enc_dense1 .. enc_dense8}.  Returns like lpcnet_hip_dred_model_info */
LPCNET_EXPORT int lpcnet_hip_dred_enc_model_info(const unsigned char *data, int len, int *info);

/* State interchange with the single-stream API (PLC-style snapshot / rollback). */
LPCNET_EXPORT int lpcnet_batch_export_state(LPCNetBatch *b, int stream, LPCNetState *st);
LPCNET_EXPORT int lpcnet_batch_import_state(LPCNetBatch *b, int stream, const LPCNetState *st);

/* Tuning / introspection */
LPCNET_EXPORT int lpcnet_batch_set_streams_per_workgroup(LPCNetBatch *b, int s);      /* 1, 2, 4, 8; 0 = auto.  8 = the two-group kernel (float blobs with a dense GRU-B matrix and
                                                                                        * <= 32 GRU-A items per lane, bit-exact arithmetic): chosen automatically beyond four streams per CU.
                                                                                        * Models of 33 .. 96 items per lane: after lpcnet_batch_set_two_group_streaming(b, 1).
                                                                                        * FAST fp32 arithmetic: after lpcnet_batch_set_fast_two_group(b, 1); without it a pinned
                                                                                        * eight runs at four while FAST is on */
LPCNET_EXPORT int lpcnet_batch_get_streams_per_workgroup(const LPCNetBatch *b);
/* Which form of the two-group kernel runs at eight streams per workgroup: 0 = eight waves (two per SIMD), 1 = twelve waves (three per SIMD; needs the
 * model's twelve-wave image: an error without it), -1 = as measured / as the table says.  Both forms produce the same bits.  get: what a launch of the
 * whole batch runs now (0 / 1). */
LPCNET_EXPORT int lpcnet_batch_set_twelve_waves(LPCNetBatch *b, int mode);
LPCNET_EXPORT int lpcnet_batch_get_twelve_waves(const LPCNetBatch *b);
/* The two-group kernel for models of 33 .. 96 GRU-A items per lane (heavy-tailed, trained-like sparsity): its streamed variants keep 24 items of a
 * lane in registers and fetch the others from L2 every sample.  Off by default; a batch that does not ask behaves as before.  on = 1 waits for
 * enqueued work, uploads the model's wide image once, and from then on this batch treats eight streams per workgroup like any two-group model: the
 * value may be pinned, lpcnet_batch_tune and the first host-pointer call measure it, the group schedule may answer it.  The cost table alone never
 * chooses eight for such a model.  Same bits as the four-stream kernel.  FAST arithmetic under a pinned eight runs at four (the streamed variants have no
 * FAST form, lpcnet_batch_set_fast_two_group refuses such a model); the twelve-wave form stays unavailable.  on = 0 puts the batch back on the four-stream kernel (LPCNET_HIP_E_ARG while eight is pinned).
 * A model that has the ordinary two-group image: returns 0 and changes nothing.  int8 blobs, a block-sparse GRU-B matrix, more than 96 items:
 * LPCNET_HIP_E_MODEL with a message, setting unchanged.  LPCNET_HIP_X2_STREAMED=1, read when a batch is created, switches it on where the model allows. */
LPCNET_EXPORT int lpcnet_batch_set_two_group_streaming(LPCNetBatch *b, int on);
LPCNET_EXPORT int lpcnet_batch_get_two_group_streaming(const LPCNetBatch *b);
/* The two-group kernel under FAST fp32 arithmetic (lpcnet_batch_set_fast(b, 1)): GRU-A's items accumulate on the matrix pipe, every activation is the
 * hardware exp2 / rcp, the sampling tree's terms are fused; GRU-B's chains keep their separately rounded sums.  Off by default; a batch that does not
 * ask behaves as before (FAST runs at up to four streams per workgroup, a pinned eight at four).  on = 1 waits for enqueued work and sets the switch
 * on every shard; it may be set while PARITY is active and takes effect whenever FAST = 1 is on: eight streams per workgroup may then be pinned, and
 * the cost table picks eight at exactly the stream counts where it does under PARITY (beyond four streams per CU) -- FAST is never measured, so its
 * output stays a function of the stream count and this switch, not of timing.  Under PARITY and under FAST = 2 (fp16 dual FC) nothing that runs
 * changes; the twelve-wave form is never chosen under FAST.  Not the bits of the four-stream FAST kernel (another summation order): inside the same
 * teacher-forced envelope (tests/test_gpu_x2_fast.py).  on = 0 puts the batch back (LPCNET_HIP_E_ARG while FAST is on and eight is pinned).
 * int8 blobs, a block-sparse GRU-B matrix, a model whose two-group image is the wide one (33 .. 96 items per lane) or absent: LPCNET_HIP_E_MODEL with
 * a message, setting unchanged.  LPCNET_HIP_X2_FAST=1, read when a batch is created, switches it on where the model allows. */
LPCNET_EXPORT int lpcnet_batch_set_fast_two_group(LPCNetBatch *b, int on);
LPCNET_EXPORT int lpcnet_batch_get_fast_two_group(const LPCNetBatch *b);
/* The group schedule: how the compacted groups of a PLC step or a per-stream step (lpcnet_batch_synthesize_step) are launched.  Off by default.
 * form: 0 = groups launch in the batch's form (default), 1 = in the cost table's form for the group's own size -- while the streams per
 *   workgroup are not pinned and the arithmetic is bit-exact, where every form gives the same samples; a pinned value and FAST keep the batch's form.
 * lanes: 1 (default) .. 4: groups that name disjoint streams are enqueued on up to three streams of the batch's own beside the caller's and
 *   joined into the caller's stream before the call returns or reaches a launch on the whole batch: the ordering rules above do not change.
 * LPCNET_HIP_E_ARG otherwise, with the setting unchanged.  Waits for enqueued work.  Every shard gets the same setting; the output does not
 * depend on it. */
LPCNET_EXPORT int lpcnet_batch_set_group_schedule(LPCNetBatch *b, int form, int lanes);
LPCNET_EXPORT int lpcnet_batch_get_group_schedule(const LPCNetBatch *b, int *form, int *lanes);
/* streams per workgroup a group of cnt streams (1 .. the streams of shard 0) launches with under the present settings (no device work) */
LPCNET_EXPORT int lpcnet_batch_group_form(const LPCNetBatch *b, int cnt);
/* the groups of the most recent plc_step / synthesize_step of shard 0:
 * rec[k] = {lane, slot, cnt, kind, N, preload, streams per workgroup, workgroups}; returns their number (at most `cap` are written) */
LPCNET_EXPORT int lpcnet_batch_last_groups(const LPCNetBatch *b, int *rec, int cap);
/* Streams per workgroup are measured on the batch itself (PARITY arithmetic; FAST takes a table value so that its output
 * never depends on timing): lpcnet_batch_tune() does it now, on the engine's own stream (~10 ms).  Without it the first
 * host-pointer call measures; the enqueue-only *_device calls on a caller's stream never do (they use the table value). */
LPCNET_EXPORT int lpcnet_batch_tune(LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_enable_timing(LPCNetBatch *b, int on);
LPCNET_EXPORT int lpcnet_batch_last_timing(LPCNetBatch *b, float *ms_sample_kernel, float *ms_frame_kernels);
LPCNET_EXPORT const char *lpcnet_batch_last_error(void);

/* Parity seams used by the test-suite (SURVEY.md §7 hard part 9): the two halves of the path alone.
 *   tail:   sample loop only, frame products given: cond_a [n][T][1152], cond_b [n][T][48], lpc [n][T][16]
 *   frames: frame network + LPC only, products returned in the same layouts (any may be NULL)
 *   decode: the packet unpacker only (decode_packet + the double interpolation), launched as lpcnet_batch_decode launches it: packets
 *           [n][n_packets][8] -> features [n][4 n_packets][20] (the row stride is fixed at 20: cepstrum [0..17], pitch [18], correlation [19]).
 *           Advances the decoder's VQ memory and nothing else: the synthesis state, the kept frame products and whether they exist stay as they
 *           were.  LPCNET_HIP_E_ARG for n_packets <= 0 or a NULL pointer, LPCNET_HIP_E_MODEL without a model or without codebooks. */
LPCNET_EXPORT int lpcnet_batch_run_tail(LPCNetBatch *b, const float *cond_a, const float *cond_b, const float *lpc,
                                        short *pcm, int n_frames, int preload);
LPCNET_EXPORT int lpcnet_batch_run_frames(LPCNetBatch *b, const float *features, int feat_stride,
                                          float *cond_a, float *cond_b, float *lpc, int n_frames);
LPCNET_EXPORT int lpcnet_batch_run_decode(LPCNetBatch *b, const unsigned char *packets, float *features, int n_packets);
/* tools: the single-stream unpacker on the host (what lpcnet_decode runs before it synthesises; no device work): one 8-byte packet and the
 * stream's VQ memory [18] (in and out) -> features [4][36] with the installed codebooks.  LPCNET_HIP_E_ARG for a NULL pointer,
 * LPCNET_HIP_E_MODEL without codebooks. */
LPCNET_EXPORT int lpcnet_hip_packet_features(const unsigned char *buf8, float *vq_mem18, float *features4x36);
/* tools: GRU-A row dealing of a blob (out[65]: items per lane, then per wave bound[4] + candidate-only flags[3], then
 * per wave the number of early head items of slot 0) */
LPCNET_EXPORT int lpcnet_hip_model_layout(const unsigned char *data, int len, int *out);
/* the engine's own correctly rounded 10^x of the LPC path (pow(10.f, x) of src/freq.c:317) evaluated on the device */
LPCNET_EXPORT int lpcnet_hip_exp10_device(const float *x, double *out, int n);
/* The arithmetic identities the bit-exact (PARITY) kernels rest on, evaluated on the device with the library's own compile flags
 * and float mode, as bit patterns: v_mfma_f32_4x4x1(A, B, C = -0.0) == v_mul_f32 (out_mfma / out_mul, [n][4]: product k of lane i =
 * a[4*(i/4) + k] * b[i]) and the halves of v_pk_mul_f32 / v_pk_add_f32 == v_mul_f32 / v_add_f32 (out_pk / out_sc, [n][4] =
 * {mul (a[i], b[i]), mul (a[i^1], b[i^1]), add (a[i], b[i]), add (a[i^1], b[i^1])}).  n a multiple of 64.
 * tests/test_gpu_parity.py::test_matrix_pipe_multiplier_and_packed_math_are_exact feeds it stratified operands (subnormal
 * inputs and products, underflow, +-0, the largest finite products, infinities). */
LPCNET_EXPORT int lpcnet_hip_arith_identities_device(const float *a, const float *b, unsigned *out_mfma, unsigned *out_mul,
                                                     unsigned *out_pk, unsigned *out_sc, int n);
/* The int8 kernels re-quantise the GRU states with ONE instruction (v_cvt_rpi_i32_f32) where the reference evaluates
 * (int)floor(.5 + 127 x) with the sum in double (src/vec.h:311-316): this runs both over ALL 2^32 float bit patterns on the device.
 * out3 = {mismatches among finite |t| < 2^31, mismatches inside the reachable |t| <= 127.5, one mismatching pattern}. */
LPCNET_EXPORT int lpcnet_hip_quant_sweep_device(unsigned long long *out3);
/* Streams that come and go.  A batch is a CAPACITY of n streams; of shard k's count_k streams the first active_k are ACTIVE, 0 <= active_k <=
 * count_k (default: all).  A batch that never calls lpcnet_batch_set_active runs exactly what it ran before these functions existed.
 * set_active: active[k] for every shard (n_shards must equal lpcnet_batch_shards(b)); host-only, no wait, no device work: it takes effect for
 *   calls enqueued after it, calls already enqueued keep the count they were enqueued with.  A count beyond its shard's streams is
 *   LPCNET_HIP_E_ARG and no shard has changed.  get_active returns the number of shards, active_streams the sum of the counts.
 * Which calls follow the prefix: every call that ADVANCES streams acts on the active streams only -- the host-pointer, device-pointer and _shard
 *   forms of synthesize, synthesize_preload, synthesize_step, decode, analyze(_float), encode, compute_features, plc_step and plc_fec_feed, and
 *   the parity seams run_tail / run_frames / run_decode / plc_burg / plc_pred.  Array layouts do not change: host arrays stay [n_streams][...], a shard's device
 *   arrays [count_k][...]; the rows of inactive streams are neither read nor written, and every byte of an inactive stream's states stays as it
 *   was (synthesis, decoder VQ, analysis, encoder VQ and PLC states, the PLC's control state, the kept frame products and whether they exist).
 *   lost[s], clear[s], skip[s] and mode[s] / n_samples[s] / preload[s] of an inactive stream are ignored; dropped[s] is written 0; a non-zero
 *   count[s] of an inactive stream in plc_fec_feed* is LPCNET_HIP_E_ARG with nothing changed (the packed array would be ambiguous).
 *   A shard with active_k == 0 launches nothing and the call returns 0.
 * Per-stream maintenance calls work on ANY stream of the capacity, active or not -- that is how a joining stream is prepared: reset,
 *   analysis_reset, plc_reset, get / set_*_state, get / set_*_vq_mem, export / import_state, plc_fec_add / plc_fec_clear, copy_streams.
 * The sample kernel's form on a prefix: with active_k == count_k what the batch runs anyway (a measured value and the twelve-wave form
 *   included).  With active_k < count_k a pinned streams-per-workgroup value holds; otherwise the launch takes the cost table's form for
 *   active_k streams, as lpcnet_batch_group_form answers for a group; the twelve-wave form is never used and nothing is measured inside a call
 *   (lpcnet_batch_tune keeps measuring the full capacity).  PARITY gives the same bits in every form.  FAST output is a function of the ACTIVE
 *   count and the batch's switches: it equals what a batch of active_k streams with those switches gives.
 * copy_streams: stream src[i] -> stream dst[i], i < m: EVERYTHING the batch keeps per stream that is allocated at the time of the call -- the
 *   synthesis state, the decoder's and the encoder's VQ memory, the analysis state, the kept frame products and whether they exist, every
 *   per-stream array of the PLC and its control state.  All dst distinct, no stream in both lists (a source may feed several destinations),
 *   every index inside the capacity: else LPCNET_HIP_E_ARG and nothing has changed.  Pairs inside one shard: one upload of the pair list and ONE
 *   launch per shard, only enqueued on hip_stream (NULL = the batch's own; on a sharded batch it must be NULL) under the ordering rules of
 *   lpcnet_batch_analyze_device; LPCNET_HIP_E_ARG on a capturing stream.  The host halves (PLC control state, the products' flag) are copied
 *   when the call is made, which is when the planners of the steps run too: call order is the order.  Pairs ACROSS shards are grouped by
 *   (source shard, destination shard) and move like copy_streams_to below: one gather, one transfer and one scatter per shard pair, only enqueued.
 * A stream leaves by copying the last active stream of its shard into its slot and lowering the count; a stream joins by reset (and
 *   analysis_reset / plc_reset where used) of the slot at the count and raising it.  lpcnet_amd/roster.py (StreamRoster) keeps that book. */
LPCNET_EXPORT int lpcnet_batch_set_active(LPCNetBatch *b, const int *active, int n_shards);
LPCNET_EXPORT int lpcnet_batch_get_active(const LPCNetBatch *b, int *active, int cap);
LPCNET_EXPORT int lpcnet_batch_active_streams(const LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_copy_streams(LPCNetBatch *b, const int *src, const int *dst, int m, void *hip_stream);
/* the decoder's per-stream VQ memory (float[18]; zero after lpcnet_batch_reset): with it a per-stream snapshot covers every state of a stream */
LPCNET_EXPORT int lpcnet_batch_get_decoder_vq_mem(LPCNetBatch *b, int stream, float *out18);
LPCNET_EXPORT int lpcnet_batch_set_decoder_vq_mem(LPCNetBatch *b, int stream, const float *in18);
/* Stream snapshots: m streams' complete records to or from one contiguous buffer, in one launch per shard.
 * A RECORD is everything copy_streams moves, laid end to end: every per-stream array that is allocated at the time of the call is one SECTION, in
 *   the order of the ids below, each on a 16-byte boundary, its bytes the device array's; the PLC's control ints (LPCNET_SNAP_PLC_CTL, 9 ints, with
 *   PLC enabled) and the kept products' flag (LPCNET_SNAP_KEEP_FLAG, 1 int, always) are sections too.  The record length is a multiple of 16.
 * snapshot_layout: the batch's present section table, sections [k][3] = {id, bytes per stream, offset in the record} (entries beyond `cap` rows are
 *   not written) and the record length; returns k.  snapshot_bytes: the size of a host blob of m streams with that layout (0 without a model).
 * snapshot: the records of streams[0 .. m) (distinct, any stream of the capacity) as a host BLOB: header ("LPCS", version, m), the layout -- record
 *   length, sections, the blob's flavour, the PLC options and widths, the DRED encoder's record length, this library's state_size /
 *   analysis_state_size / plc_state_size and a 64-bit hash of the model blob (information only) --, meta [m][LPCNET_SNAP_META] ints (the host halves),
 *   m records.  Copies out and synchronises; LPCNET_HIP_E_ARG when cap is below snapshot_bytes(b, m).  buf must be 4-byte aligned.
 * restore: record i of the blob -> stream streams[i], i < m (m at most the blob's count: the first m records; streams distinct).  The blob's layout
 *   must MATCH the batch: a section on both sides has equal bytes; another flavour, PLC on one side only or with other options or widths, and a blob
 *   of a build with other struct sizes are LPCNET_HIP_E_MODEL with a message that names the section; a section only the snapshot has makes the host
 *   form enable that subsystem in the batch first (analysis, encoder, kept products, DRED encoder, the DRED decoder's record in a batch that has
 *   dred_enable'd -- one that has not is LPCNET_HIP_E_MODEL: max_latents is the batch's to say -- as copy_streams across shards does); a section
 *   only the batch has receives a fresh stream's record (zeros, a reset control state, flag 0).  A NULL, truncated or inconsistent blob is
 *   LPCNET_HIP_E_ARG.  On any refusal nothing has changed.  On a sharded batch both host forms run one host thread per shard.
 * snapshot_device / restore_device: the same on device memory, ONE upload of the list and ONE launch, only enqueued on hip_stream (NULL = the batch's
 *   own) under the ordering rules of lpcnet_batch_analyze_device; LPCNET_HIP_E_ARG on a capturing stream.  d_records holds m records of the batch's
 *   present layout (16-byte aligned); meta [m][LPCNET_SNAP_META] is a HOST array: snapshot_device has filled it when it returns, restore_device reads
 *   it when it is called -- the host halves move when the call is made, which is when the planners of the steps run too: call order is the order, as
 *   for copy_streams.  restore_device takes the section table the records were written with ([n_sections][3]); flavour and PLC options do not travel
 *   in it, and a section only the snapshot has is LPCNET_HIP_E_MODEL here (nothing is allocated).  Neither call allocates after the batch's first
 *   snapshot or copy, waits for enqueued work or changes the active counts.  The forms without _shard need a batch of one shard.
 * copy_streams_to: stream src[i] of `from` -> stream dst[i] of `to`, i < m (src distinct, dst distinct; the two batches differ): a snapshot of
 *   `from` and a restore into `to` through staging buffers the library owns, shard pair by shard pair.  On one device: a gather on the source's
 *   stream, a scatter on the destination's behind an event -- no host hop, no wait.  On two devices: gather, one device-to-device copy (one bounce
 *   of the whole buffer through pinned host memory where the devices cannot reach each other), scatter.  Only enqueued; `from` is unchanged; missing
 *   subsystems are enabled in `to` as restore does.  Ordering as copy_streams: the host halves move when the call is made. */
#define LPCNET_SNAP_SYNTH      1
#define LPCNET_SNAP_DEC_VQ     2
#define LPCNET_SNAP_AN         3
#define LPCNET_SNAP_ENC_VQ     4
#define LPCNET_SNAP_KEEP_A     5
#define LPCNET_SNAP_KEEP_B     6
#define LPCNET_SNAP_KEEP_LPC   7
#define LPCNET_SNAP_KEEP_FLAG  8
#define LPCNET_SNAP_PLC_Q      9
#define LPCNET_SNAP_PLC_FEAT  10
#define LPCNET_SNAP_PLC_NET   11
#define LPCNET_SNAP_PLC_DC    12
#define LPCNET_SNAP_PLC_DELTA 13
#define LPCNET_SNAP_PLC_FEC   14
#define LPCNET_SNAP_PLC_FBUF  15
#define LPCNET_SNAP_PLC_LP    16
#define LPCNET_SNAP_PLC_BURG  17
#define LPCNET_SNAP_PLC_AN    18
#define LPCNET_SNAP_PLC_CTL   19
#define LPCNET_SNAP_DRED_ENC  20
#define LPCNET_SNAP_DRED_DEC  21      /* the DRED decoder's per-stream record (lpcnet_batch_dred_state_enable): present when the batch has it */
#define LPCNET_SNAP_META      10      /* ints of a stream's host halves: the PLC's nine control ints (zero without PLC), the kept products' flag */
#define LPCNET_SNAP_CONFIG    10      /* ints of a configuration, below */
#define LPCNET_SNAP_LAYOUT_INTS 92    /* the most ints a layout has: 14 head fields and 26 sections */
LPCNET_EXPORT int    lpcnet_batch_snapshot_layout(const LPCNetBatch *b, int *sections, int cap, int *record_bytes);
LPCNET_EXPORT size_t lpcnet_batch_snapshot_bytes(const LPCNetBatch *b, int m);
LPCNET_EXPORT int    lpcnet_batch_snapshot(LPCNetBatch *b, const int *streams, int m, void *buf, size_t cap);
LPCNET_EXPORT int    lpcnet_batch_restore(LPCNetBatch *b, const int *streams, int m, const void *buf, size_t len);
LPCNET_EXPORT int    lpcnet_batch_snapshot_device(LPCNetBatch *b, const int *streams, int m, void *d_records, int *meta, void *hip_stream);
LPCNET_EXPORT int    lpcnet_batch_restore_device(LPCNetBatch *b, const int *streams, int m, const void *d_records, const int *meta,
                                                 const int *sections, int n_sections, void *hip_stream);
/* ... on ONE shard of a sharded batch: the shard's own stream indices, pointers on the shard's device */
LPCNET_EXPORT int    lpcnet_batch_snapshot_device_shard(LPCNetBatch *b, int shard, const int *streams, int m, void *d_records, int *meta, void *hip_stream);
LPCNET_EXPORT int    lpcnet_batch_restore_device_shard(LPCNetBatch *b, int shard, const int *streams, int m, const void *d_records, const int *meta,
                                                       const int *sections, int n_sections, void *hip_stream);
LPCNET_EXPORT int    lpcnet_batch_copy_streams_to(LPCNetBatch *from, const int *src, LPCNetBatch *to, const int *dst, int m);
/* Without a device.  snapshot_layout: config [LPCNET_SNAP_CONFIG] = {int8 blob, analysis, encoder, kept products, PLC, PLC options, PLC widths g1, g2,
 * floats of the DRED encoder's record (0: not enabled), its max_dframes} -> out [k][3] as above, then the record length in out[3 k] where cap (ints)
 * allows; returns k.  (A configuration describes a batch without the DRED decoder's record: LPCNET_SNAP_DRED_DEC has no field of its own, in a
 * configuration or in a layout's head -- a batch's own snapshot_layout reports the section, whose size says what it holds.)  snapshot_info: a blob's header and layout, info = {version, m, record bytes, sections k, flavour, PLC, PLC options, g1, g2,
 * DRED encoder floats, its max_dframes, state_size, analysis_state_size, plc_state_size, hash low, hash high, k x {id, bytes, offset}}; returns the
 * ints written (at most cap), LPCNET_HIP_E_ARG for a NULL, truncated, wrong-magic or wrong-version buffer or one whose lengths do not add up.
 * snapshot_match: would a snapshot of config_snap restore into a batch of config_batch?  0 yes; 1 yes in the host form, which enables the missing
 * subsystem first (with enqueue_only != 0 that is a refusal); LPCNET_HIP_E_MODEL no, *section (may be NULL) the section the message names. */
LPCNET_EXPORT int    lpcnet_hip_snapshot_layout(const int *config, int *out, int cap);
LPCNET_EXPORT int    lpcnet_hip_snapshot_info(const void *buf, size_t len, int *info, int cap);
LPCNET_EXPORT int    lpcnet_hip_snapshot_match(const int *config_snap, const int *config_batch, int enqueue_only, int *section);
/* raw per-stream state record (layout = struct lpcn_stream_state in lpcnet_amd/csrc/lpcnet_engine.h) */
LPCNET_EXPORT int lpcnet_batch_state_size(void);
LPCNET_EXPORT int lpcnet_batch_get_raw_state(LPCNetBatch *b, int stream, void *out);
LPCNET_EXPORT int lpcnet_batch_set_raw_state(LPCNetBatch *b, int stream, const void *in);
LPCNET_EXPORT int lpcnet_batch_debug_trace(LPCNetBatch *b, int n_samples, float *host_out);
/* shader-clock totals per phase of the sample kernel (workgroup 0): out == NULL enables/zeros, else 8 values */
LPCNET_EXPORT int lpcnet_batch_profile(LPCNetBatch *b, unsigned long long *out);

#ifdef __cplusplus
}
#endif
#endif
