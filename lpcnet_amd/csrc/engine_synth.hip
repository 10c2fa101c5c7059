// Synthesis: which sample kernel a launch gets and its launch, the frame kernels' launch, the streams-per-workgroup measurement, the run
// entry points, the legacy combined pass and the codec decode path.  Owns frame_kernels.hip.h, decode_kernel.hip.h and lpcn_set_args_kernel.
#include "engine_core.h"
#include "sample_variants.h"
#include "frame_kernels.hip.h"
#include "decode_kernel.hip.h"

// HIP-graph capture: a captured copy node re-reads its HOST source at every replay, so the argument block of a captured launch cannot come from the
// caller's stack -- it travels as the by-value parameter of a one-lane kernel instead, which the graph's kernel node owns (round 6, ADVICE r5: round 5's
// pinned pool of 32 slots leaked a slot per captured launch and ended every capture after the 32nd)
__global__ void lpcn_set_args_kernel(LpcnSampleArgs *dst, const LpcnSampleArgs a) { *dst = a; }

// ------------------------------------------------------------------------------- launches -----
// The sample kernel's variants (streams per workgroup x items per lane x blob flavour x arithmetic) are compiled in
// separate translation units, one per streams-per-workgroup value (sample_variants.hip), so they build in parallel.
extern "C" int lpcn_launch_sample_s1(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);
extern "C" int lpcn_launch_sample_s2(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);
extern "C" int lpcn_launch_sample_s4(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);
extern "C" int lpcn_launch_sample_x2(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);      // sample_x2.hip: two groups of four streams
extern "C" int lpcn_launch_sample_x2w(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);     // sample_x2w.hip: its streamed variants (more than 32 items per lane)
extern "C" int lpcn_launch_sample_x2f(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);     // sample_x2f.hip: its register-resident variants with FAST fp32 arithmetic
extern "C" int lpcn_x2_lds_bytes(int nb_b);
extern "C" int lpcn_launch_sample_x3(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args);      // sample_x3.hip: the same on twelve waves (same LDS layout, its own cells behind it)
extern "C" int lpcn_x3_lds_bytes(int nb_b);

// What a whole-batch call launches: every stream in the batch's form -- or, on an active prefix shorter than the batch, streams [0, active) in a
// pinned form, else the cost table's form for that many streams (as a compacted group gets: a table look-up, never a measurement), never on twelve
// waves.  PARITY gives the same bits in every form; FAST output is that of a batch of `active` streams with the same switches.
static LaunchShape whole_batch(const lpcn_batch_dev *b)
{
    if (b->active == b->n) return {b->n, b->frame_len, b->d_state, b->S, b->pack2, b->x3};
    const int S = b->S_auto ? auto_streams_per_wg(b, b->active) : b->S;
    return {b->active, b->frame_len, b->d_state, S, use_pack2(b, b->active, S), false};
}

SamplePlan plan_sample(const lpcn_batch_dev *b, const LaunchShape &sh, int n_frames)
{
    const lpcn_engine *e = b->e;
    SamplePlan p{sh.S, sh.pack2, false, nullptr, 0, 0};
    // Eight streams per workgroup become four (a) while the two-group kernel is unavailable (the arithmetic flavour changed under a pinned value and the
    // batch has not asked for the kernel's FAST form, or the flavour is FAST with the fp16 dual FC) and
    // (b) for a launch with 4 GB or more of conditioning rows -- more than ~9 300 streams x 100 frames -- which the two-group kernel, addressing them
    // with 32-bit byte offsets, cannot reach
    if (sh.S == 8 && (!x2_available(b) || (unsigned long long)sh.n * (unsigned long long)n_frames * LPCN_ROWS_A * 4ull >= (1ull << 32))) { p.S = 4; p.pack2 = false; }
    p.x3 = p.S == 8 && sh.x3 && x3_available(b);
    p.image = p.x3 ? &e->image[IMG_X3] : &gru_a_image(e, p.S);
    p.lds = p.x3 ? lpcn_x3_lds_bytes(e->nb_b) : p.S == 8 ? lpcn_x2_lds_bytes(e->nb_b) : p.S == 1 ? lpcn::Lds<1>::total(e->nb_b, e->is_int8) : p.S == 2 ? lpcn::Lds<2>::total(e->nb_b, e->is_int8) : lpcn::Lds<4>::total(e->nb_b, e->is_int8);
    p.grid = (sh.n + p.S - 1) / p.S;
    return p;
}
// (what a whole-batch launch of one frame runs with: four while FAST arithmetic is on under a pinned eight, unless the batch opted in -- x2_fast)
extern "C" int lpcn_batch_dev_streams_per_wg(const lpcn_batch_dev *b) { return plan_sample(b, whole_batch(b), 1).S; }
extern "C" int lpcn_batch_dev_x3(const lpcn_batch_dev *b) { return plan_sample(b, whole_batch(b), 1).x3 ? 1 : 0; }

// one chunk of the per-sample kernel; cond_a/cond_b/lpc for the chunk are already in the batch buffers
int launch_sample(lpcn_batch_dev *b, const LaunchShape &sh, hipStream_t st, short *d_pcm, size_t pcm_stride, int n_frames, int preload, bool fc_from_frames)
{
    const lpcn_engine *e = b->e;
    const SamplePlan p = plan_sample(b, sh, n_frames);
    const int nw = p.image->nw_variant;
    LpcnSampleArgs a = p.image->args;
    a.n_streams = sh.n; a.n_frames = n_frames; a.preload = preload; a.frame_len = sh.frame_len;
    a.fc_advance = fc_from_frames ? 1 : 0;
    a.cond_a = b->d_cond_a + (size_t)sh.slot * LPCN_ROWS_A; a.cond_b = b->d_cond_b + (size_t)sh.slot * LPCN_ROWS_B; a.lpc = b->d_lpc + (size_t)sh.slot * LPCN_LPC_ORDER;
    a.fc_base = fc_from_frames ? b->d_fc_base + sh.slot : nullptr;
    a.pcm = d_pcm; a.pcm_stride = (long long)pcm_stride;
    a.state = sh.d_state; a.dbg = b->d_dbg; a.prof = b->d_prof;
    a.fc_f16 = (e->fast && e->fc_f16) ? 1 : 0;
    if ((size_t)sh.arg >= b->d_args.cap) { snprintf(g_err, sizeof(g_err), "sample launch: the step's launches exceed their argument records"); return LPCN_E_HIP; }
    LpcnSampleArgs *d_args = b->d_args + sh.arg;
    // (d_dbg / d_prof are one buffer per batch: the trace and the phase profile are meaningful with one lane only)
    if (stream_is_capturing(st)) {
        hipLaunchKernelGGL(lpcn_set_args_kernel, dim3(1), dim3(1), 0, st, d_args, a);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpyAsync(d_args, &a, sizeof(a), hipMemcpyHostToDevice, st));
    }
    const int i8 = e->is_int8 ? 1 : 0;
    const int flags = (e->fast ? 1 : 0) | (p.pack2 ? 2 : 0);
    int rc = 0;
    switch (p.S) {
    case 8: rc = p.x3 ? lpcn_launch_sample_x3(p.grid, p.lds, st, d_args) : (e->fast ? lpcn_launch_sample_x2f : nw > LPCN_X2_NW_MAX ? lpcn_launch_sample_x2w : lpcn_launch_sample_x2)(nw, p.grid, p.lds, st, d_args); break;
    case 1: rc = lpcn_launch_sample_s1(nw, i8, flags, p.grid, p.lds, st, d_args); break;
    case 2: rc = lpcn_launch_sample_s2(nw, i8, flags, p.grid, p.lds, st, d_args); break;
    default: rc = lpcn_launch_sample_s4(nw, i8, flags, p.grid, p.lds, st, d_args); break;
    }
    if (rc == LPCN_NO_SUCH_VARIANT) { snprintf(g_err, sizeof(g_err), "no compiled sample-kernel variant for %d items per lane at %d streams per workgroup", nw, p.S); return LPCN_E_HIP; }
    if (rc) { snprintf(g_err, sizeof(g_err), "sample kernel launch failed: %s", hipGetErrorString((hipError_t)rc)); return LPCN_E_HIP; }
    return 0;
}

int launch_frames(lpcn_batch_dev *b, const LaunchShape &sh, hipStream_t st, const float *d_feat, int feat_stride, size_t feat_stream_stride, int n_frames)
{
    return lpcn_launch_frame_kernels(b->e->fmodel, st, sh.n, n_frames, d_feat, feat_stride, feat_stream_stride,
                                     sh.d_state, b->d_fc_base + sh.slot, b->d_cond + (size_t)sh.slot * LPCN_COND, b->d_cond_a + (size_t)sh.slot * LPCN_ROWS_A,
                                     b->d_cond_b + (size_t)sh.slot * LPCN_ROWS_B, b->d_lpc + (size_t)sh.slot * LPCN_LPC_ORDER, g_err, sizeof(g_err));
}

// Streams per workgroup, measured instead of looked up (the table in auto_streams_per_wg holds THIS model's step
// times; a denser / sparser blob or another item-count variant has other optima).  Before the first run of a batch whose
// value is not pinned, each candidate S runs live frames on the batch's own buffers -- zeroed frame products, the stream
// states saved and restored around it -- timed with HIP events: a warm-up launch, then one frame and five frames; the
// DIFFERENCE is the steady-state cost of four frames (a launch's prologue -- filling registers and LDS with the weights --
// is ~4 % of a two-frame launch and grows with the workgroup count, which biased a plain two-frame timing against the
// two-workgroups-per-CU form of the int8 kernel).  ~9 launches, ~12 ms, once per batch and arithmetic flavour;
// LPCNET_HIP_NO_AUTOTUNE=1 keeps the table value.
// Round 4: (a) the FAST flavour is never timed -- its float kernels switch GRU-B's algorithm with S (matrix-pipe GEMM at S >= 2,
// fused DPP chains at S = 1: different summation orders), so a measured S would make FAST output depend on timing noise;
// it takes the table's value, a pure function of (blob kind, stream count, device, the batch's FAST two-group opt-in).  (b) the measurement is the best of
// three timing pairs.  (c) it never runs inside the enqueue-only device-pointer calls on a caller's stream (those take the
// table's value unless lpcnet_batch_tune() has been called): it allocates, synchronises and would break stream capture.
static int autotune_streams_per_wg(lpcn_batch_dev *b, hipStream_t st)
{
    b->tuned = true;
    const char *off = getenv("LPCNET_HIP_NO_AUTOTUNE");
    if ((off && *off == '1') || b->n < 2 || b->e->fast) return 0;     // (one stream: one workgroup whatever S is)
    const int nf = 5 < b->max_chunk ? 5 : b->max_chunk;
    int rc = 0;
    DevBuf<lpcn_stream_state> saved;
    DevBuf<short> pcm;                                       // (a buffer of its own: the caller may be holding the staging buffer's address)
    if ((rc = saved.alloc(b->n)) || (rc = pcm.alloc((size_t)b->n * nf * LPCN_FRAME_SIZE))) return rc;
    std::vector<int> fc((size_t)b->n, LPCN_FEATURES_DELAY + 3);                     // every stream live
    if (hipMemcpyAsync(saved, b->d_state, sizeof(lpcn_stream_state) * b->n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemsetAsync(b->d_cond_a, 0, sizeof(float) * (size_t)b->n * nf * LPCN_ROWS_A, st) != hipSuccess ||
        hipMemsetAsync(b->d_cond_b, 0, sizeof(float) * (size_t)b->n * nf * LPCN_ROWS_B, st) != hipSuccess ||
        hipMemsetAsync(b->d_lpc, 0, sizeof(float) * (size_t)b->n * nf * LPCN_LPC_ORDER, st) != hipSuccess ||
        hipMemcpyAsync(b->d_fc_base, fc.data(), sizeof(int) * b->n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { snprintf(g_err, sizeof(g_err), "auto-tune: buffer setup failed"); return LPCN_E_HIP; }
    int best = b->S;
    bool best_x3 = false;
    float best_ms = -1.f;
    // the candidates: S = 1, 2, 4, 8 and -- where eight has won, the model has the image, the choice is the engine's and the batch has more than four streams
    // per CU -- eight on twelve waves (both forms of the two-group kernel produce the same bits: the choice cannot change a result)
    const bool try_x3 = x3_available(b) && b->x3_mode < 0 && b->n > 4 * device_cus(b->e);
    for (int c = 0; c < 5; ++c) {
        const int S = c < 4 ? 1 << c : 8;
        if (S == 8 && (!x2_available(b) || b->n <= 4)) break;
        // The twelve-wave form competes with the eight-wave form only, where that one has won: the two share everything this measurement does not see.
        // What is timed is live frames in steady state; the two-group kernels run a call's silent start-up frames at full price, the others do not.  At
        // 2 560 streams (320 workgroups in two rounds against 640 in three) the twelve-wave form ties with four streams per workgroup on live frames
        // (0.3 - 0.8 % apart, inside the spread) and takes 1.42 x the time on a call of 6 frames from reset (21.5 against 15.1 ms): as one more candidate
        // among all it was taken from batch to batch (round 13), with a margin of 2 % still now and then.
        if (c == 4 && (!try_x3 || best != 8)) break;
        const LaunchShape sh = {b->n, b->frame_len, b->d_state, S, use_pack2(b, b->n, S), c == 4 || (S == 8 && b->x3_mode == 1)};
        float ms = -1.f, ms1 = 0.f;
        for (int pass = 0; pass < 7 && !rc; ++pass) {          // warm-up (1 frame), then three pairs of (1 frame, nf frames): the smallest difference
            const int k = (pass && !(pass & 1)) ? nf : 1;
            float t = 0.f;
            if (hipEventRecord(b->ev[1], st) != hipSuccess) rc = LPCN_E_HIP;
            if (!rc) rc = launch_sample(b, sh, st, pcm, (size_t)nf * LPCN_FRAME_SIZE, k, 0, true);
            if (!rc && (hipEventRecord(b->ev[2], st) != hipSuccess || hipEventSynchronize(b->ev[2]) != hipSuccess ||
                        hipEventElapsedTime(&t, b->ev[1], b->ev[2]) != hipSuccess)) rc = LPCN_E_HIP;
            if (pass & 1) ms1 = t;
            else if (pass) { const float d = nf > 1 ? t - ms1 : t; if (ms < 0.f || d < ms) ms = d; }      // nf - 1 frames in steady state
        }
        if (rc) break;
        if (best_ms < 0.f || ms < best_ms) { best_ms = ms; best = S; best_x3 = sh.x3; }
    }
    // the measurement ran on the real state: put it back
    if (hipMemcpyAsync(b->d_state, saved, sizeof(lpcn_stream_state) * b->n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) rc = rc ? rc : LPCN_E_HIP;
    if (rc) return rc;
    b->S = best; b->pack2 = use_pack2(b, b->n, best);
    if (b->x3_mode < 0) b->x3 = best_x3;
    return 0;
}

// lpcnet_batch_tune(): measure now, on the engine's own stream (e.g. right after lpcnet_batch_load_model), so that the first
// synthesize call -- in particular an enqueue-only one on a caller's stream -- carries no measurement
extern "C" int lpcn_batch_dev_tune(lpcn_batch_dev *b)
{
    DeviceGuard guard(b->e->device);
    if (!b->S_auto) return 0;
    hipStream_t st = b->e->stream;
    int rc = order_begin(b, st);
    if (rc) return rc;
    if ((rc = autotune_streams_per_wg(b, st))) return rc;
    return order_end(b, st);
}

// The measurement before the first run of a batch whose value is not pinned (allocates, synchronises, launches trial kernels).  Only the
// host-pointer entry points call it, on the engine's own stream, and BEFORE they make their launch shape, so that the measuring call itself
// runs on the measured value; the enqueue-only device-pointer entry points never do, whichever stream they name (a NULL hip_stream
// used to select the engine's own stream AND the measurement).
// (never on an active prefix shorter than the batch: nothing is measured inside such a call, lpcn_batch_dev_tune measures the full capacity)
int tune_if_due(lpcn_batch_dev *b, hipStream_t st) { return (b->S_auto && !b->tuned && b->active == b->n) ? autotune_streams_per_wg(b, st) : 0; }

static int run_impl(lpcn_batch_dev *b, const LaunchShape &sh, const float *d_features, int feat_stride, short *d_pcm, int n_frames, int preload, void *hip_stream)
{
    if (n_frames <= 0 || feat_stride < LPCN_NB_FEAT || preload < 0 || preload > LPCN_FRAME_SIZE) {
        snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG;
    }
    if (sh.n < 1) return 0;            // (no active stream: nothing to launch)
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    float tf = 0.f, ts = 0.f;
    { int rco = order_begin(b, st); if (rco) return rco; }
    forget_keep(b);      // (the step call's per-stream frame products are stale now)
    for (int f0 = 0; f0 < n_frames; f0 += b->max_chunk) {
        const int nf = n_frames - f0 < b->max_chunk ? n_frames - f0 : b->max_chunk;
        if (b->timing) HIP_TRY(hipEventRecord(b->ev[0], st));
        int rc = launch_frames(b, sh, st, d_features + (size_t)f0 * feat_stride, feat_stride, (size_t)n_frames * feat_stride, nf);
        if (rc) return rc;
        if (b->timing) HIP_TRY(hipEventRecord(b->ev[1], st));
        rc = launch_sample(b, sh, st, d_pcm + (size_t)f0 * LPCN_FRAME_SIZE, (size_t)n_frames * LPCN_FRAME_SIZE, nf, preload, true);
        if (rc) return rc;
        if (b->timing) {
            HIP_TRY(hipEventRecord(b->ev[2], st));
            HIP_TRY(hipEventSynchronize(b->ev[2]));
            float a = 0.f, c = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, b->ev[0], b->ev[1]));
            HIP_TRY(hipEventElapsedTime(&c, b->ev[1], b->ev[2]));
            tf += a; ts += c;
        }
    }
    if (b->timing) { b->ms_frame = tf; b->ms_sample = ts; }
    return order_end(b, st);
}

extern "C" int lpcn_batch_dev_run(lpcn_batch_dev *b, const float *d_features, int feat_stride,
                                  short *d_pcm, int n_frames, int preload, void *hip_stream)
{
    return run_impl(b, whole_batch(b), d_features, feat_stride, d_pcm, n_frames, preload, hip_stream);
}

// the staging buffers of the host-pointer calls, for at least that many floats of features and samples of PCM
int ensure_staging(lpcn_batch_dev *b, size_t feat_floats, size_t pcm_samples)
{
    const int rc = b->d_feat.reserve(b, feat_floats);
    return rc ? rc : b->d_pcm.reserve(b, pcm_samples);
}

extern "C" int lpcn_batch_dev_run_host(lpcn_batch_dev *b, const float *features, int feat_stride,
                                       short *pcm, int n_frames, int preload)
{
    if (n_frames <= 0) { snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t nfeat = (size_t)b->active * n_frames * feat_stride, npcm = (size_t)b->active * n_frames * LPCN_FRAME_SIZE;      // (the active streams' rows lead the arrays)
    int rc = ensure_staging(b, nfeat, npcm);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;      // the staging buffers may still be read by work on a caller stream
    HIP_TRY(hipMemcpyAsync(b->d_feat, features, nfeat * sizeof(float), hipMemcpyHostToDevice, st));
    if (preload > 0) HIP_TRY(hipMemcpyAsync(b->d_pcm, pcm, npcm * sizeof(short), hipMemcpyHostToDevice, st));
    if ((rc = tune_if_due(b, st))) return rc;
    rc = run_impl(b, whole_batch(b), b->d_feat, feat_stride, b->d_pcm, n_frames, preload, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, npcm * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// Single-stream fast path of the legacy per-frame API (a batch of one stream): one frame-network step + frame_len samples
// with ONE host synchronisation.  The caller's POD state is uploaded only when it differs from the device copy
// (st_in == NULL: the device copy is current); features, state and PCM travel through one pinned buffer.
extern "C" int lpcn_batch_dev_run_single(lpcn_batch_dev *b, const lpcn_stream_state *st_in, const float *feat, short *pcm,
                                         lpcn_stream_state *st_out)
{
    if (b->n != 1) { snprintf(g_err, sizeof(g_err), "run_single needs a batch of one stream"); return LPCN_E_ARG; }
    DeviceGuard guard(b->e->device);
    const size_t off_feat = sizeof(lpcn_stream_state), off_pcm = off_feat + LPCN_NB_FEAT * sizeof(float);
    int rc = ensure_staging(b, LPCN_NB_FEAT, LPCN_FRAME_SIZE);
    if (!rc) rc = b->h_pin.reserve(off_pcm + LPCN_FRAME_SIZE * sizeof(short));
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    unsigned char *pin = (unsigned char *)b->h_pin.p;
    if (st_in) {
        memcpy(pin, st_in, sizeof(*st_in));
        HIP_TRY(hipMemcpyAsync(b->d_state, pin, sizeof(*st_in), hipMemcpyHostToDevice, st));
    }
    memcpy(pin + off_feat, feat, LPCN_NB_FEAT * sizeof(float));
    HIP_TRY(hipMemcpyAsync(b->d_feat, pin + off_feat, LPCN_NB_FEAT * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = tune_if_due(b, st))) return rc;
    rc = run_impl(b, whole_batch(b), b->d_feat, LPCN_NB_FEAT, b->d_pcm, 1, 0, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pin, b->d_state, sizeof(lpcn_stream_state), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pin + off_pcm, b->d_pcm, LPCN_FRAME_SIZE * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    b->pending = false;
    memcpy(st_out, pin, sizeof(*st_out));
    memcpy(pcm, pin + off_pcm, (size_t)b->frame_len * sizeof(short));
    return 0;
}

// Combined pass of the legacy per-frame API (api.c: callers of one model that arrive while a pass is in flight are served together):
// k <= capacity independent streams, each with its caller's POD state -- states up, kernels, states and results down, ONE
// synchronisation.  The batch was created with the capacity as its stream count; a pass uses its first k slots.  `kind`:
//   LPCN_GROUP_FRAME_SAMPLES  frame network on feat[i] + frame_len samples (lpcnet_synthesize / lpcnet_synthesize_impl, src/lpcnet.c:273-281);
//                             the first `preload` samples of pcm[i] are imposed (teacher forcing); the frame products come back in
//                             ga[i] / gb[i] (the reference keeps them in the state for a later tail call; lpc is part of the state record)
//   LPCN_GROUP_TAIL           frame_len samples from the caller's products ga[i] / gb[i] / lpc[i] (lpcnet_synthesize_tail_impl, :235-271)
//   LPCN_GROUP_FRAMES         frame network only; products returned in ga[i] / gb[i] / lpc[i] (run_frame_network, :82-120)
// Nothing is written to the callers' memory unless the whole pass succeeded.
extern "C" int lpcn_batch_dev_run_group(lpcn_batch_dev *b, int k, int kind, int frame_len, int preload, const lpcn_stream_state *const *st_in,
                                        const float *const *feat, short *const *pcm, lpcn_stream_state *const *st_out,
                                        float *const *ga, float *const *gb, float *const *lpc)
{
    const bool samples = kind != LPCN_GROUP_FRAMES, frames = kind != LPCN_GROUP_TAIL;
    if (k < 1 || kind < 0 || kind > 2 || (samples && (frame_len < 1 || frame_len > LPCN_FRAME_SIZE || preload < 0 || preload > frame_len))) {
        snprintf(g_err, sizeof(g_err), "bad group arguments"); return LPCN_E_ARG;
    }
    DeviceGuard guard(b->e->device);
    const int cap = b->n;
    if (k > cap) { snprintf(g_err, sizeof(g_err), "group of %d exceeds the batch's %d streams", k, cap); return LPCN_E_ARG; }
    // pinned staging: states | features | pcm | cond_a | cond_b | lpc, each for `cap` streams
    const size_t sz_st = sizeof(lpcn_stream_state), off_feat = sz_st * cap, off_pcm = off_feat + sizeof(float) * LPCN_NB_FEAT * cap;
    const size_t off_ga = off_pcm + sizeof(short) * LPCN_FRAME_SIZE * cap, off_gb = off_ga + sizeof(float) * LPCN_ROWS_A * cap;
    const size_t off_lpc = off_gb + sizeof(float) * LPCN_ROWS_B * cap, pin_bytes = off_lpc + sizeof(float) * LPCN_LPC_ORDER * cap;
    int rc = ensure_staging(b, (size_t)cap * LPCN_NB_FEAT, (size_t)cap * LPCN_FRAME_SIZE);
    if (!rc) rc = b->h_pin.reserve(pin_bytes);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    unsigned char *pin = (unsigned char *)b->h_pin.p;
    for (int i = 0; i < k; ++i) {
        memcpy(pin + sz_st * i, st_in[i], sz_st);
        if (frames) memcpy(pin + off_feat + sizeof(float) * LPCN_NB_FEAT * i, feat[i], sizeof(float) * LPCN_NB_FEAT);
        if (samples && preload > 0) memcpy(pin + off_pcm + sizeof(short) * LPCN_FRAME_SIZE * i, pcm[i], sizeof(short) * (size_t)preload);
        if (kind == LPCN_GROUP_TAIL) {
            memcpy(pin + off_ga + sizeof(float) * LPCN_ROWS_A * i, ga[i], sizeof(float) * LPCN_ROWS_A);
            memcpy(pin + off_gb + sizeof(float) * LPCN_ROWS_B * i, gb[i], sizeof(float) * LPCN_ROWS_B);
            memcpy(pin + off_lpc + sizeof(float) * LPCN_LPC_ORDER * i, lpc[i], sizeof(float) * LPCN_LPC_ORDER);
        }
    }
    HIP_TRY(hipMemcpyAsync(b->d_state, pin, sz_st * k, hipMemcpyHostToDevice, st));
    if (frames) HIP_TRY(hipMemcpyAsync(b->d_feat, pin + off_feat, sizeof(float) * LPCN_NB_FEAT * k, hipMemcpyHostToDevice, st));
    if (samples && preload > 0) HIP_TRY(hipMemcpyAsync(b->d_pcm, pin + off_pcm, sizeof(short) * LPCN_FRAME_SIZE * k, hipMemcpyHostToDevice, st));
    if (kind == LPCN_GROUP_TAIL) {     // (one frame per stream: the chunk buffers are dense [stream][...])
        HIP_TRY(hipMemcpyAsync(b->d_cond_a, pin + off_ga, sizeof(float) * LPCN_ROWS_A * k, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_cond_b, pin + off_gb, sizeof(float) * LPCN_ROWS_B * k, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_lpc, pin + off_lpc, sizeof(float) * LPCN_LPC_ORDER * k, hipMemcpyHostToDevice, st));
    }
    const int S = auto_streams_per_wg(b, k);               // (the table's value for the group's size, never a measurement)
    const LaunchShape sh = {k, samples ? frame_len : b->frame_len, b->d_state, S, use_pack2(b, k, S), b->x3_mode == 1};
    forget_keep(b);
    if (kind == LPCN_GROUP_FRAME_SAMPLES) rc = run_impl(b, sh, b->d_feat, LPCN_NB_FEAT, b->d_pcm, 1, preload, st);
    else if (kind == LPCN_GROUP_TAIL) rc = launch_sample(b, sh, st, b->d_pcm, (size_t)LPCN_FRAME_SIZE, 1, preload, false);
    else rc = launch_frames(b, sh, st, b->d_feat, LPCN_NB_FEAT, (size_t)LPCN_NB_FEAT, 1);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pin, b->d_state, sz_st * k, hipMemcpyDeviceToHost, st));
    if (samples) HIP_TRY(hipMemcpyAsync(pin + off_pcm, b->d_pcm, sizeof(short) * LPCN_FRAME_SIZE * k, hipMemcpyDeviceToHost, st));
    if (frames) {
        HIP_TRY(hipMemcpyAsync(pin + off_ga, b->d_cond_a, sizeof(float) * LPCN_ROWS_A * k, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pin + off_gb, b->d_cond_b, sizeof(float) * LPCN_ROWS_B * k, hipMemcpyDeviceToHost, st));
        if (kind == LPCN_GROUP_FRAMES) HIP_TRY(hipMemcpyAsync(pin + off_lpc, b->d_lpc, sizeof(float) * LPCN_LPC_ORDER * k, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    b->pending = false;
    for (int i = 0; i < k; ++i) {
        memcpy(st_out[i], pin + sz_st * i, sz_st);
        // live frames return the imposed samples unchanged; start-up frames are cleared entirely (src/lpcnet.c:239-243)
        if (samples) memcpy(pcm[i], pin + off_pcm + sizeof(short) * LPCN_FRAME_SIZE * i, sizeof(short) * (size_t)frame_len);
        if (frames && ga[i]) {                               // (ga[i] == NULL: this caller does not take the frame products back)
            memcpy(ga[i], pin + off_ga + sizeof(float) * LPCN_ROWS_A * i, sizeof(float) * LPCN_ROWS_A);
            memcpy(gb[i], pin + off_gb + sizeof(float) * LPCN_ROWS_B * i, sizeof(float) * LPCN_ROWS_B);
            if (kind == LPCN_GROUP_FRAMES) memcpy(lpc[i], pin + off_lpc + sizeof(float) * LPCN_LPC_ORDER * i, sizeof(float) * LPCN_LPC_ORDER);
        }
    }
    return 0;
}

// Codec path: 8-byte packets [stream][packet][8] -> 4 frames each.  Device pointers, work only enqueued.
static int decode_impl(lpcn_batch_dev *b, const unsigned char *d_packets, short *d_pcm, int n_packets, void *hip_stream, bool may_tune)
{
    forget_keep(b);
    if (n_packets <= 0) { snprintf(g_err, sizeof(g_err), "bad decode arguments"); return LPCN_E_ARG; }
    if (!b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->e->stream;
    const int T = 4 * n_packets;
    {   // (growing the staging buffer waits for the batch's outstanding work first; it happens once per size)
        int rc = ensure_staging(b, (size_t)b->n * T * LPCN_NB_FEAT, 0);
        if (rc) return rc;
        if ((rc = order_begin(b, st))) return rc;
    }
    hipLaunchKernelGGL(lpcn::decode_kernel, dim3((b->active + 1) / 2), dim3(64), 0, st, b->e->dec, d_packets, b->active, n_packets, b->d_vq_mem,
                       b->d_feat, LPCN_NB_FEAT);
    HIP_TRY(hipGetLastError());
    if (may_tune) { int rct = tune_if_due(b, st); if (rct) return rct; }      // (decode_host only: the engine's own stream)
    return run_impl(b, whole_batch(b), b->d_feat, LPCN_NB_FEAT, d_pcm, T, 0, st);
}
extern "C" int lpcn_batch_dev_decode(lpcn_batch_dev *b, const unsigned char *d_packets, short *d_pcm, int n_packets, void *hip_stream)
{
    return decode_impl(b, d_packets, d_pcm, n_packets, hip_stream, false);
}

extern "C" int lpcn_batch_dev_decode_host(lpcn_batch_dev *b, const unsigned char *packets, short *pcm, int n_packets)
{
    if (n_packets <= 0) { snprintf(g_err, sizeof(g_err), "bad decode arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t nbytes = (size_t)b->active * n_packets * 8, npcm = (size_t)b->active * n_packets * 4 * LPCN_FRAME_SIZE;
    int rc = b->d_packets.reserve(b, nbytes);
    if (rc) return rc;
    if ((rc = ensure_staging(b, 0, npcm))) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_packets, packets, nbytes, hipMemcpyHostToDevice, st));
    rc = decode_impl(b, b->d_packets, b->d_pcm, n_packets, nullptr, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, npcm * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// Parity seam: the unpacker alone.  decode_kernel launched as decode_impl launches it (stride LPCN_NB_FEAT, two streams per workgroup, the active
// count), the staging rows copied back: features [active][4 n_packets][20].  Only the decoder's VQ memory advances: no frame network runs, so the
// synthesis state, the kept frame products and their flag stay (no forget_keep).
extern "C" int lpcn_batch_dev_run_decode_host(lpcn_batch_dev *b, const unsigned char *packets, float *features, int n_packets)
{
    if (n_packets <= 0 || !packets || !features) { snprintf(g_err, sizeof(g_err), "bad decode arguments"); return LPCN_E_ARG; }
    if (!b->e->has_codebooks) { snprintf(g_err, sizeof(g_err), "no VQ codebooks installed (lpcnet_hip_set_codebooks)"); return LPCN_E_MODEL; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t nbytes = (size_t)b->active * n_packets * 8, nfeat = (size_t)b->active * n_packets * 4 * LPCN_NB_FEAT;
    int rc = b->d_packets.reserve(b, nbytes);
    if (rc) return rc;
    if ((rc = ensure_staging(b, nfeat, 0))) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_packets, packets, nbytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lpcn::decode_kernel, dim3((b->active + 1) / 2), dim3(64), 0, st, b->e->dec, b->d_packets, b->active, n_packets, b->d_vq_mem,
                       b->d_feat, LPCN_NB_FEAT);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(features, b->d_feat, nfeat * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_run_tail_host(lpcn_batch_dev *b, const float *cond_a, const float *cond_b,
                                            const float *lpc, short *pcm, int n_frames, int preload)
{
    forget_keep(b);
    if (n_frames <= 0 || preload < 0 || preload > LPCN_FRAME_SIZE) { snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t npcm = (size_t)b->active * n_frames * LPCN_FRAME_SIZE;
    int rc = ensure_staging(b, 0, npcm);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    if ((rc = tune_if_due(b, st))) return rc;
    if (preload > 0) HIP_TRY(hipMemcpyAsync(b->d_pcm, pcm, npcm * sizeof(short), hipMemcpyHostToDevice, st));
    for (int f0 = 0; f0 < n_frames; f0 += b->max_chunk) {
        const int nf = n_frames - f0 < b->max_chunk ? n_frames - f0 : b->max_chunk;
        // gather the chunk [stream][f0..f0+nf) into the dense chunk buffers
        HIP_TRY(hipMemcpy2DAsync(b->d_cond_a, (size_t)nf * LPCN_ROWS_A * 4, cond_a + (size_t)f0 * LPCN_ROWS_A, (size_t)n_frames * LPCN_ROWS_A * 4,
                                 (size_t)nf * LPCN_ROWS_A * 4, b->active, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(b->d_cond_b, (size_t)nf * LPCN_ROWS_B * 4, cond_b + (size_t)f0 * LPCN_ROWS_B, (size_t)n_frames * LPCN_ROWS_B * 4,
                                 (size_t)nf * LPCN_ROWS_B * 4, b->active, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(b->d_lpc, (size_t)nf * LPCN_LPC_ORDER * 4, lpc + (size_t)f0 * LPCN_LPC_ORDER, (size_t)n_frames * LPCN_LPC_ORDER * 4,
                                 (size_t)nf * LPCN_LPC_ORDER * 4, b->active, hipMemcpyHostToDevice, st));
        if (b->timing) HIP_TRY(hipEventRecord(b->ev[1], st));
        rc = launch_sample(b, whole_batch(b), st, b->d_pcm + (size_t)f0 * LPCN_FRAME_SIZE, (size_t)n_frames * LPCN_FRAME_SIZE, nf, preload, false);
        if (rc) return rc;
        if (b->timing) {
            HIP_TRY(hipEventRecord(b->ev[2], st));
            HIP_TRY(hipEventSynchronize(b->ev[2]));
            HIP_TRY(hipEventElapsedTime(&b->ms_sample, b->ev[1], b->ev[2]));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipMemcpyAsync(pcm, b->d_pcm, npcm * sizeof(short), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lpcn_batch_dev_run_frames_host(lpcn_batch_dev *b, const float *features, int feat_stride,
                                              float *cond_a, float *cond_b, float *lpc, int n_frames)
{
    forget_keep(b);
    if (n_frames <= 0 || feat_stride < LPCN_NB_FEAT) { snprintf(g_err, sizeof(g_err), "bad run arguments"); return LPCN_E_ARG; }
    if (!b->active) return 0;
    DeviceGuard guard(b->e->device);
    const size_t nfeat = (size_t)b->active * n_frames * feat_stride;
    int rc = ensure_staging(b, nfeat, 0);
    if (rc) return rc;
    hipStream_t st = b->e->stream;
    if ((rc = order_begin(b, st))) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_feat, features, nfeat * sizeof(float), hipMemcpyHostToDevice, st));
    for (int f0 = 0; f0 < n_frames; f0 += b->max_chunk) {
        const int nf = n_frames - f0 < b->max_chunk ? n_frames - f0 : b->max_chunk;
        rc = launch_frames(b, whole_batch(b), st, b->d_feat + (size_t)f0 * feat_stride, feat_stride, (size_t)n_frames * feat_stride, nf);
        if (rc) return rc;
        if (cond_a) HIP_TRY(hipMemcpy2DAsync(cond_a + (size_t)f0 * LPCN_ROWS_A, (size_t)n_frames * LPCN_ROWS_A * 4, b->d_cond_a, (size_t)nf * LPCN_ROWS_A * 4,
                                             (size_t)nf * LPCN_ROWS_A * 4, b->active, hipMemcpyDeviceToHost, st));
        if (cond_b) HIP_TRY(hipMemcpy2DAsync(cond_b + (size_t)f0 * LPCN_ROWS_B, (size_t)n_frames * LPCN_ROWS_B * 4, b->d_cond_b, (size_t)nf * LPCN_ROWS_B * 4,
                                             (size_t)nf * LPCN_ROWS_B * 4, b->active, hipMemcpyDeviceToHost, st));
        if (lpc) HIP_TRY(hipMemcpy2DAsync(lpc + (size_t)f0 * LPCN_LPC_ORDER, (size_t)n_frames * LPCN_LPC_ORDER * 4, b->d_lpc, (size_t)nf * LPCN_LPC_ORDER * 4,
                                          (size_t)nf * LPCN_LPC_ORDER * 4, b->active, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}
